// host_util.h -- small host-side helpers shared by the C-ABI translation units.
#ifndef SWC_HOST_UTIL_H
#define SWC_HOST_UTIL_H

#include <hip/hip_runtime.h>
#include <chrono>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "swc_common.h"
#include "../../include/swc_hip.h"

namespace swc {

// RAII device allocation from the stream-ordered pool, on the calling thread's own stream (hipStreamPerThread: concurrent
// callers do not serialise on the default stream) (hipMalloc / hipFree cost milliseconds
// each, which dominated the single-shot calls: 9.4 ms for one 64 KiB block; the pool keeps up to 1 GiB cached, see
// device_ready()).  ok() is false when the allocation failed (=> SWC_E_DEVICE, never a CPU fallback).
class DevBuf {
public:
    DevBuf() : p_(nullptr), n_(0) {}
    explicit DevBuf(size_t n) : p_(nullptr), n_(0) { alloc(n); }
    ~DevBuf() { release(); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    bool alloc(size_t n) {
        release();
        if (n == 0) n = 1;
        if (hipMallocAsync(&p_, n, hipStreamPerThread) != hipSuccess) { p_ = nullptr; (void)hipGetLastError(); return false; }
        n_ = n;
        return true;
    }
    void release() {
        if (p_) (void)hipFreeAsync(p_, hipStreamPerThread);
        p_ = nullptr; n_ = 0;
    }
    bool ok() const { return p_ != nullptr; }
    uint8_t* u8() const { return static_cast<uint8_t*>(p_); }
    void* ptr() const { return p_; }
    size_t size() const { return n_; }
private:
    void* p_;
    size_t n_;
};

// Page-locked host staging memory of the calling thread, kept between calls (pageable hipMemcpy was most of a small
// single-shot call).  nullptr if the allocation fails (the caller falls back to its own pageable buffer).
uint8_t* pinned_stage(int which, size_t n);
// A staging buffer above "pinned_keep_mib" goes back when the call that needed it is over: run_units does this itself; a call that
// staged something and never reaches run_units does it here
void pinned_trim();

// Host result handed to the caller (released with swc_free).  Large results come from -- and go back to -- a small cache
// of buffers whose pages are already mapped (api.cpp): a fresh 268 MB allocation costs more in page faults (24 ms) than the
// PCIe transfer that fills it (5 ms).
uint8_t* host_result(size_t n);
void host_result_free(void* p);

bool device_is_gfx950(int dev);  // api.cpp: device `dev` exists and is a gfx950 (also prepares its memory pool, once)
bool device_ready();  // api.cpp: true when a gfx950 device is present and selected

constexpr int kSumSha256 = 6;   // HostUnit::sum_kind: SHA-256 (behind the swc_checksum kinds)

// One unit of work for the host-side batch runner (host pointers; the runner stages to HBM).
struct HostUnit {
    const uint8_t* in = nullptr;
    size_t in_len = 0;
    // Optional: the host buffer `in` points into (a container, a multi-member file).  Units with the same base are staged
    // ONCE and address their sub-range of it -- not each its own copy of everything behind its start.
    const uint8_t* base = nullptr;
    size_t base_len = 0;
    // Optional: `base` is in HBM already, here (the caller keeps it until run_units returns): sub-ranges of it are not staged again
    const uint8_t* base_dev = nullptr;
    size_t cap_hint = 0;         // 0 = use the codec's default policy
    bool cap_exact = false;      // cap_hint is authoritative (declared size): do not grow
    int32_t aux = 0;
    const uint8_t* dict = nullptr;
    size_t dict_len = 0;
    // LZ4: the prefix is staged directly in front of the unit's output, so that it is history in place (swc_hip.h: an adjacent prefix)
    bool dict_adjacent = false;
    // LZ4: the unit is part of a chain (its head, or a unit with SWC_LZ4_LINKED right behind its predecessor in the list).  The
    // runner lays the outputs of a chain out back to back and never launches one of its units again on its own: a status that
    // would otherwise mean "once more with more room" (SWC_E_CAPACITY, SWC_E_NEED_WORKSPACE) is the caller's to act on.
    bool chain = false;
    // Deflate: the unit is part of a RUN -- the units one stream was cut into at its flush points (framing_deflate.cpp), `chain` set on
    // all of them, SWC_DEFLATE_JOINED on all but the head.  run_len: on the head, the number of units of the run (0 on the others).
    size_t run_len = 0;
    uint64_t extra = 0;          // codec specific (goes to Job::dict_len when dict == nullptr)
    uint64_t dict_value = 0;     // codec specific integer carried in Job::dict when dict == nullptr (LZMA: dictionary size)
    // Optional: where the output is wanted (a place inside the caller's final buffer, `dst_cap` bytes of room).  If the
    // unit's output fits it is copied THERE from the pinned staging buffer -- once -- and `out` stays empty (in_dst, out_size).
    uint8_t* dst = nullptr;
    size_t dst_cap = 0;
    // Optional: a checksum of the output computed ON THE DEVICE in the same launch sequence (swc_checksum kinds of
    // include/swc_hip.h: 1 CRC-32, 2 Adler-32, 3 CRC-64, 4 bzip2 CRC-32, 5 XXH32; kSumSha256, internal: SHA-256, swc_batch_sha256's
    // kernel); one kind per run_units call.
    int sum_kind = 0;
    // ... of the unit's INPUT instead (the encoders: the check of an .xz block is of what went in): taken over a view of the staged
    // input; all units of a call that ask for a checksum agree on this
    bool sum_of_input = false;
    // results
    std::vector<uint8_t> out;
    bool in_dst = false;         // the output is at `dst`, not in `out`
    size_t out_size = 0;         // bytes of output (wherever they are)
    uint64_t sum = 0;            // the checksum, if sum_valid (kinds 1-5)
    uint8_t digest[32] = {0};    // the SHA-256, if sum_valid (kind 6)
    bool sum_valid = false;
    const uint8_t* data() const { return in_dst ? dst : out.data(); }
    size_t size() const { return in_dst ? out_size : out.size(); }
    size_t in_consumed = 0;
    int32_t status = SWC_OK;
    int32_t aux_out = 0;         // codec specific result (bzip2: computed block CRC; Deflate: SWC_DEFLATE_OPEN, LZMA2: SWC_LZMA2_OPEN where the unit ended open)
    // results of a Deflate run, on its head: the units in front of unit run_used ended open at their last byte; run_ok: unit run_used
    // met a final block, and the head's output is the stream's -- run_bytes of it (out_size stays the head's own share)
    bool run_ok = false;
    size_t run_used = 0, run_bytes = 0;
    uint64_t need = 0;           // Deflate run units: out_len as the job reported it (the room it needs, for SWC_E_CAPACITY)
};

// Stage units to HBM, run ONE batched launch of `codec` (re-launching only the units that reported
// SWC_E_CAPACITY with a larger buffer), fetch the results.  Returns SWC_OK or SWC_E_DEVICE.
int run_units(int codec, std::vector<HostUnit>& units);

// SWC_TRACE=1 in the environment: the host-side stages of a call with their wall-clock times, on stderr
struct Trace {
    bool on;
    std::chrono::steady_clock::time_point t0, last;
    Trace() { static const bool e = getenv("SWC_TRACE") != nullptr; on = e; t0 = last = std::chrono::steady_clock::now(); }
    void mark(const char* what, size_t bytes = 0) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[swc] %-28s %8.3f ms  (%zu bytes)\n", what, std::chrono::duration<double, std::milli>(now - last).count(), bytes);
        last = now;
    }
};

// swc_stat counters (api.cpp), named as swc_stat's keys
enum Stat { kStatLaunches, kStatUnits, kStatXzCacheHits, kStatDeflateUnitFallbacks, kStatSha256DeviceUnits, kStatLzma2RunUnits,
            kStatLzma2RunFallbacks, kStatGzipScanMembers, kStatGzipScanWalked, kStatBzip2ScanMarks,
            kStatBzip2ScanFiles, kStatCount };
void stat_add(Stat which, long long v);

}  // namespace swc
#endif
