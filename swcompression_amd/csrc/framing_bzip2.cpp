// framing_bzip2.cpp -- host side of BZip2: stream header, block discovery, CRC chaining.
//   BZip2.decompress(data:) / decompress(_ bitReader:)   reference Sources/BZip2/BZip2.swift:22-26, 50-95
//   BZip2.multiDecompress(data:)                          :40-48
//   BlockSize.init?                                       Sources/BZip2/BZip2+BlockSize.swift:29-52
// bzip2 blocks start at arbitrary BIT offsets and carry no length, so the sequential reference only
// learns where block k+1 starts after decoding block k.  Here the host scans the input for every
// occurrence of the 48-bit block magic, hands ALL candidates to one batched device launch, and then
// replays the reference's sequential walk over the results: a candidate is used only if the walk
// arrives exactly at its bit offset, so false positives inside block data are simply never visited
// and the outcome (bytes, error, error order) is identical to the sequential decoder.
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <map>
#include <memory>
#include <thread>
#include <system_error>
#include <vector>
#include "framing.h"
#include "launch.h"
#include "bzip2_scan.h"

namespace swc {
namespace {

constexpr uint64_t kBlockMagic = 0x314159265359ull;
constexpr uint64_t kEosMagic = 0x177245385090ull;

inline uint64_t read_bits(const uint8_t* d, uint64_t bit, int count) {  // MSB-first, count <= 56, caller checked bounds
    uint64_t v = 0;
    for (int i = 0; i < count; i++) {
        const uint64_t p = bit + i;
        v = (v << 1) | ((d[p >> 3] >> (7 - (p & 7))) & 1u);
    }
    return v;
}

// every bit offset (>= from_bit) at which the 48-bit block magic occurs, in increasing order.
// Discovery is the host's share of a bzip2 decode and must not be slower than the device: per BYTE position one big-endian
// 64-bit window is compared against the magic at its eight bit alignments (48 + 7 bits fit), and large inputs are cut into
// ranges scanned by several threads (a magic is found by the range that holds its first bit).
// Ends: the magic of the end of a stream is looked for as well, and reported with kEndFound set in its offset (kind 10; without it
// the loop is the one it was).
constexpr uint64_t kEndFound = (uint64_t)1 << 63;
template <bool Ends>
void scan_range(const uint8_t* d, size_t n, size_t lo, size_t hi, uint64_t from_bit, std::vector<uint64_t>& out) {
    for (size_t i = lo; i < hi; i++) {
        if (i + 6 > n) break;                        // fewer than 48 bits left
        uint64_t v = 0;
        const size_t take = n - i < 8 ? n - i : 8;
        for (size_t k = 0; k < take; k++) v |= (uint64_t)d[i + k] << (56 - 8 * k);
        for (int s = 0; s < 8; s++) {
            const uint64_t w = (v >> (16 - s)) & 0xFFFFFFFFFFFFull;
            if (w != kBlockMagic && !(Ends && w == kEosMagic)) continue;
            if (s > 0 && i + 7 > n) continue;        // the last bits would lie past the end
            const uint64_t start = (uint64_t)i * 8 + (uint64_t)s;
            if (start >= from_bit) out.push_back(!Ends || w == kBlockMagic ? start : start | kEndFound);
        }
    }
}
template <bool Ends = false>
void scan_block_magics(const uint8_t* d, size_t n, uint64_t from_bit, std::vector<uint64_t>& out) {
    if (n < 6) return;
    const size_t kMinPerThread = (size_t)4 << 20;
    size_t threads = n / kMinPerThread;
    const size_t hw = std::thread::hardware_concurrency();
    if (threads > 16) threads = 16;
    if (hw && threads > hw) threads = hw;
    if (threads < 2) { scan_range<Ends>(d, n, 0, n, from_bit, out); return; }
    std::vector<std::vector<uint64_t>> found(threads);
    std::vector<std::thread> pool;
    const size_t per = (n + threads - 1) / threads;
    size_t started = 0;
    try {
        for (size_t t = 0; t < threads; t++) {
            pool.emplace_back([&, t] { scan_range<Ends>(d, n, t * per, std::min(n, (t + 1) * per), from_bit, found[t]); });
            started = t + 1;
        }
    } catch (const std::system_error&) {}   // no more threads to be had: this one scans the ranges nobody took
    for (size_t t = started; t < threads; t++) scan_range<Ends>(d, n, t * per, std::min(n, (t + 1) * per), from_bit, found[t]);
    for (auto& th : pool) th.join();
    for (auto& f : found) out.insert(out.end(), f.begin(), f.end());
}

struct Decoded {
    int status;
    std::vector<uint8_t> out;
    uint64_t end_bit;
};

// decompress(_:) BZip2.swift:50-95 replayed over pre-decoded blocks.  `byte_pos` is the aligned start of
// the stream; on return it is the aligned position just past the stream (callers align(), :45).
// The four bytes in front of the blocks (:53-66): what the walk answers before it looks at a block, or SWC_OK.
int stream_header(const uint8_t* d, size_t n, size_t byte_pos) {
    if ((uint64_t)n * 8 - (uint64_t)byte_pos * 8 < 32) return SWC_E_BZIP2_WRONG_MAGIC;        // :53
    if (!(d[byte_pos] == 0x42 && d[byte_pos + 1] == 0x5A)) return SWC_E_BZIP2_WRONG_MAGIC;   // "BZ" :59-60
    if (d[byte_pos + 2] != 104) return SWC_E_BZIP2_WRONG_VERSION;                  // 'h' :62-63
    if (d[byte_pos + 3] < 0x31 || d[byte_pos + 3] > 0x39) return SWC_E_BZIP2_WRONG_BLOCK_SIZE;  // :65-66
    return SWC_OK;
}

int walk_stream(const uint8_t* d, size_t n, size_t& byte_pos, const std::map<uint64_t, Decoded>& blocks,
                std::vector<uint8_t>& out) {
    const uint64_t total = (uint64_t)n * 8;
    uint64_t cur = (uint64_t)byte_pos * 8;
    if (const int st = stream_header(d, n, byte_pos)) return st;
    cur += 32;
    uint32_t total_crc = 0;
    for (;;) {
        if (total - cur < 80) return SWC_E_BZIP2_WRONG_MAGIC;                     // :71
        const uint64_t type = read_bits(d, cur, 48);
        const uint32_t crc = (uint32_t)read_bits(d, cur + 48, 32);
        if (type == kBlockMagic) {
            auto it = blocks.find(cur);
            if (it == blocks.end()) return SWC_E_DEVICE;                           // cannot happen: every magic was scanned
            const Decoded& b = it->second;
            if (b.status != SWC_OK && b.status != SWC_E_BZIP2_WRONG_CRC) return b.status;
            out.insert(out.end(), b.out.begin(), b.out.end());
            if (b.status == SWC_E_BZIP2_WRONG_CRC) return SWC_E_BZIP2_WRONG_CRC;   // :81 carries everything so far
            total_crc = (total_crc << 1) | (total_crc >> 31);                      // :83-84
            total_crc ^= crc;
            cur = b.end_bit;
        } else if (type == kEosMagic) {
            if (total_crc != crc) return SWC_E_BZIP2_WRONG_CRC;                    // :86
            cur += 80;
            break;
        } else {
            return SWC_E_BZIP2_WRONG_BLOCK_TYPE;                                   // :89
        }
    }
    byte_pos = (size_t)((cur + 7) >> 3);
    return SWC_OK;
}

}  // namespace

// Every bit offset at which the block magic occurs (candidates: a magic inside block data is possible).
void bzip2_magic_index(const uint8_t* in, size_t in_len, std::vector<BlockRef64>& out) {
    std::vector<uint64_t> cand;
    scan_block_magics(in, in_len, 32, cand);
    for (uint64_t c : cand) out.push_back({c, 0, 0, 0});
}

// The marks of include/swc_hip.h (swc_index_blocks kind 10) on the host: what launch_bzip2_index leaves on the device.
void bzip2_mark_index(const uint8_t* in, size_t in_len, std::vector<BlockRef64>& out) {
    std::vector<uint64_t> cand;
    scan_block_magics<true>(in, in_len, 32, cand);
    const uint64_t total = (uint64_t)in_len * 8;
    const size_t first = out.size();
    for (uint64_t c : cand) {
        const uint64_t b = c & ~kEndFound;
        if (total - b < 80) continue;   // (the walk reports wrongMagic there before it looks)
        if (out.size() > first) out.back().comp_len = b - out.back().offset;
        out.push_back({b, total - b, 0, (uint32_t)read_bits(in, b + 48, 32), (c & kEndFound) ? 1u : 0u});
    }
}

// ---- block marks found on the device (csrc/bzip2_scan.h) ---------------------------------------------------------
static std::atomic<int> g_bzip2_scan_bytes{0};
void set_bzip2_scan_bytes(int v) { g_bzip2_scan_bytes = v; }

// The file staged once and indexed on the device: `cand` = the bit offsets of its block marks, every one checked against the host
// copy; the staged copy joins `keep` (its units address it, HostUnit::base_dev).  False: no device memory, a failed call, a ref
// that is not what the file says -- the host scans, and of this attempt only the launches it issued stay counted ("launches" counts
// what ran).  Where no run_units call follows -- the attempt failed, or the file holds no block -- the pinned stage is trimmed here.
static bool bzip2_scan_device(const uint8_t* d, size_t n, std::vector<uint64_t>& cand, Bzip2Staged& keep, const uint8_t*& staged) {
    if (n < bzscan::kLeast || !device_ready()) return false;
    hipStream_t stream = hipStreamPerThread;
    std::unique_ptr<DevBuf> d_in(new DevBuf(n + 16));
    if (!d_in->ok()) return false;
    struct Trim { bool on = true; ~Trim() { if (on) pinned_trim(); } } trim;   // (runs after every synchronize below)
    uint8_t* up = pinned_stage(0, n);
    if (up) memcpy(up, d, n);
    if (hipMemcpyAsync(d_in->ptr(), up ? up : d, n, hipMemcpyHostToDevice, stream) != hipSuccess) { (void)hipGetLastError(); return false; }
    std::vector<swc_block_ref> found;
    uint64_t cap = std::max<uint64_t>(4096, n / 4096);
    for (int turn = 0;; turn++) {   // (a second turn for a file with more marks than the first had room for: there cap = what it counted)
        const size_t ws_bytes = swc_bzip2_index_workspace_bytes(n, cap);
        DevBuf d_refs(cap * sizeof(swc_block_ref) + sizeof(uint64_t)), d_ws(ws_bytes);
        if (!d_refs.ok() || !d_ws.ok()) { (void)hipStreamSynchronize(stream); return false; }
        uint64_t* d_n = reinterpret_cast<uint64_t*>(d_refs.u8() + cap * sizeof(swc_block_ref));
        swc_batch_opts opts = {-1, stream, 0, 0};
        uint64_t m = 0;
        const bool issued = swc_batch_bzip2_index(d_in->u8(), n, reinterpret_cast<swc_block_ref*>(d_refs.ptr()), cap, d_n, d_ws.ptr(), ws_bytes, &opts) == SWC_OK &&
                            hipMemcpyAsync(&m, d_n, sizeof m, hipMemcpyDeviceToHost, stream) == hipSuccess;
        if (hipStreamSynchronize(stream) != hipSuccess || !issued) { (void)hipGetLastError(); return false; }   // (nothing of this call in flight any more)
        stat_add(kStatLaunches, 1);
        if (m > cap) {
            if (turn || m > bzscan::most(n)) return false;
            cap = m;
            continue;
        }
        found.resize((size_t)m);
        if (m && (hipMemcpyAsync(found.data(), d_refs.ptr(), (size_t)m * sizeof(swc_block_ref), hipMemcpyDeviceToHost, stream) != hipSuccess ||
                  hipStreamSynchronize(stream) != hipSuccess)) { (void)hipGetLastError(); return false; }
        break;
    }
    // (a ref is checked against the file before it is used: nothing the device says is trusted with an address)
    const uint64_t total = (uint64_t)n * 8;
    std::vector<uint64_t> blocks;
    uint64_t behind = 32;   // the least offset the next ref may have
    for (const swc_block_ref& r : found) {
        if (r.offset < behind || r.offset > total - 80) return false;
        const uint64_t magic = read_bits(d, r.offset, 48);
        if (magic != ((r.flags & 1) ? kEosMagic : kBlockMagic)) return false;
        behind = r.offset + 1;
        if (!(r.flags & 1)) blocks.push_back(r.offset);
    }
    cand = std::move(blocks);
    stat_add(kStatBzip2ScanFiles, 1);
    stat_add(kStatBzip2ScanMarks, (long long)cand.size());
    staged = d_in->u8();
    keep.files.push_back(std::move(d_in));
    trim.on = cand.empty();   // (units follow: run_units trims)
    return true;
}

// Units for every candidate block of `d` (appended to `units`; `used` receives their bit offsets).  `keep`: the copy of the file in
// HBM that the units address where the marks were found there ("bzip2_scan_bytes"); it lives until run_units has returned.
void bzip2_collect_candidates(const uint8_t* d, size_t n, std::vector<HostUnit>& units, std::vector<uint64_t>& used, Bzip2Staged& keep) {
    if (stream_header(d, n, 0) != SWC_OK) return;   // (the walk stops in front of the first block: no candidate is ever visited, and the answer needs no device)
    std::vector<uint64_t> cand;
    const uint8_t* staged = nullptr;
    const int least = g_bzip2_scan_bytes.load();
    if (!(least > 0 && n >= (size_t)least && bzip2_scan_device(d, n, cand, keep, staged))) scan_block_magics(d, n, 32, cand);
    // first capacity of a block: what the stream header's level allows for the BWT column (level x 100,000 bytes,
    // BZip2+BlockSize.swift:11-33) -- the output is larger only where RLE1 runs expand, and such blocks are relaunched with
    // the size they report
    const size_t level = (n >= 4 && d[0] == 0x42 && d[1] == 0x5A && d[2] == 104 && d[3] >= 0x31 && d[3] <= 0x39) ? (size_t)(d[3] - 0x30) : 9;
    for (uint64_t c : cand) {
        if ((uint64_t)n * 8 - c < 80) continue;                                    // the walk reports wrongMagic there
        HostUnit u;
        u.in = d;
        u.in_len = n;
        if (staged) { u.base = d; u.base_len = n; u.base_dev = staged; }         // the copy the index read: not staged again
        u.extra = c + 80;                                                         // bit offset of the block body
        u.dict_value = read_bits(d, c + 48, 32);                                  // stored block CRC
        u.cap_hint = std::min<size_t>(level * 100000 + 64, std::max<size_t>(4096, n * 64));
        units.push_back(std::move(u));
        used.push_back(c);
    }
}

namespace {
void build_blocks(std::vector<HostUnit>& units, size_t first_unit, const std::vector<uint64_t>& used, std::map<uint64_t, Decoded>& blocks) {
    for (size_t i = 0; i < used.size(); i++) {
        HostUnit& u = units[first_unit + i];
        Decoded dec;
        dec.status = u.status;
        dec.out = std::move(u.out);
        dec.end_bit = u.in_consumed;                                              // bits for this codec
        blocks.emplace(used[i], std::move(dec));
    }
}
}  // namespace

// The sequential walk of one stream over its decoded candidates units[first_unit .. first_unit + used.size()).
int bzip2_finish_stream(const uint8_t* d, size_t n, std::vector<HostUnit>& units, size_t first_unit, const std::vector<uint64_t>& used,
                        std::vector<uint8_t>& res, size_t& byte_pos) {
    std::map<uint64_t, Decoded> blocks;
    build_blocks(units, first_unit, used, blocks);
    return walk_stream(d, n, byte_pos, blocks, res);
}

namespace {

// Decode every candidate block of `d` on the device in one batch.
int decode_candidates(const uint8_t* d, size_t n, std::map<uint64_t, Decoded>& blocks) {
    std::vector<HostUnit> units;
    std::vector<uint64_t> used;
    Bzip2Staged keep;
    bzip2_collect_candidates(d, n, units, used, keep);
    if (!units.empty()) {
        int st = run_units(SWC_CODEC_BZIP2_BLOCK, units);
        if (st) return st;
    }
    build_blocks(units, 0, used, blocks);
    return SWC_OK;
}

}  // namespace
}  // namespace swc

namespace swc { int bzip2_compress_device(const uint8_t* data, size_t len, int level, uint8_t** out, size_t* out_len); }   // bzip2_compress.hip
using namespace swc;

extern "C" {

size_t swc_bzip2_index_workspace_bytes(uint64_t len, uint64_t cap) { return (size_t)bzscan::plan(len, cap).bytes + 8; }   // (+ 8: cut from the first 8-byte boundary)

int swc_batch_bzip2_index(const uint8_t* src, uint64_t len, swc_block_ref* refs, uint64_t cap, uint64_t* n, void* workspace, size_t workspace_bytes,
                          const swc_batch_opts* opts) try {
    static_assert(sizeof(swc_block_ref) == sizeof(bzscan::Ref) && offsetof(swc_block_ref, flags) == offsetof(bzscan::Ref, flags), "layout");
    if ((len && !src) || (cap && !refs) || !n || !workspace) return SWC_E_INVALID_ARGUMENT;
    if (workspace_bytes < swc_bzip2_index_workspace_bytes(len, cap)) return SWC_E_NEED_WORKSPACE;
    if (!device_ready()) return SWC_E_DEVICE;
    if (opts && opts->device >= 0 && hipSetDevice(opts->device) != hipSuccess) return SWC_E_DEVICE;
    hipStream_t stream = opts ? static_cast<hipStream_t>(opts->stream) : nullptr;
    uint8_t* ws = reinterpret_cast<uint8_t*>(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
    const hipError_t e = launch_bzip2_index(src, len, refs, cap, n, ws, stream);
    if (e == hipErrorInvalidValue) return SWC_E_INVALID_ARGUMENT;
    if (e != hipSuccess) return SWC_E_DEVICE;
    if (opts && opts->synchronize && hipStreamSynchronize(stream) != hipSuccess) return SWC_E_DEVICE;
    return SWC_OK;
} catch (...) {
    return SWC_E_DEVICE;
}

int swc_bzip2_decompress(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len, size_t* in_consumed) try {
    if (!out || !out_len || (in_len && !in)) return SWC_E_INVALID_ARGUMENT;
    std::map<uint64_t, Decoded> blocks;
    std::vector<uint8_t> res;
    int st = decode_candidates(in, in_len, blocks);
    if (st) { give_empty(out, out_len); return st; }
    size_t pos = 0;
    st = walk_stream(in, in_len, pos, blocks, res);
    if (st != SWC_OK && st != SWC_E_BZIP2_WRONG_CRC) res.clear();                  // only wrongCRC carries data
    if (in_consumed) *in_consumed = pos;
    give(res, out, out_len);
    return st;
} catch (...) {   // std::bad_alloc / length_error from a size taken from the input: never through the C boundary
    if (out && out_len) give_empty(out, out_len);
    return SWC_E_DEVICE;
}

int swc_bzip2_multi_decompress(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len, size_t** sizes, size_t* n_streams) try {
    if (!out || !out_len || !sizes || !n_streams || (in_len && !in)) return SWC_E_INVALID_ARGUMENT;
    std::map<uint64_t, Decoded> blocks;
    std::vector<uint8_t> all;
    std::vector<size_t> sz;
    int st = decode_candidates(in, in_len, blocks);
    if (st) { give_empty(out, out_len); *sizes = give_sizes(sz); *n_streams = 0; return st; }
    size_t pos = 0;
    while (pos < in_len) {                                                         // :43 !reader.isFinished
        std::vector<uint8_t> one;
        st = walk_stream(in, in_len, pos, blocks, one);
        if (st == SWC_E_BZIP2_WRONG_CRC) { all = std::move(one); sz.assign(1, all.size()); break; }  // carries the failing archive only
        if (st) { all.clear(); sz.clear(); break; }
        sz.push_back(one.size());
        all.insert(all.end(), one.begin(), one.end());
    }
    give(all, out, out_len);
    *sizes = give_sizes(sz);
    *n_streams = sz.size();
    return st;
} catch (...) {   // std::bad_alloc / length_error from a size taken from the input: never through the C boundary
    if (out && out_len) give_empty(out, out_len);
    if (sizes) *sizes = nullptr;
    if (n_streams) *n_streams = 0;
    return SWC_E_DEVICE;
}

// BZip2.compress(data:blockSize:) BZip2+Compress.swift:40-74 (BZip2.compress(data:) = block size one, :19-21)
int swc_bzip2_compress(const uint8_t* data, size_t len, int block_size, uint8_t** out, size_t* out_len) try {
    if (!out || !out_len || (len && !data) || block_size < 1 || block_size > 9) return SWC_E_INVALID_ARGUMENT;
    if (!device_ready()) { give_empty(out, out_len); return SWC_E_DEVICE; }
    const int st = bzip2_compress_device(data, len, block_size, out, out_len);   // assembled in the caller's buffer
    if (st) { give_empty(out, out_len); return st; }
    stat_add(kStatLaunches, 1);
    return SWC_OK;
} catch (...) {
    if (out && out_len) give_empty(out, out_len);
    return SWC_E_DEVICE;
}

}  // extern "C"
