// launch.h -- host-side launch wrappers implemented in kernels.hip (launch_inflate_team: inflate_team.hip; launch_lzma2_compress:
// lzma_compress.hip): which kernels, in which
// order, with which flags.  What a kernel does with its job is in job_kernels.h.
#ifndef SWC_LAUNCH_H
#define SWC_LAUNCH_H
#include <hip/hip_runtime.h>
#include "swc_common.h"
namespace swc {
// ws_off != nullptr: device array of n + 1 prefix-summed per-job workspace offsets (then ws_bytes is ignored)
// crcs != nullptr: device array of n words that the launch leaves as launch_crc32 would (the wave copy kernel folds the CRC-32 of
// a stream into its tail; behind the workgroup kernel the CRC kernels run)
hipError_t launch_inflate(Job* jobs, size_t n, void* ws, size_t ws_bytes, hipStream_t stream, const uint64_t* ws_off = nullptr, uint32_t* crcs = nullptr);
// inflate_team.hip: phase 1 with a team of wavefronts per stream (launches of few streams); `scratch`: inflate_team_scratch_bytes(n)
size_t inflate_team_scratch_bytes(size_t n);
hipError_t launch_inflate_team(Job* jobs, size_t n, uint8_t* ws, size_t stride, const uint64_t* ws_off, uint8_t* scratch, hipStream_t stream);
size_t inflate_ws_bytes_per_job(uint64_t cap);
hipError_t launch_crc32(const Job* jobs, size_t n, uint32_t* crcs, hipStream_t stream);
hipError_t launch_delta(Job* jobs, size_t n, hipStream_t stream);
hipError_t launch_checksum(int kind, const Job* jobs, size_t n, uint64_t* sums, hipStream_t stream);
// SHA-256 of every job's output (the coverage rule of the other sums): 32 bytes per job at `digests`, any alignment
hipError_t launch_sha256(const Job* jobs, size_t n, uint8_t* digests, hipStream_t stream);
void set_profile_buffer(void* p);
void set_phase_timing(int on);
void set_lzma_coder_cache(int on);
void set_lz_copier(int v);
void set_deflate_team(int v);
void set_bzip2_hot_cxx(int v);
void set_bzip2_team_walk(int v);
int last_phase_ms(float* ms, int cap);
hipError_t launch_lz4(Job* jobs, size_t n, void* ws, size_t ws_bytes, hipStream_t stream, const uint64_t* ws_off = nullptr);
size_t lz4_ws_bytes_per_job(uint64_t cap);
// the launch order of a batch on `stream` (kernels.hip: longest jobs first): perm[b] = the job of workgroup b, nullptr = the plain
// XCD-aware order of xcd_job
const uint32_t* job_order(const Job* jobs, size_t n, hipStream_t stream, bool chains = false);
hipError_t launch_lz4_compress(Job* jobs, size_t n, hipStream_t stream);
hipError_t launch_deflate_compress(Job* jobs, size_t n, hipStream_t stream);
hipError_t launch_deflate_compress_dynamic(Job* jobs, size_t n, hipStream_t stream);
// lzma_compress.hip: one LZMA2 run per wavefront (lzma_comp.h)
hipError_t launch_lzma2_compress(Job* jobs, size_t n, hipStream_t stream);
// bgzf_pack.h: the whole BGZF writer on `stream` (set-up, one compress launch, CRC-32, offsets, pack); `ws`: 16-byte aligned device
// memory of bgzf::plan(len, bs).bytes, the Result at its plan().res; eof: the end-of-file member behind the last one
hipError_t launch_bgzf_archive(const uint8_t* src, uint64_t len, uint32_t bs, bool dynamic, uint8_t* dst, uint64_t dst_cap, uint64_t* total,
                               uint64_t* sizes, uint8_t* ws, bool eof, hipStream_t stream);
// gzip_scan.h: the candidate members of a buffer on `stream` (count, offsets, starts, refs); `ws`: 8-byte aligned device memory of
// gzscan::plan(len, cap).bytes; *n (device) = the candidates found, refs (device, swc_block_ref) = the first min(*n, cap) of them
hipError_t launch_gzip_index(const uint8_t* src, uint64_t len, void* refs, uint64_t cap, uint64_t* n, uint8_t* ws, hipStream_t stream);
// bzip2_scan.h: the marks of a buffer (block and end-of-stream magics at any bit) on `stream`, as launch_gzip_index; `ws`: 8-byte aligned
// device memory of bzscan::plan(len, cap).bytes
hipError_t launch_bzip2_index(const uint8_t* src, uint64_t len, void* refs, uint64_t cap, uint64_t* n, uint8_t* ws, hipStream_t stream);
hipError_t launch_lzma(bool lzma2, Job* jobs, size_t n, void* spill, hipStream_t stream);
size_t lzma_spill_bytes_per_job();
hipError_t launch_bzip2(Job* jobs, size_t n, void* ws, size_t ws_bytes, hipStream_t stream);
size_t bzip2_ws_bytes_per_job(size_t lcap);
}
#endif
