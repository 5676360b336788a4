// swc_common.h -- shared declarations for the MI355X decode engine (device code + host launcher).
//
// The per-lane decoders in this directory are written as plain sequential C++ ("one lane = one
// compressed stream") so that the same source compiles for gfx950 (hipcc) and, with
// -DSWC_HOST_EMULATION, for the host (g++) where tests/ run every lane of a wave sequentially and
// compare against the oracle without a GPU.  The host build is test infrastructure only; the
// shipped library contains the device build and nothing else.
#ifndef SWC_COMMON_H
#define SWC_COMMON_H

#include <stdint.h>
#include <stddef.h>
#include "../../include/swc_status.h"

#if defined(__HIPCC__) && !defined(SWC_HOST_EMULATION)
#include <hip/hip_runtime.h>
#define SWC_HD __host__ __device__ __forceinline__
#define SWC_D __device__ __forceinline__
#else
#define SWC_HD inline
#define SWC_D inline
#endif

// Makes a value opaque to the optimiser at no run-time cost.  Used where register-resident tables are read through
// select trees: without it LLVM folds `c ? a[i] : a[j]` into a load at a DYNAMIC offset, which pins the whole
// table (and the struct around it) in scratch memory instead of VGPRs.
#if defined(__HIP_DEVICE_COMPILE__)
#define SWC_OPAQUE(x) asm("" : "+v"(x))
#define SWC_OPAQUE_S(x) asm("" : "+s"(x))   // the same for a wave-uniform value (stays in a scalar register)
#else
#define SWC_OPAQUE(x) ((void)0)
#define SWC_OPAQUE_S(x) ((void)0)
#endif

namespace swc {

constexpr int kWave = 64;  // CDNA wavefront width; LDS tables are interleaved at this stride

// One decode job.  Layout == `swc_job` of include/swc_hip.h (checked by static_assert in api.cpp).
struct Job {
    const uint8_t* in;
    uint64_t in_len;
    uint8_t* out;
    uint64_t out_cap;
    uint64_t out_len;      // result: bytes produced (or required, for SWC_E_CAPACITY on size-countable codecs)
    uint64_t in_consumed;  // result: bytes of `in` consumed (after the caller-side align())
    int32_t status;        // result: swc_status
    int32_t aux;           // codec specific input (LZMA2: dictionary-size byte; LZMA: packed lc/lp/pb; LZ4: unused)
    const uint8_t* dict;   // optional prefix dictionary (LZ4) / reserved
    uint64_t dict_len;     // LZ4: dictionary length; LZMA: declared uncompressed size (or ~0 = unknown)
};

// aux of an LZ4 block job (include/swc_hip.h: SWC_LZ4_LINKED, SWC_LZ4_STORED)
constexpr int32_t kLz4Linked = 1, kLz4Stored = 2;
// aux of a Deflate job (include/swc_hip.h: SWC_DEFLATE_JOINED, SWC_DEFLATE_OPEN, SWC_DEFLATE_LINKED)
constexpr int32_t kDeflateJoined = 1, kDeflateOpen = 2, kDeflateLinked = 4;
// aux of an LZMA2 job above its dictionary-size byte (include/swc_hip.h: SWC_LZMA2_OPEN)
constexpr int32_t kLzma2Open = 0x100;

// A kernel's results back to its entry of the job list (AUX: `aux` too -- bzip2's block CRC)
template <bool AUX = false>
SWC_D void put_result(Job* jobs, uint32_t g, const Job& job) {
    jobs[g].out_len = job.out_len;
    jobs[g].in_consumed = job.in_consumed;
    jobs[g].status = job.status;
    if (AUX) jobs[g].aux = job.aux;
}

SWC_HD uint32_t brev32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(x);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    return (x >> 16) | (x << 16);
#endif
}

// ---- per-lane bit helpers: one instruction (or a few) on the device, portable C on the host; the cross-lane steps and the
// atomics are in simt.h
SWC_HD uint32_t funnel32(uint32_t hi, uint32_t lo, uint32_t sh) {  // bits [sh, sh + 32) of hi:lo; only sh % 32 counts
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31u));
#endif
}
SWC_HD uint32_t bfe32(uint32_t v, uint32_t off, uint32_t width) {   // only off % 32 and width % 32 count; width 0 -> 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ubfe(v, off, width);
#else
    off &= 31u; width &= 31u;
    return width == 0 ? 0u : (v >> off) & ((1u << width) - 1u);
#endif
}
SWC_HD uint32_t sbfe1(uint32_t v, uint32_t bit) {   // all ones if the bit is set
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_sbfe((int)v, bit, 1u);
#else
    return (v >> bit) & 1u ? 0xFFFFFFFFu : 0u;
#endif
}
SWC_HD uint32_t bfi32(uint32_t m, uint32_t a, uint32_t b) {   // (a & m) | (b & ~m) as v_bfi_b32 (the optimiser turns the C form into a compare and a select when m is a sign mask)
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t d;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(d) : "v"(m), "v"(a), "v"(b));
    return d;
#else
    return (a & m) | (b & ~m);
#endif
}
// bytes [n, n + 4) of hi:lo, n = nbytes % 4 (v_alignbyte_b32 takes the shift from the low bits of a byte address: lz_copy.h and
// lz4_wave.h build LDS reads at any alignment from aligned dwords with it)
SWC_HD uint32_t alignbyte32(uint32_t hi, uint32_t lo, uint32_t nbytes) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, nbytes);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (nbytes & 3u)));
#endif
}
// (a << K) + b as ONE instruction (v_lshl_add_u32): the optimiser otherwise regroups sums of shifted terms into more of them
template <int K>
SWC_HD uint32_t lshl_add(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t d;
    asm("v_lshl_add_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "n"(K), "v"(b));
    return d;
#else
    return (a << K) + b;
#endif
}
// the same with the shift in a register (only k % 32 counts)
SWC_HD uint32_t lshl_add_v(uint32_t a, uint32_t k, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t d;
    asm("v_lshl_add_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(k), "v"(b));
    return d;
#else
    return (a << (k & 31u)) + b;
#endif
}
// (a & m) | o as ONE instruction (v_and_or_b32) with both constants in registers (a VOP3 instruction of gfx9 takes no literal)
SWC_HD uint32_t and_or(uint32_t a, uint32_t m, uint32_t o) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t d;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(m), "v"(o));
    return d;
#else
    return (a & m) | o;
#endif
}
// m ? 0 : b for a mask m of all ones or all zeros (v_bfi_b32 with the constant 0: the optimiser turns the C form into a compare and a select)
SWC_HD uint32_t clear_if(uint32_t m, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t d;
    asm("v_bfi_b32 %0, %1, 0, %2" : "=v"(d) : "v"(m), "v"(b));
    return d;
#else
    return b & ~m;
#endif
}
// a * k + b, a signed 24-bit multiply-add (v_mad_i32_i24)
SWC_HD uint32_t mad24(uint32_t a, int32_t k, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(k), "v"(b));
    return d;
#else
    return (uint32_t)((int32_t)a * k) + b;
#endif
}
SWC_HD uint32_t log2u(uint32_t v) {   // floor(log2 v), v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 31u - (uint32_t)__clz((int)v);
#else
    return 31u - (uint32_t)__builtin_clz(v);
#endif
}
SWC_HD uint32_t mod_small(uint32_t m, uint32_t d) {   // m % d for m, d < 2^16, d != 0
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t q = (uint32_t)((float)m * __builtin_amdgcn_rcpf((float)d));   // v_rcp_f32: off by at most one, fixed up below
    uint32_t r = m - q * d;
    if ((int32_t)r < 0) r += d;
    if (r >= d) r -= d;
    return r;
#else
    return m % d;
#endif
}

// Pointers into HBM.  On the device they carry the global address space so that the compiler emits
// global_load/global_store instead of FLAT instructions (pointers loaded from a job record are generic
// otherwise; FLAT ops tie up both vmcnt and lgkmcnt and serialise against the LDS table reads).
#if defined(__HIP_DEVICE_COMPILE__)
#define SWC_AS_GLOBAL __attribute__((address_space(1)))
#else
#define SWC_AS_GLOBAL
#endif
typedef const SWC_AS_GLOBAL uint8_t* gcptr;
typedef SWC_AS_GLOBAL uint8_t* gptr;
typedef uint32_t __attribute__((aligned(1), may_alias)) u32_unaligned;
typedef uint64_t __attribute__((aligned(1), may_alias)) u64_unaligned;
typedef uint16_t __attribute__((aligned(1), may_alias)) u16_unaligned;

// gfx950 global loads/stores are unaligned-capable (hipcc emits plain global_load_dword for these)
SWC_HD uint32_t load_u32(gcptr p) { return *(const SWC_AS_GLOBAL u32_unaligned*)p; }
SWC_HD uint64_t load_u64(gcptr p) { return *(const SWC_AS_GLOBAL u64_unaligned*)p; }
SWC_HD void store_u32(gptr p, uint32_t v) { *(SWC_AS_GLOBAL u32_unaligned*)p = v; }
SWC_HD void store_u64(gptr p, uint64_t v) { *(SWC_AS_GLOBAL u64_unaligned*)p = v; }
SWC_HD void store_u64_stream(gptr p, uint64_t v) {   // past the caches: for data that is read once, much later
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_nontemporal_store(v, (SWC_AS_GLOBAL uint64_t*)p);
#else
    store_u64(p, v);
#endif
}
struct __attribute__((packed, may_alias)) u128_any { uint32_t x, y, z, w; };
SWC_HD void store_u128_a4(gptr p, uint32_t x, uint32_t y, uint32_t z, uint32_t w) { *(SWC_AS_GLOBAL u128_any*)p = u128_any{x, y, z, w}; }   // 16 bytes at any alignment
SWC_HD u128_any load_u128(gcptr p) { return *(const SWC_AS_GLOBAL u128_any*)p; }   // likewise (global_load_dwordx4)

// Workgroup barrier of the group-per-stream checksum kernels.  The host emulation build runs the T "threads" of a group
// as real host threads and plugs its own barrier in here (tests/host_emu/emu.cpp).
#if defined(__HIP_DEVICE_COMPILE__)
SWC_D void group_sync() { __syncthreads(); }
#elif defined(SWC_HOST_EMULATION)
inline thread_local void (*emu_group_sync)() = nullptr;
SWC_D void group_sync() { if (emu_group_sync) emu_group_sync(); }
#else
SWC_D void group_sync() {}
#endif

// Per-lane view of an LDS region interleaved at wave stride: word j of this lane lives at
// base[j * 64 + lane], so any per-lane index pattern is bank-conflict free for 32-bit accesses
// (bank = lane % 32, the two 32-lane halves are serviced separately).
struct LaneLds {
    uint32_t* p;  // base + stream column
    int stride;   // streams per wave (64 when every lane owns a stream)
    SWC_HD uint32_t get(int j) const { return p[j * stride]; }
    SWC_HD void set(int j, uint32_t v) const { p[j * stride] = v; }
};

}  // namespace swc
#endif
