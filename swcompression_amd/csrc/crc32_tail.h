// crc32_tail.h -- CRC-32 of a stream by the wave that has just written it: the tail of the Deflate copy kernel (lz_copy.h,
// kernels.hip: swc_lz_copy_crc32_kernel).
//
// When a copy wave has flushed the last byte of its stream, its LDS window is dead: the CRC tables go THERE -- no LDS is added
// to the kernel and no wave is lost -- and the wave folds its own output, read back from memory, while the other waves of the
// CU go on copying.  The arithmetic is that of crc32_wave.h (pieces of 32 bytes, piece 64 j + t to lane t, rows of 2 KB, front
// padding with zeros to whole rows, the initial value xor-ed into the first four data bytes, six fold levels at the end); what
// differs is where the constants live and how memory is read:
//   * WaveConsts is 9 KB, the window 6 KiB.  TailConsts is 6,144 bytes: a slice-by-TWO data table (2 KB: the same number of
//     look-ups per byte as slice-by-4, twice the dependent steps -- two rows are folded side by side to cover them) and the
//     four tables of the row shift G (4 KB).  Both are parts of WaveConsts in device memory (tab[0..1], tabg) and are copied
//     from there;
//   * the fold matrices are used once per stream and stay in device memory: wave-uniform (scalar) loads;
//   * the data is a stream that is read exactly once: loads that pass by the CU's L1 (see ld_stream below), FOUR rows ahead;
//   * streams shorter than four bytes take a bitwise loop and touch no table.
#ifndef SWC_CRC32_TAIL_H
#define SWC_CRC32_TAIL_H

#include "crc32_wave.h"

namespace swc {
namespace crct {

using crcw::kPiece;
using crcw::kRow;
using crcw::kLevels;
using crcw::q128u;

struct TailConsts {
    uint32_t tab[2][256];    // slice-by-2: WaveConsts::tab[0..1]
    uint32_t tabg[4][256];   // WaveConsts::tabg
};
constexpr uint32_t kTailBytes = 6144;   // the Deflate copy kernel's window (lz_copy.h: CfgDeflate)
static_assert(sizeof(TailConsts) == kTailBytes, "the constants of the tail fill the window and no more");
static_assert(offsetof(crcw::WaveConsts, tabg) == 4096 && offsetof(crcw::WaveConsts, fold) == 8192, "load_consts copies by offset");

// Wave-uniform reads of constants in device memory: the constant address space makes them scalar loads.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) uint32_t* kcptr;
#else
typedef const uint32_t* kcptr;
#endif

// The loads of the tail.  They must see what THIS wave's flushes stored -- the 16-byte chunks and the single bytes of a first
// or last chunk that is not whole alike.  The copier waits for all of its stores before it comes here (vmcnt(0): every store
// has been acknowledged by the L2, the vector L1 writes through), so the L2 holds the stream; the CU's L1 may not: a far
// source that was read while the rest of its line had not been written yet left the line there as it was then.  Non-temporal
// loads are served by the L2 and do not look at the L1 (nor fill it: the other waves' records and far sources keep it).
SWC_D q128u ld_stream(gcptr p) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef u32x4 __attribute__((aligned(1))) u32x4_any;
    const u32x4 v = __builtin_nontemporal_load((const SWC_AS_GLOBAL u32x4_any*)p);
    return q128u{v.x, v.y, v.z, v.w};
#else
    return *(const q128u*)p;
#endif
}
SWC_D uint32_t ld_stream32(gcptr p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_nontemporal_load((const SWC_AS_GLOBAL u32_unaligned*)p);
#else
    return load_u32(p);
#endif
}
SWC_D uint32_t ld_stream8(gcptr p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

// four data bytes: two slice-by-2 steps
SWC_D uint32_t step22(const TailConsts* c, uint32_t s, uint32_t data) {
    const uint32_t w = s ^ data;
    const uint32_t u = c->tab[1][w & 0xFF] ^ c->tab[0][(w >> 8) & 0xFF] ^ (w >> 16);
    return c->tab[1][u & 0xFF] ^ c->tab[0][(u >> 8) & 0xFF] ^ (u >> 16);
}
SWC_D uint32_t stepg(const TailConsts* c, uint32_t x) {
    return c->tabg[0][x & 0xFF] ^ c->tabg[1][(x >> 8) & 0xFF] ^ c->tabg[2][(x >> 16) & 0xFF] ^ c->tabg[3][x >> 24];
}
// a piece from state zero
SWC_D uint32_t chain(const TailConsts* c, const q128u& u, const q128u& v) {
    uint32_t z = step22(c, 0, u.x);
    z = step22(c, z, u.y);
    z = step22(c, z, u.z);
    z = step22(c, z, u.w);
    z = step22(c, z, v.x);
    z = step22(c, z, v.y);
    z = step22(c, z, v.z);
    return step22(c, z, v.w);
}

// crcw::head_word with the loads of the tail
SWC_D uint32_t head_word(gcptr out, int64_t r) {
    uint32_t w = 0;
    if (r >= 0) w = ld_stream32(out + r);
    else if (r > -4) for (int b = (int)-r; b < 4; b++) w |= ld_stream8(out + (r + b)) << (8 * b);
    if (r > -4 && r < 4) w ^= r >= 0 ? 0xFFFFFFFFu >> (8 * r) : 0xFFFFFFFFu << (8 * -r);
    return w;
}

// The constants of the tail from `g` (device memory, built by crcw::build_consts) into `c` (the window): 384 16-byte moves.
SWC_D void load_consts(TailConsts* c, const crcw::WaveConsts* g) {
    constexpr int N = kWave;
    const SWC_AS_GLOBAL q128u* src = (const SWC_AS_GLOBAL q128u*)g;
    q128u* dst = (q128u*)c;
    SIMT_BEGIN(t, N)
#pragma unroll
        for (int i = t; i < (int)(kTailBytes / 16u); i += N) dst[i] = src[i < 128 ? i : i + 128];   // tab[0..1] | tabg
    SIMT_END_WAVE
}

// CRC-32 of out[0..len), len < 2^32, by the 64 lanes of one wave that has WAITED for its stores to `out`; `c`: kTailBytes of
// LDS (plain memory on the host) that nothing else uses any more, `g`: the constants in device memory.  The same value in
// every lane.
SWC_D uint32_t crc32_tail(gcptr out, uint32_t len, TailConsts* c, const crcw::WaveConsts* g) {
    using namespace simt;
    constexpr int N = kWave;
    if (len < 4u) {   // the same serial loop in every lane
        uint32_t s = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < len; i++) {
            s ^= ld_stream8(out + i);
            for (int k = 0; k < 8; k++) s = (s >> 1) ^ ((s & 1u) ? crcw::kPoly : 0u);
        }
        return ~s;
    }
    load_consts(c, g);
    const uint32_t pad = (uint32_t)(kRow - (len & (kRow - 1))) & (kRow - 1);
    const uint32_t rows = (uint32_t)(((uint64_t)len + pad) / kRow);
    PT<uint32_t, N> x, y;
    SIMT_BEGIN(t, N)
        const int ln = t & (N - 1);
        // row 0 of a stream that needs padding: begins in the padding, holds (most of) the four bytes that carry the initial
        // value.  A stream that is a whole number of rows starts in the main loop.
        const uint32_t first = pad != 0 ? 1 : 0;
        uint32_t s = 0;
        const int64_t r0 = (int64_t)ln * kPiece - (int64_t)pad;
        if (pad != 0 && r0 + kPiece > 0) {
#pragma unroll
            for (int k = 0; k < kPiece / 4; k++) s = step22(c, s, head_word(out, r0 + 4 * k));
        }
        uint32_t acc = s;
        const int64_t r1 = r0 + (int64_t)first * kRow;   // >= 0
        gcptr p = out + r1;
        uint32_t j = first;
        const uint32_t init = r1 < 4 ? 0xFFFFFFFFu >> (8 * r1) : 0u;   // the initial value on data bytes r1..3 (0..r1-1 were in row 0)
        bool fresh = true;                                             // ... has not been applied yet
        if (((rows - first) & 1u) != 0u) {   // an odd row first
            q128u a0 = ld_stream(p), a1 = ld_stream(p + 16);
            a0.x ^= init;
            fresh = false;
            acc = stepg(c, acc) ^ chain(c, a0, a1);
            p += kRow;
            j++;
        }
        // Two rows per step -- two independent table chains of sixteen dependent steps each, and the two G steps -- from a ring
        // of four rows: the loads of rows j + 4 and j + 5 are issued before the table steps of rows j and j + 1.  (Measured: one
        // row per step is as fast; FOUR are slower than no fusion at all -- sixteen look-ups of one wave at a time in the queue
        // of an LDS that the other waves of the CU copy through.  profiles/r08_experiments.txt, r08b.)
        const q128u zero = {0, 0, 0, 0};
        q128u a[4][2] = {{zero, zero}, {zero, zero}, {zero, zero}, {zero, zero}};
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (j + (uint32_t)k < rows) { a[k][0] = ld_stream(p + k * kRow); a[k][1] = ld_stream(p + k * kRow + 16); }
        if (fresh) a[0][0].x ^= init;
        while (j < rows) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (j >= rows) break;
                const q128u v0 = a[2 * h][0], v1 = a[2 * h][1], v2 = a[2 * h + 1][0], v3 = a[2 * h + 1][1];
                if (j + 4u < rows) {
                    a[2 * h][0] = ld_stream(p + 4 * kRow); a[2 * h][1] = ld_stream(p + 4 * kRow + 16);
                    a[2 * h + 1][0] = ld_stream(p + 5 * kRow); a[2 * h + 1][1] = ld_stream(p + 5 * kRow + 16);
                }
                const uint32_t sa = chain(c, v0, v1), sb = chain(c, v2, v3);
                acc = stepg(c, stepg(c, acc) ^ sa) ^ sb;
                p += 2 * kRow;
                j += 2;
            }
        }
        x[t] = acc;
    SIMT_END
    // the 64 lane states in six levels; the matrices (columns) from device memory, the same address in every lane
    kcptr fold = (kcptr)&g->fold[0][0];
    for (int k = 0; k < kLevels; k++) {
        wave_shift_down(y, x, 1 << k);
        SIMT_BEGIN(t, N)
            uint32_t z = 0;
#pragma unroll
            for (int b = 0; b < 32; b++) z ^= (x[t] >> b) & 1u ? fold[32 * k + b] : 0u;
            x[t] = z ^ y[t];   // (only the lanes that are multiples of 2^(k+1) are used further on)
        SIMT_END
    }
    return ~wave_read(x, 0);
}

}  // namespace crct
}  // namespace swc
#endif
