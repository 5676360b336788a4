// bzip2_scan.h -- where the blocks and the ends of the streams of a .bz2 file may start, found on the device.
//
// A bzip2 block starts at any BIT and carries no length; what can be found without a decode is every place the 48-bit magic of a
// block (0x314159265359) or of the end of a stream (0x177245385090) stands -- the marks of include/swc_hip.h (swc_index_blocks kind
// 10): bit offset b >= 32 with the magic and the 32-bit word behind it in the buffer (b + 80 <= 8 len).  The passes are those of
// gzip_scan.h, and so are the workspace, the slot more than cap and the virtual positions of a `src` at any alignment:
//   count_tile   a wavefront per tile of kTile bytes: the number of marks whose first bit lies in the tile;
//   scan_tiles   gzscan::scan_tiles, the ONE wavefront over the tile counts (gzip_scan.h);
//   write_tile   the pass of count_tile once more -- only over a tile that counted marks: mark j of it stores its bit offset at
//                starts[prefix + j];
//   mark_refs    a thread per mark: the word behind the magic and which magic it is read from the buffer, the ref written.
// The order of the refs is the order of the file by construction: no atomics, no LDS.
//
// The pass is bound by instructions, not by bandwidth: a lane's chunk of 16 bytes is 128 places.  So a cheap NECESSARY test comes
// first.  Whatever the bit s = 0..7 a mark starts at inside its first byte, the four whole bytes behind that byte are bits 8 - s ..
// 40 - s of the magic: one dword per magic and s.  A lane compares the unaligned dword behind each of its 16 bytes with those 16
// constants (an alignbyte and 16 compares a byte) and goes on only where one of them is met -- about once in 10^7 chunks of
// arbitrary bytes.  There it reads the chunk again byte by byte and compares all 48 bits at all eight s: that compare alone decides
// what is a mark, and the bounds with it.  The first test cannot lose a mark: all six or seven bytes of a mark lie in the buffer, so
// the dword it looked at is the file's (bytes outside [src, src + len), taken as zero in the chunks at both ends, are never part of one).
#ifndef SWC_BZIP2_SCAN_H
#define SWC_BZIP2_SCAN_H

#include "gzip_scan.h"

namespace swc {
namespace bzscan {

using gzscan::kChunk;
using gzscan::kStep;
using gzscan::kSteps;
using gzscan::kTile;
using gzscan::Plan;
using gzscan::Ref;

constexpr uint64_t kBlockMagic = 0x314159265359ull, kEndMagic = 0x177245385090ull, kMask48 = 0xFFFFFFFFFFFFull;
constexpr uint32_t kHeadBits = 32, kMarkBits = 80;   // nothing in front of the stream header's end; the magic and the word behind it
constexpr uint32_t kEnd = 1;                          // swc_block_ref::flags bit 0: the end of a stream
constexpr uint32_t kLeast = (kHeadBits + kMarkBits) / 8;   // 14: the shortest buffer that holds a mark

// a buffer of `len` bytes holds at most this many marks (one per bit from 32 to 8 len - 80)
SWC_HD uint64_t most(uint64_t len) { return len < kLeast ? 0 : 8 * len - (kHeadBits + kMarkBits) + 1; }
// tiles of a buffer that starts `a` bytes behind a 16-byte boundary
SWC_HD uint64_t tiles(uint64_t len, uint32_t a) { return most(len) ? (len + a + kTile - 1) / kTile : 0; }
// the workspace of one call, as gzscan::plan cuts it: [prefix (tiles) | starts (slots) | counts (tiles)], slots = the refs and one more
SWC_HD Plan plan(uint64_t len, uint64_t cap) {
    Plan p;
    const uint64_t m = most(len);
    p.tiles = tiles(len, 15);   // (whatever the alignment of src)
    p.slots = (cap < m ? cap : m) + 1;
    p.prefix = 0;
    p.starts = p.prefix + p.tiles * sizeof(uint64_t);
    p.counts = p.starts + p.slots * sizeof(uint64_t);
    p.bytes = p.counts + ((p.tiles * sizeof(uint32_t) + 7) & ~(uint64_t)7);
    return p;
}

// the four whole bytes behind the first byte of a mark of magic m that starts at bit s of it, as a dword loaded from memory
constexpr uint32_t behind(uint64_t m, uint32_t s) {
    const uint32_t be = (uint32_t)(m >> (8 + s));   // bits 8 - s .. 40 - s, MSB-first
    return (be >> 24) | ((be >> 8) & 0xFF00u) | ((be << 8) & 0xFF0000u) | (be << 24);
}
SWC_D uint32_t may_start(uint32_t d) {   // d: the dword behind a byte
    uint32_t hit = 0;
#pragma unroll
    for (uint32_t s = 0; s < 8; s++) hit |= (uint32_t)(d == behind(kBlockMagic, s)) | (uint32_t)(d == behind(kEndMagic, s));
    return hit;
}

// The marks whose first bit lies in the chunk at virtual position v0 (a multiple of 16): bit 8 j + s of (lo, hi) for the mark at bit s
// of byte j.  base = src - a (16-byte aligned), end = a + len.
struct Marks { uint64_t lo, hi; };
SWC_D uint32_t byte_or_zero(gcptr base, uint32_t a, uint64_t end, uint64_t v) { return v >= a && v < end ? (uint32_t)base[v] : 0u; }
SWC_D Marks chunk_marks(gcptr base, uint32_t a, uint64_t end, uint64_t v0) {
    Marks r = {0, 0};
    if (v0 + kMarkBits / 8 > end) return r;   // no mark from here on: it would not have its 80 bits
    uint32_t w[5];
    if (v0 >= a && v0 + kChunk + 4 <= end) {   // all 20 bytes in the buffer
        const gzscan::q128a16 q = *(const SWC_AS_GLOBAL gzscan::q128a16*)(base + v0);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        w[4] = *(const SWC_AS_GLOBAL uint32_t*)(base + v0 + kChunk);
    } else {                                   // the chunk src starts in, the last ones in front of its end
#pragma unroll
        for (uint32_t i = 0; i < 5; i++) {
            uint32_t d = 0;
#pragma unroll
            for (uint32_t b = 0; b < 4; b++) d |= byte_or_zero(base, a, end, v0 + 4 * i + b) << (8 * b);
            w[i] = d;
        }
    }
    uint32_t hit = 0;
#pragma unroll
    for (uint32_t j = 0; j < kChunk; j++) {
        const uint32_t at = j + 1;   // the dword behind byte j
        hit |= may_start((at & 3u) ? alignbyte32(w[at / 4 + 1], w[at / 4], at & 3u) : w[at / 4]);
    }
    if (!hit) return r;
    // rare: all 48 bits at every place of the chunk, V = the seven bytes from byte j on, MSB-first
    uint64_t V = 0;
    for (uint32_t i = 0; i < 6; i++) V = (V << 8) | byte_or_zero(base, a, end, v0 + i);
    const uint64_t first = 8 * (uint64_t)a + kHeadBits, last = 8 * end - kMarkBits;   // virtual bit positions a mark may have
#pragma unroll 1
    for (uint32_t j = 0; j < kChunk; j++) {
        V = ((V << 8) | byte_or_zero(base, a, end, v0 + j + 6)) & 0x00FFFFFFFFFFFFFFull;
        uint32_t m = 0;
#pragma unroll
        for (uint32_t s = 0; s < 8; s++) {
            const uint64_t t = (V >> (8 - s)) & kMask48, vb = 8 * (v0 + j) + s;
            m |= (uint32_t)((t == kBlockMagic || t == kEndMagic) && vb >= first && vb <= last) << s;
        }
        if (j < 8) r.lo |= (uint64_t)m << (8 * j);
        else r.hi |= (uint64_t)m << (8 * (j - 8));
    }
    return r;
}

// ---- pass 1: wave `tile` counts its tile ----------------------------------------------------------------------------------------
template <int N>
SWC_D void count_tile(uint64_t tile, const uint8_t* src, uint64_t len, uint32_t* counts) {
    using namespace simt;
    static_assert(N == kWave, "one wavefront");
    const uint32_t a = (uint32_t)((uintptr_t)src & 15u);
    gcptr base = (gcptr)src - a;
    const uint64_t end = len + a, v = tile * kTile;
    PT<uint32_t, N> c;
    SIMT_BEGIN(t, N)
        uint32_t k = 0;
#pragma unroll 2
        for (uint32_t s = 0; s < kSteps; s++) {
            const Marks m = chunk_marks(base, a, end, v + s * kStep + (uint32_t)t * kChunk);
            k += (uint32_t)(popc64(m.lo) + popc64(m.hi));
        }
        c[t] = k;
    SIMT_END
    wave_scan_incl(c);
    const uint32_t total = wave_read(c, N - 1);
    SIMT_BEGIN(t, N)
        if (t == 0) counts[tile] = total;
    SIMT_END
}

// ---- pass 2: wave `tile` stores where its marks start, those with an index below `slots`; nothing to do where it counted none -------
template <int N>
SWC_D void write_tile(uint64_t tile, const uint8_t* src, uint64_t len, const uint32_t* counts, const uint64_t* prefix, uint64_t* starts,
                      uint64_t slots) {
    using namespace simt;
    static_assert(N == kWave, "one wavefront");
    if (uniform(counts[tile]) == 0) return;
    const uint32_t a = (uint32_t)((uintptr_t)src & 15u);
    gcptr base = (gcptr)src - a;
    const uint64_t end = len + a, v = tile * kTile;
    uint64_t run = uniform(prefix[tile]);
    if (run >= slots) return;
    for (uint32_t s = 0; s < kSteps; s++) {
        PT<uint64_t, N> lo, hi;
        PT<uint32_t, N> incl;
        PT<bool, N> any;
        SIMT_BEGIN(t, N)
            const Marks m = chunk_marks(base, a, end, v + s * kStep + (uint32_t)t * kChunk);
            lo[t] = m.lo;
            hi[t] = m.hi;
            incl[t] = (uint32_t)(popc64(m.lo) + popc64(m.hi));
            any[t] = (m.lo | m.hi) != 0;
        SIMT_END
        if (wave_ballot(any) == 0) continue;
        wave_scan_incl(incl);
        SIMT_BEGIN(t, N)
            uint64_t l = lo[t], h = hi[t];
            uint64_t k = run + incl[t] - (uint32_t)(popc64(l) + popc64(h));
            const uint64_t b0 = 8 * (v + s * kStep + (uint32_t)t * kChunk - a);   // the bit offset of the chunk (wraps in front of src: no mark there)
            while (l) {
                if (k < slots) starts[k] = b0 + (uint32_t)ctz64(l);
                l &= l - 1u;
                k++;
            }
            while (h) {
                if (k < slots) starts[k] = b0 + 64u + (uint32_t)ctz64(h);
                h &= h - 1u;
                k++;
            }
        SIMT_END
        run += wave_read(incl, N - 1);
    }
}

// ---- refs: thread g * N + t writes the ref of mark k = its number, k < min(*n, cap) --------------------------------------------------
template <int N>
SWC_D void mark_refs(uint64_t g, const uint8_t* src, uint64_t len, const uint64_t* starts, const uint64_t* n, uint64_t cap, Ref* refs) {
    gcptr in = (gcptr)src;
    const uint64_t found = *n;
    SIMT_BEGIN(t, N)
        const uint64_t k = g * N + (uint32_t)t;
        if (k < found && k < cap) {
            const uint64_t b = starts[k], next = k + 1 < found ? starts[k + 1] : 8 * len;   // (k + 1 == cap: the slot behind the last ref's)
            // the 80 bits from b lie in bytes p .. p + 9, and in byte p + 10 where b is no multiple of 8
            const uint64_t p = b >> 3;
            const uint32_t s = (uint32_t)b & 7u;
            const uint64_t V = __builtin_bswap64(load_u64(in + p));
            const uint64_t W = (V & 0xFFFFu) << 24 | (uint64_t)in[p + 8] << 16 | (uint64_t)in[p + 9] << 8 | (s ? (uint64_t)in[p + 10] : 0u);
            const uint32_t aux = (uint32_t)(W >> (8 - s));
            const uint32_t flags = ((V >> (16 - s)) & kMask48) == kEndMagic ? kEnd : 0u;
            gptr r = (gptr)reinterpret_cast<uint8_t*>(refs + k);
            store_u64(r, b);
            store_u64(r + 8, next - b);
            store_u64(r + 16, 0);
            store_u64(r + 24, (uint64_t)aux | (uint64_t)flags << 32);
        }
    SIMT_END
}

}  // namespace bzscan
}  // namespace swc
#endif
