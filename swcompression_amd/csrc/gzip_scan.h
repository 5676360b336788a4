// gzip_scan.h -- where the members of a PLAIN multi-member gzip file may start, found on the device.
//
// A gzip member carries no compressed size, so the sequential walk of GzipArchive.multiUnarchive finds member k + 1 only behind the
// decode of member k.  What CAN be found without a decode is every place a member MAY start -- the candidate rule of
// include/swc_hip.h (swc_index_blocks kind 9): 1f 8b 08 and a flags byte without reserved bits, with room for the smallest member
// behind it -- and, for each such place, how long its header is and what the member's size fields would be if the NEXT candidate
// is where it ends.  The host decodes all candidates ahead in one launch and lets the walk decide (framing_deflate.cpp).  Four bodies:
//   count_tile   a wavefront per tile of kTile bytes: the number of candidates whose first byte lies in the tile;
//   scan_tiles   ONE wavefront walks the tile counts 64 at a time: their exclusive 64-bit prefix sums, the total into *n;
//   write_tile   the pass of count_tile once more: candidate j of the tile stores its offset at starts[prefix + j];
//   parse_refs   a thread per candidate: the header measured, the ref written.
// The order of the refs is the order of the file by construction: no atomics, no LDS.
//
// The passes and their borders.  `src` has any alignment, the loads are 16-byte aligned ones: the file is laid over the aligned
// addresses, v = p + (src % 16) is the VIRTUAL position of byte p, and tiles, wave steps (1 KiB) and chunks (16 bytes, one per lane
// and step) are cut in v.  A candidate needs the three bytes behind its first, so a lane loads its chunk and the dword behind it --
// as one 16-byte and one 4-byte load where all 20 bytes lie in the buffer, else byte by byte with every byte outside [src, src + len)
// taken as zero (at most two chunks of a buffer: the one src starts in and the one it ends in; zero matches no magic).
#ifndef SWC_GZIP_SCAN_H
#define SWC_GZIP_SCAN_H

#include "swc_common.h"
#include "simt.h"

namespace swc {
namespace gzscan {

constexpr uint32_t kChunk = 16, kStep = kChunk * kWave;   // a lane's bytes, a wave's bytes per step
constexpr uint32_t kTile = 16384;                        // a wave's bytes per launch: 16 steps
constexpr uint32_t kSteps = kTile / kStep;
static_assert(kTile % 1024 == 0 && kTile <= 65536 && kTile % kStep == 0, "a tile: whole steps, at most 64 KiB");
constexpr uint32_t kLeast = 20;      // the smallest member: 10 header bytes, an empty static block, 8 trailer bytes
constexpr uint32_t kNameMax = 256;   // FNAME / FCOMMENT with their zero: what one thread reads of a field at most
constexpr uint32_t kUnusable = 1;    // swc_block_ref::flags bit 0

// One ref as the device writes it (the layout of swc_block_ref, include/swc_hip.h)
struct Ref { uint64_t offset, comp_len, uncomp_len; uint32_t aux, flags; };

// a buffer of `len` bytes holds at most this many candidates (three bytes apart, the last one kLeast bytes in front of the end)
SWC_HD uint64_t most(uint64_t len) { return len < kLeast ? 0 : (len - kLeast) / 3 + 1; }
// tiles of a buffer that starts `a` bytes behind a 16-byte boundary
SWC_HD uint64_t tiles(uint64_t len, uint32_t a) { return most(len) ? (len + a + kTile - 1) / kTile : 0; }

// The workspace of one call, cut from an 8-byte aligned base: [prefix (tiles) | starts (slots) | counts (tiles)].  slots: the
// candidates that get a ref and ONE more -- ref cap - 1 of a call that found more than cap ends where candidate cap starts.
struct Plan {
    uint64_t tiles, slots, prefix, starts, counts, bytes;
};
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

struct __attribute__((aligned(16), may_alias)) q128a16 { uint32_t x, y, z, w; };

// The candidates whose first byte lies in the chunk at virtual position v0 (a multiple of 16), as a mask of its 16 bytes.
// base = src - a (16-byte aligned), end = a + len.
SWC_D uint32_t chunk_mask(gcptr base, uint32_t a, uint64_t end, uint64_t v0) {
    if (v0 + kLeast > end) return 0;   // no candidate from here on: it would not have its kLeast bytes
    uint32_t w[5];
    if (v0 >= a) {                     // (v0 + 20 <= end: all of it in the buffer)
        const q128a16 q = *(const SWC_AS_GLOBAL q128a16*)(base + v0);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        w[4] = *(const SWC_AS_GLOBAL uint32_t*)(base + v0 + kChunk);
    } else {                           // the chunk src starts in
#pragma unroll
        for (uint32_t i = 0; i < 5; i++) {
            uint32_t d = 0;
#pragma unroll
            for (uint32_t b = 0; b < 4; b++) {
                const uint64_t v = v0 + 4 * i + b;
                if (v >= a && v < end) d |= (uint32_t)base[v] << (8 * b);
            }
            w[i] = d;
        }
    }
    // byte j starts a candidate: 1f 8b 08, then a byte without the bits 0xE0 ...
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < kChunk; j++) {
        const uint32_t d = alignbyte32(w[j / 4 + 1], w[j / 4], j & 3u);
        m |= (uint32_t)((d & 0xE0FFFFFFu) == 0x00088B1Fu) << j;
    }
    // ... and kLeast bytes from it on lie in the buffer
    const uint64_t room = end - kLeast - v0;   // the last j that has them
    return room >= kChunk - 1 ? m : m & ((2u << (uint32_t)room) - 1u);
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
#pragma unroll 4
        for (uint32_t s = 0; s < kSteps; s++) k += (uint32_t)popc32(chunk_mask(base, a, end, v + s * kStep + (uint32_t)t * kChunk));
        c[t] = k;
    SIMT_END
    wave_scan_incl(c);
    const uint32_t total = wave_read(c, N - 1);
    SIMT_BEGIN(t, N)
        if (t == 0) counts[tile] = total;
    SIMT_END
}

// ---- offsets: ONE wavefront, 64 tiles per step.  Two users: the candidates here and the marks of bzip2_scan.h; a step's sum stays far
// below 2^32 for both (64 x kTile / 3 candidates, 64 x 8 x kTile = 2^23 marks) ---------------------------------------------------------
template <int N>
SWC_D void scan_tiles(const uint32_t* counts, uint64_t n_tiles, uint64_t* prefix, uint64_t* n) {
    using namespace simt;
    static_assert(N == kWave, "one wavefront");
    uint64_t run = 0;
    for (uint64_t at = 0; at < n_tiles; at += N) {
        PT<uint32_t, N> c, incl;
        SIMT_BEGIN(t, N)
            const uint64_t i = at + (uint32_t)t;
            c[t] = i < n_tiles ? counts[i] : 0u;
            incl[t] = c[t];
        SIMT_END
        wave_scan_incl(incl);
        SIMT_BEGIN(t, N)
            const uint64_t i = at + (uint32_t)t;
            if (i < n_tiles) prefix[i] = run + incl[t] - c[t];
        SIMT_END
        run += wave_read(incl, N - 1);
    }
    SIMT_BEGIN(t, N)
        if (t == 0) *n = run;
    SIMT_END
}

// ---- pass 2: wave `tile` stores where its candidates start, those with an index below `slots` ----------------------------------------
template <int N>
SWC_D void write_tile(uint64_t tile, const uint8_t* src, uint64_t len, const uint64_t* prefix, uint64_t* starts, uint64_t slots) {
    using namespace simt;
    static_assert(N == kWave, "one wavefront");
    const uint32_t a = (uint32_t)((uintptr_t)src & 15u);
    gcptr base = (gcptr)src - a;
    const uint64_t end = len + a, v = tile * kTile;
    uint64_t run = uniform(prefix[tile]);
    if (run >= slots) return;
    for (uint32_t s = 0; s < kSteps; s++) {
        PT<uint32_t, N> m, incl;
        PT<bool, N> any;
        SIMT_BEGIN(t, N)
            m[t] = chunk_mask(base, a, end, v + s * kStep + (uint32_t)t * kChunk);
            incl[t] = (uint32_t)popc32(m[t]);
            any[t] = m[t] != 0;
        SIMT_END
        if (wave_ballot(any) == 0) continue;
        wave_scan_incl(incl);
        SIMT_BEGIN(t, N)
            uint32_t mm = m[t];
            uint64_t k = run + incl[t] - (uint32_t)popc32(mm);
            const uint64_t v0 = v + s * kStep + (uint32_t)t * kChunk;
            while (mm) {
                if (k < slots) starts[k] = v0 + (uint32_t)ctz64(mm) - a;
                mm &= mm - 1u;
                k++;
            }
        SIMT_END
        run += wave_read(incl, N - 1);
    }
}

// ---- refs: thread g * N + t measures candidate k = its number, k < min(*n, cap) ----------------------------------------------------
// The length of the header at p by the rule (XLEN skipped, the names up to kNameMax bytes with their zero, two bytes of FHCRC), every
// read in front of `len`; 0: the header leaves the buffer or a name is longer.
SWC_D uint64_t header_bytes(gcptr in, uint64_t len, uint64_t p) {
    const uint32_t flags = in[p + 3];
    uint64_t q = p + 10;
    if (flags & 0x04u) {
        if (q + 2 > len) return 0;
        q += 2u + ((uint32_t)in[q] | (uint32_t)in[q + 1] << 8);
    }
    for (uint32_t bit = 0x08u; bit <= 0x10u; bit <<= 1) {
        if (!(flags & bit)) continue;
        uint32_t i = 0;
        for (;; i++) {
            if (i == kNameMax || q + i >= len) return 0;
            if (in[q + i] == 0) break;
        }
        q += i + 1;
    }
    if (flags & 0x02u) q += 2;
    return q > len ? 0 : q - p;
}
template <int N>
SWC_D void parse_refs(uint64_t g, const uint8_t* src, uint64_t len, const uint64_t* starts, const uint64_t* n, uint64_t cap, Ref* refs) {
    gcptr in = (gcptr)src;
    const uint64_t found = *n;
    SIMT_BEGIN(t, N)
        const uint64_t k = g * N + (uint32_t)t;
        if (k < found && k < cap) {
            const uint64_t p = starts[k], next = k + 1 < found ? starts[k + 1] : len;   // (k + 1 == cap: the slot behind the last ref's)
            const uint64_t h = header_bytes(in, len, p);
            const bool usable = h != 0 && p + h + 10 <= next;
            const uint64_t at = p + h;
            gptr r = (gptr)reinterpret_cast<uint8_t*>(refs + k);
            store_u64(r, usable ? at : p);
            store_u64(r + 8, usable ? next - at - 8 : 0);
            store_u64(r + 16, usable ? (uint64_t)load_u32(in + next - 4) : 0);
            store_u64(r + 24, usable ? h : (uint64_t)kUnusable << 32);
        }
    SIMT_END
}

}  // namespace gzscan
}  // namespace swc
#endif
