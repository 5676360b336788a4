// deflate_comp.h -- Deflate COMPRESSION, one buffer per WAVEFRONT (the second piece of the encode side).
//
// Replaces Deflate.compress(data:) (reference Sources/Deflate/Deflate+Compress.swift:22-213): ONE block for the whole buffer --
// static Huffman (RFC 1951 3.2.6) over a greedy LZ77 parse (minimum match 3, maximum 258, distances up to 32,768; no match
// STARTS in the last two bytes, :155, but one may end on the last byte, :185, :146-213), or a stored block when that is not larger and the buffer fits its 16-bit length
// (:30-45, with the reference's own size formula :48-83 applied to THIS parse).
//
// The reference finds matches through an exact dictionary of the most recent position of every three-byte group it has looked
// up (a Swift Dictionary); a GPU wave keeps a HASH table of 4,096 positions in LDS (16-bit entries: a match reaches 32,768
// bytes back, so the low half of a position is enough to find the distance), looks 64 consecutive positions up at once --
// of the lanes of a window that share a hash the HIGHEST enters its position, found with one ballot per hash bit, so the
// result does not depend on the order of the lanes -- and takes the matches of the window greedily from the left; all 64
// lanes extend a match together.  The output therefore is A valid Deflate stream for the same bytes, not the reference's
// bytes: the contract of this path is decode(compress(x)) == x under the reference decoder (Deflate.swift:30-249), zlib and the
// engine's own decoder, and a size close to that of the reference's encoder restated (oracle/rc_deflatec.c) -- not byte
// parity of the compressed stream.
//
//   bits     the codes of a sequence -- up to 62 literals, the length code with its extra bits, the distance code with its
//            extra bits -- are computed one per lane (the static codes are arithmetic: no table), a wave scan of their bit
//            counts gives every lane its place, and the lanes OR their bits into a staging area of the bit stream in LDS
//            (ds_or_b32); whole dwords leave for HBM when half of the area is full.
//
// DYNAMIC blocks (BTYPE 10, opt-in: SWC_CODEC_DEFLATE_COMPRESS_DYNAMIC) -- an extension, the reference writes none.
// The same parse runs twice: pass 1 only counts the lit/len and distance symbols and the extra bits (Compressor<N, kCount>);
// the code lengths come from the shared length-limited builder (huffman_wave.h), and the exact sizes of the static and the
// dynamic block from the counts; pass 2 emits the better one with its codes read from a table in LDS (Compressor<N, kTable>),
// or no pass 2 runs at all and the stored block is written.  Not picking the dynamic block, it writes the static path's bytes.
#ifndef SWC_DEFLATE_COMP_H
#define SWC_DEFLATE_COMP_H

#include "swc_common.h"
#include "simt.h"
#include "huffman_wave.h"

namespace swc {
namespace defc {

// Positions in the hash table: 13 / 12 / 11 bits = 17 / 9 / 5 KB of LDS per wave = 9 / 17 / 30 waves per CU.  100,000 x 64 KiB:
// 443 / 312 / 256 ms, 0.999 / 1.015 / 1.050 x the size of the reference encoder restated (profiles/r05_experiments.txt): 12.
#ifndef SWC_DEFC_HASH_BITS
#define SWC_DEFC_HASH_BITS 12
#endif
constexpr uint32_t kHashBits = SWC_DEFC_HASH_BITS, kHashSize = 1u << kHashBits;
constexpr uint32_t kStageDw = 256;                 // dwords of the bit stream staged in LDS (an emission adds at most 64)
constexpr uint32_t kFlushDw = 128;
constexpr uint32_t kMaxMatch = 258, kMaxDist = 32768;

struct Lds {
    alignas(16) uint16_t table[kHashSize];         // the low 16 bits of the most recent position of the hash
    alignas(16) uint32_t stage[kStageDw + 2];
};

SWC_HD uint32_t hash3(uint32_t w) { return ((w & 0xFFFFFFu) * 2654435761u) >> (32 - kHashBits); }
// the largest stream `n` bytes can turn into: a static block of nine-bit literals, or the stored block
SWC_HD uint64_t bound(uint64_t n) { return n + n / 8 + 16; }
SWC_HD uint32_t rev_bits(uint32_t v, uint32_t n) { return brev32(v) >> (32u - n); }
// static code of a literal byte: (bits, count), most significant code bit first in the stream (RFC 1951 3.2.6)
SWC_HD void literal_code(uint32_t v, uint32_t& code, uint32_t& nb) {
    if (v < 144u) { code = rev_bits(0x30u + v, 8); nb = 8; }
    else { code = rev_bits(0x190u + v - 144u, 9); nb = 9; }
}
SWC_HD void litlen_code(uint32_t sym, uint32_t& code, uint32_t& nb) {   // symbols 256..285
    if (sym < 280u) { code = rev_bits(sym - 256u, 7); nb = 7; }
    else { code = rev_bits(0xC0u + sym - 280u, 8); nb = 8; }
}
// length 3..258 -> its symbol, the count and the value of its extra bits (Deflate+Constants.swift lengthCode / lengthBase as
// arithmetic)
SWC_HD void length_sym(uint32_t len, uint32_t& sym, uint32_t& e, uint32_t& extra) {
    const uint32_t l = len - 3u;
    if (len == 258u) { sym = 285; e = 0; extra = 0; }
    else if (l < 8u) { sym = 257u + l; e = 0; extra = 0; }
    else { e = log2u(l) - 2u; sym = 261u + 4u * e + ((l >> e) & 3u); extra = l & ((1u << e) - 1u); }
}
// distance 1..32768 -> the same (distanceBase as arithmetic)
SWC_HD void distance_sym(uint32_t dist, uint32_t& sym, uint32_t& e, uint32_t& extra) {
    const uint32_t d = dist - 1u;
    if (d < 4u) { sym = d; e = 0; extra = 0; }
    else { const uint32_t p = log2u(d); e = p - 1u; sym = 2u * p + ((d >> e) & 1u); extra = d & ((1u << e) - 1u); }
}
// length 3..258 -> its static code followed by its extra bits
SWC_HD void length_bits(uint32_t len, uint32_t& code, uint32_t& nb) {
    uint32_t sym, e, extra, c, n;
    length_sym(len, sym, e, extra);
    litlen_code(sym, c, n);
    code = c | (extra << n);
    nb = n + e;
}
// distance 1..32768 -> its five-bit static code followed by its extra bits
SWC_HD void distance_bits(uint32_t dist, uint32_t& code, uint32_t& nb) {
    uint32_t sym, e, extra;
    distance_sym(dist, sym, e, extra);
    code = rev_bits(sym, 5) | (extra << 5);
    nb = 5u + e;
}

constexpr uint32_t kLitLen = 286, kDist = 30, kSyms = kLitLen + kDist, kCodeLens = 19, kHuffCap = 288;
// the order of the code-length code's lengths in the header (RFC 1951 3.2.7): 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3,
// 13, 2, 14, 1, 15 -- five bits per entry, the first twelve in one word
SWC_HD uint32_t cl_order(uint32_t i) {
    return i < 12u ? (uint32_t)(0x22caa324e804a30ull >> (5u * i)) & 31u : (uint32_t)(0x3c2e1346cull >> (5u * (i - 12u))) & 31u;
}

// kStatic: the arithmetic static codes (the static kernel); kCount: pass 1 of a dynamic unit, nothing emitted, the symbols
// counted into `sym`; kTable: the codes read from `sym` (code | length << 16, reversed for the LSB-first stream), behind a
// static or a dynamic header
enum : int { kStatic = 0, kCount = 1, kTable = 2 };

template <int N, int M = kStatic>
struct Compressor {
    gcptr src;
    uint64_t n;          // bytes of input
    gptr out;            // 4-byte aligned
    uint64_t cap;
    Lds* l;
    uint64_t obits;      // bits of the stream so far (keeps counting past the capacity)
    uint64_t odw;        // dwords that have left the stage for `out`
    uint32_t fill;       // bits in the stage
    bool nonfinal = false;   // a segment of a larger buffer: BFINAL clear, an empty stored block behind the block (job.aux bit 0)
    uint32_t* sym = nullptr;        // kCount / kTable: lit/len symbols 0..285, distance symbols 286..315
    uint64_t xbits = 0;             // kCount: extra bits of the lengths and distances
    // kTable: the header -- dynamic or static (3 bits); the run-length coded code lengths (symbol | extra << 5) and the
    // code-length code (code | length << 16)
    bool dyn = false;
    const uint16_t* tok = nullptr;
    const uint32_t* clc = nullptr;
    uint32_t hlit = 0, hdist = 0, hclen = 0, ntok = 0;

    // whole dwords of the stage -> out; the incomplete one moves to the front (`all`: the incomplete one too, at the end)
    SWC_D void flush(bool all) {
        const uint32_t nd = all ? (fill + 31u) >> 5 : fill >> 5;
        const uint64_t o0 = odw;
        simt::PT<uint32_t, N> carry;
        SIMT_BEGIN(t, N)
            for (uint32_t i = (uint32_t)t; i < nd; i += (uint32_t)N) {
                const uint64_t b = 4ull * (o0 + i);
                const uint32_t w = l->stage[i];
                if (b + 4u <= cap) *(SWC_AS_GLOBAL uint32_t*)(out + b) = w;
                else for (uint32_t e = 0; e < 4u; e++) if (b + e < cap) out[b + e] = (uint8_t)(w >> (8u * e));
            }
            carry[t] = l->stage[nd];
        SIMT_END_WAVE
        SIMT_BEGIN(t, N)
            for (uint32_t i = (uint32_t)t; i < kStageDw + 2u; i += (uint32_t)N) l->stage[i] = i == 0u && !all ? carry[t] : 0u;
        SIMT_END_WAVE
        odw += nd;
        fill = all ? 0u : fill & 31u;
    }
    // every lane adds `nb` bits (0..32) of `code`, least significant first, lane after lane
    SWC_D void emit(const simt::PT<uint32_t, N>& code, const simt::PT<uint32_t, N>& nb) {
        simt::PT<uint32_t, N> x;
        SIMT_BEGIN(t, N) x[t] = nb[t]; SIMT_END
        simt::wave_scan_incl<N>(x);
        const uint32_t f0 = fill;
        SIMT_BEGIN(t, N)
            if (nb[t] != 0u) {
                const uint32_t b = f0 + x[t] - nb[t], d = b >> 5, s = b & 31u;
                simt::lds_or(&l->stage[d], code[t] << s);
                if (s + nb[t] > 32u) simt::lds_or(&l->stage[d + 1u], code[t] >> (32u - s));
            }
        SIMT_END_WAVE
        const uint32_t total = simt::wave_read<N>(x, N - 1);
        fill += total;
        obits += total;
        if (fill >= 32u * kFlushDw) flush(false);
    }
    // `lit` literals from src[from], then (mlen != 0) a match, then (eob) the end-of-block code
    SWC_D void sequence(uint64_t from, uint64_t lit, uint32_t dist, uint32_t mlen, bool eob) {
        simt::PT<uint32_t, N> code, nb;
        uint32_t lc = 0, ln = 0, dc = 0, dn = 0;
        if constexpr (M != kStatic) {
            if (mlen != 0u) {
                uint32_t ls, le, lx, ds, de, dx;
                length_sym(mlen, ls, le, lx);
                distance_sym(dist, ds, de, dx);
                if constexpr (M == kCount) {
                    uint32_t* const f = sym;
                    SIMT_BEGIN(t, N) if (t == 0) { simt::lds_add(&f[ls], 1u); simt::lds_add(&f[kLitLen + ds], 1u); } SIMT_END
                    xbits += le + de;
                } else {
                    const uint32_t a = sym[ls], b = sym[kLitLen + ds];
                    lc = (a & 0xFFFFu) | (lx << (a >> 16)); ln = (a >> 16) + le;
                    dc = (b & 0xFFFFu) | (dx << (b >> 16)); dn = (b >> 16) + de;
                }
            }
        }
        if constexpr (M == kCount) {
            uint32_t* const f = sym;
            gcptr s = src;
            SIMT_BEGIN(t, N)
                for (uint64_t i = (uint32_t)t; i < lit; i += (uint64_t)N) simt::lds_add(&f[s[from + i]], 1u);
                if (t == 0 && eob) simt::lds_add(&f[256], 1u);
            SIMT_END_WAVE
            return;
        }
        const uint64_t tail = (mlen != 0u ? 2u : 0u) + (eob ? 1u : 0u);
        for (;;) {
            const uint32_t k = lit > (uint64_t)N - tail ? (lit >= (uint64_t)N ? (uint32_t)N : (uint32_t)lit) : (uint32_t)lit;
            const bool last = (uint64_t)k == lit && (uint64_t)k + tail <= (uint64_t)N;
            if constexpr (M == kStatic) {
                SIMT_BEGIN(t, N)
                    uint32_t c = 0, b = 0;
                    if ((uint32_t)t < k) literal_code(src[from + (uint32_t)t], c, b);
                    else if (last && mlen != 0u && (uint32_t)t == k) length_bits(mlen, c, b);
                    else if (last && mlen != 0u && (uint32_t)t == k + 1u) distance_bits(dist, c, b);
                    else if (last && eob && (uint32_t)t == k + (mlen != 0u ? 2u : 0u)) litlen_code(256u, c, b);
                    code[t] = c; nb[t] = b;
                SIMT_END
            } else {
                SIMT_BEGIN(t, N)
                    uint32_t c = 0, b = 0;
                    if ((uint32_t)t < k) { const uint32_t e = sym[src[from + (uint32_t)t]]; c = e & 0xFFFFu; b = e >> 16; }
                    else if (last && mlen != 0u && (uint32_t)t == k) { c = lc; b = ln; }
                    else if (last && mlen != 0u && (uint32_t)t == k + 1u) { c = dc; b = dn; }
                    else if (last && eob && (uint32_t)t == k + (mlen != 0u ? 2u : 0u)) { const uint32_t e = sym[256]; c = e & 0xFFFFu; b = e >> 16; }
                    code[t] = c; nb[t] = b;
                SIMT_END
            }
            emit(code, nb);
            from += k;
            lit -= k;
            if (last) break;
        }
    }

    // kTable: the block header -- BFINAL, BTYPE 01 or 10, and for a dynamic block HLIT, HDIST, HCLEN, the code-length code's
    // lengths and the run-length coded code lengths (RFC 1951 3.2.7)
    SWC_D void header() {
        simt::PT<uint32_t, N> code, nb;
        SIMT_BEGIN(t, N)
            uint32_t c = 0, b = 0;
            if (t == 0) { c = (nonfinal ? 0u : 1u) | (dyn ? 4u : 2u); b = 3; }
            else if (dyn && t == 1) { c = hlit - 257u; b = 5; }
            else if (dyn && t == 2) { c = hdist - 1u; b = 5; }
            else if (dyn && t == 3) { c = hclen - 4u; b = 4; }
            else if (dyn && (uint32_t)t < 4u + hclen) { c = clc[cl_order((uint32_t)t - 4u)] >> 16; b = 3; }
            code[t] = c; nb[t] = b;
        SIMT_END
        emit(code, nb);
        for (uint32_t i0 = 0; dyn && i0 < ntok; i0 += (uint32_t)N) {
            SIMT_BEGIN(t, N)
                uint32_t c = 0, b = 0;
                if (i0 + (uint32_t)t < ntok) {
                    const uint32_t v = tok[i0 + (uint32_t)t], s = v & 31u, e = clc[s];
                    c = (e & 0xFFFFu) | ((v >> 5) << (e >> 16));
                    b = (e >> 16) + (s == 16u ? 2u : s == 17u ? 3u : s == 18u ? 7u : 0u);
                }
                code[t] = c; nb[t] = b;
            SIMT_END
            emit(code, nb);
        }
    }

    SWC_D void run() {
        using simt::PT;
        obits = 0; odw = 0; fill = 0;
        if constexpr (M == kTable) {
            // the header's tokens lie where the hash table lies (DynLds): the stage first, the header, then the table
            SIMT_BEGIN(t, N) for (uint32_t i = (uint32_t)t; i < kStageDw + 2u; i += (uint32_t)N) l->stage[i] = 0; SIMT_END_WAVE
            header();
            SIMT_BEGIN(t, N) for (uint32_t i = (uint32_t)t; i < kHashSize / 2; i += (uint32_t)N) ((uint32_t*)l->table)[i] = 0; SIMT_END_WAVE
        } else {
            SIMT_BEGIN(t, N)
                for (uint32_t i = (uint32_t)t; i < kHashSize / 2; i += (uint32_t)N) ((uint32_t*)l->table)[i] = 0;
                for (uint32_t i = (uint32_t)t; i < kStageDw + 2u; i += (uint32_t)N) l->stage[i] = 0;
            SIMT_END_WAVE
        }
        PT<uint32_t, N> cand, word, hsh, code, nb;
        PT<bool, N> pb, last;
        // of the lanes that hold the same hash, the highest: one ballot per bit of the hash narrows the set of equals
        auto highest_of_equals = [&](uint64_t valid) {
            PT<uint32_t, N> mlo, mhi;
            SIMT_BEGIN(t, N) mlo[t] = (uint32_t)valid; mhi[t] = (uint32_t)(valid >> 32); SIMT_END
            for (uint32_t b = 0; b < kHashBits; b++) {
                SIMT_BEGIN(t, N) pb[t] = ((hsh[t] >> b) & 1u) != 0u; SIMT_END
                const uint64_t bal = simt::wave_ballot<N>(pb);
                SIMT_BEGIN(t, N)
                    const uint64_t same = ((hsh[t] >> b) & 1u) ? bal : ~bal;
                    mlo[t] &= (uint32_t)same; mhi[t] &= (uint32_t)(same >> 32);
                SIMT_END
            }
            SIMT_BEGIN(t, N)
                const uint64_t m = ((uint64_t)mhi[t] << 32) | mlo[t];
                last[t] = ((valid >> t) & 1ull) != 0ull && (t == N - 1 || (m >> (t + 1)) == 0ull);
            SIMT_END
        };
        // block header: BFINAL = 1, BTYPE = 01 (Deflate+Compress.swift:103-104); a SEGMENT of a larger buffer (`nonfinal`,
        // framing_deflate.cpp) leaves BFINAL clear
        if constexpr (M == kStatic) {
            SIMT_BEGIN(t, N) code[t] = t == 0 ? (nonfinal ? 2u : 3u) : 0u; nb[t] = t == 0 ? 3u : 0u; SIMT_END
            emit(code, nb);
        }
        uint64_t pos = 0, anchor = 0;
        const uint64_t plimit = n >= 3 ? n - 3 : 0;     // the last position a match may start at (:155: i < endIndex - 2)
        while (n >= 3 && pos <= plimit) {
            SIMT_BEGIN(t, N)
                const uint64_t p = pos + (uint32_t)t;
                const bool ok = p <= plimit;
                uint32_t w = 0;
                if (ok) w = p + 4 <= n ? load_u32(src + p) & 0xFFFFFFu : (uint32_t)src[p] | ((uint32_t)src[p + 1] << 8) | ((uint32_t)src[p + 2] << 16);
                word[t] = w;
                hsh[t] = ok ? hash3(w) : 0u;
                cand[t] = ok ? (uint32_t)l->table[hsh[t]] : 0u;
                pb[t] = ok;
            SIMT_END_WAVE
            highest_of_equals(simt::wave_ballot<N>(pb));
            SIMT_BEGIN(t, N)
                const uint64_t p = pos + (uint32_t)t;
                if (last[t]) l->table[hsh[t]] = (uint16_t)p;
                bool v = false;
                const uint32_t d = ((uint32_t)p - cand[t]) & 0xFFFFu;      // the entry is the low half of a position: this is the distance
                if (p <= plimit && d != 0u && d <= kMaxDist && (uint64_t)d <= p)
                    v = (load_u32(src + p - d) & 0xFFFFFFu) == word[t];    // (p - d + 4 <= p + 3 <= n)
                pb[t] = v;
                cand[t] = d;                                                  // from here on: the distance
            SIMT_END_WAVE
            const uint64_t m = simt::wave_ballot<N>(pb);
            uint32_t cur = 0;
            while (cur < (uint32_t)N) {
                const uint64_t m2 = m & ~((cur == 0 ? 0ull : (1ull << cur) - 1ull));
                if (m2 == 0) break;
                const uint32_t f = (uint32_t)simt::ctz64(m2);
                const uint64_t mp = pos + f;
                if (mp < anchor) { cur = f + 1; continue; }     // (inside the match just written)
                const uint32_t dist = simt::uniform(simt::wave_read<N>(cand, (int)f));
                const uint64_t c = mp - dist;
                uint32_t len = 3;
                for (;;) {   // all lanes extend the match, 64 bytes per step (:185: up to 258, not past the end)
                    SIMT_BEGIN(t, N)
                        const uint64_t a = mp + len + (uint32_t)t;
                        pb[t] = !(a < n && len + (uint32_t)t < kMaxMatch && src[a] == src[c + len + (uint32_t)t]);
                    SIMT_END
                    const uint64_t mm = simt::wave_ballot<N>(pb);
                    if (mm) { len += (uint32_t)simt::ctz64(mm); break; }
                    len += N;
                }
                sequence(anchor, mp - anchor, dist, len, false);
                anchor = mp + len;
                cur = anchor - pos >= (uint64_t)N ? (uint32_t)N : (uint32_t)(anchor - pos);
            }
            pos = anchor > pos + N ? anchor : pos + N;
        }
        sequence(anchor, n - anchor, 0, 0, true);   // the rest as literals, the end-of-block code (:198-207, :135)
        if constexpr (M == kCount) return;
        if (nonfinal) {
            // an empty stored block behind it (000, the padding to the byte, LEN = 0, NLEN = 0xFFFF): the segment ends on a byte,
            // and the segments of a buffer are one Deflate stream when they are put one behind the other
            const uint32_t pad = (8u - (uint32_t)((obits + 3u) & 7u)) & 7u;
            SIMT_BEGIN(t, N)
                code[t] = t == 3 ? 0xFFFFu : 0u;
                nb[t] = t == 0 ? 3u : t == 1 ? pad : t == 2 || t == 3 ? 16u : 0u;
            SIMT_END
            emit(code, nb);
        }
        flush(true);
    }
};

// Deflate+Compress.swift:30-45: a stored block -- BFINAL (clear for a segment), BTYPE 00, LEN, NLEN, the bytes
template <int N>
SWC_D void write_stored(gptr o, gcptr s, uint32_t nn, uint64_t cap, bool nonfinal) {
    const uint32_t nl = nn ^ 0xFFFFu;
    SIMT_BEGIN(t, N)
        if (t == 0) {
            const uint8_t h[5] = {(uint8_t)(nonfinal ? 0 : 1), (uint8_t)(nn & 0xFFu), (uint8_t)(nn >> 8), (uint8_t)(nl & 0xFFu), (uint8_t)(nl >> 8)};
            for (uint32_t k = 0; k < 5u; k++) if (k < cap) o[k] = h[k];
        }
        for (uint32_t i = (uint32_t)t; i < nn; i += (uint32_t)N) if (5ull + i < cap) o[5u + i] = s[i];
    SIMT_END_WAVE
}

// One wavefront = one job: job.in / in_len = the buffer, job.out (4-byte aligned) / out_cap = room for the stream.
// job.out_len = bytes of the stream (SWC_E_CAPACITY with the size needed if it does not fit out_cap).
template <int N>
SWC_D void deflate_compress_job(Job& job, Lds* lds) {
    Compressor<N> c;
    c.src = (gcptr)job.in;
    c.n = job.in_len;
    c.out = (gptr)job.out;
    c.cap = job.out_cap;
    c.l = lds;
    c.nonfinal = (job.aux & 1) != 0;
    c.run();
    uint64_t size = (c.obits + 7) >> 3;
    // Deflate+Compress.swift:30-45: stored if not larger than the static block and the length fits 16 bits
    if (5 + c.n <= size && 5 + c.n <= 65535) {
        size = 5 + c.n;
        write_stored<N>(c.out, c.src, (uint32_t)c.n, c.cap, c.nonfinal);
    }
    job.out_len = size;
    job.in_consumed = job.in_len;
    job.status = size > job.out_cap ? SWC_E_CAPACITY : SWC_OK;
}

// ---- dynamic blocks ----------------------------------------------------------------------------------------------------------
// LDS of one wave: the parse's hash table and stage (passes 1 and 2) share their place with what is built between the passes;
// the counts / code table of the symbols stay.  9,232 + 1,264 = 10,496 B.
struct DynLds {
    union {
        Lds parse;
        struct {
            uint16_t tok[kSyms];             // the code lengths of both tables, run-length coded: symbol | extra bits << 5
            uint32_t cl[kCodeLens];          // the code-length code: counts, then code | length << 16
            uint32_t misc[8];                // results of lane 0 for the whole wave
            huff::HuffLds<kHuffCap> h;       // the builder (ends inside the stage, which is idle until the header)
        } b;
    };
    uint32_t sym[kSyms];                     // pass 1: counts (lit/len 0..285, distance 286..315); then code | length << 16
};
static_assert(sizeof(((DynLds*)nullptr)->b) <= sizeof(Lds), "the builder must fit in the parse's place");
static_assert(offsetof(Lds, stage) >= (kSyms * 2u + (kCodeLens + 8u) * 4u), "the header's tokens must lie clear of the stage");

// the code of one alphabet from the counts in f[0 .. nsym): the symbols that occur, and fillers of weight 1 at the lowest unused
// symbols until there are two (a complete code), go to the builder as a list in ascending order; f[s] becomes the code of s,
// reversed for the LSB-first stream, | length << 16 (0: no code).  Returns sum of count x length.
template <int N>
SWC_D uint64_t build_code(DynLds* l, uint32_t* f, uint32_t nsym, uint32_t max_len) {
    auto& b = l->b;
    SIMT_BEGIN(t, N)
        if (t == 0) {
            uint32_t used = 0;
            for (uint32_t s = 0; s < nsym; s++) used += f[s] != 0u ? 1u : 0u;
            uint32_t need = used < 2u ? 2u - used : 0u, m = 0;
            for (uint32_t s = 0; s < nsym; s++) {
                uint32_t w = f[s];
                if (w == 0u && need != 0u) { w = 1u; need--; }
                if (w != 0u) b.h.w[m++] = w;
            }
            b.misc[0] = m;
        }
    SIMT_END_WAVE
    const uint32_t alpha = b.misc[0];
    huff::huffman_wave<N>(&b.h, alpha, max_len);
    SIMT_BEGIN(t, N)
        if (t == 0) {
            uint32_t used = 0;
            for (uint32_t s = 0; s < nsym; s++) used += f[s] != 0u ? 1u : 0u;
            uint32_t need = used < 2u ? 2u - used : 0u, m = 0;
            uint64_t cost = 0;
            for (uint32_t s = 0; s < nsym; s++) {
                const uint32_t c = f[s];
                bool u = c != 0u;
                if (!u && need != 0u) { u = true; need--; }
                uint32_t e = 0;
                if (u) {
                    const uint32_t v = b.h.wt[m++], ln = v >> 24;
                    e = rev_bits(v & 0xFFFFFFu, ln) | (ln << 16);
                    cost += (uint64_t)c * ln;
                }
                f[s] = e;
            }
            b.misc[1] = (uint32_t)cost;
            b.misc[2] = (uint32_t)(cost >> 32);
        }
    SIMT_END_WAVE
    return ((uint64_t)b.misc[2] << 32) | b.misc[1];
}

// the code lengths of one table, run-length coded (RFC 1951 3.2.7, as zlib codes them: 16 repeats the length just written,
// so it never comes first; 17 / 18 for runs of zeros); returns the new token count, adds the extra bits to `xb`
SWC_HD uint32_t rle_lengths(const uint32_t* f, uint32_t n, uint16_t* tok, uint32_t nt, uint32_t* cnt, uint32_t& xb) {
    auto put = [&](uint32_t s, uint32_t x, uint32_t e) { tok[nt++] = (uint16_t)(s | (x << 5)); cnt[s]++; xb += e; };
    for (uint32_t i = 0; i < n;) {
        const uint32_t v = f[i] >> 16;
        uint32_t run = 1;
        while (i + run < n && (f[i + run] >> 16) == v) run++;
        i += run;
        if (v == 0u) {
            while (run >= 11u) { const uint32_t k = run < 138u ? run : 138u; put(18, k - 11u, 7); run -= k; }
            if (run >= 3u) { put(17, run - 3u, 3); run = 0; }
        } else {
            put(v, 0, 0);
            run--;
            while (run >= 3u) { const uint32_t k = run < 6u ? run : 6u; put(16, k - 3u, 2); run -= k; }
        }
        while (run > 0u) { put(v, 0, 0); run--; }
    }
    return nt;
}

// the bits of a block (its header included) -> bytes of the unit: a segment adds 000, the padding and LEN / NLEN
SWC_HD uint64_t unit_bytes(uint64_t bits, bool nonfinal) { return nonfinal ? (bits + 3u + 7u) / 8u + 4u : (bits + 7u) / 8u; }

// One wavefront = one job, as deflate_compress_job, the block dynamic where that is smaller (SWC_CODEC_DEFLATE_COMPRESS_DYNAMIC)
template <int N>
SWC_D void deflate_compress_dynamic_job(Job& job, DynLds* lds) {
    const bool nonfinal = (job.aux & 1) != 0;
    const uint64_t n = job.in_len;
    SIMT_BEGIN(t, N) for (uint32_t i = (uint32_t)t; i < kSyms; i += (uint32_t)N) lds->sym[i] = 0u; SIMT_END_WAVE
    // ---- pass 1: the parse, counted
    Compressor<N, kCount> c1;
    c1.src = (gcptr)job.in;
    c1.n = n;
    c1.out = (gptr)job.out;
    c1.cap = 0;
    c1.l = &lds->parse;
    c1.sym = lds->sym;
    c1.run();
    const uint64_t xbits = c1.xbits;
    uint32_t* const f = lds->sym;
    auto& b = lds->b;
    // ---- the static block's size from the counts
    SIMT_BEGIN(t, N)
        if (t == 0) {
            uint64_t bits = 0;
            for (uint32_t s = 0; s < kSyms; s++) {
                const uint32_t ln = s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : s < kLitLen ? 8u : 5u;
                bits += (uint64_t)f[s] * ln;
            }
            b.misc[3] = (uint32_t)bits;
            b.misc[4] = (uint32_t)(bits >> 32);
        }
    SIMT_END_WAVE
    const uint64_t bits_s = 3u + (((uint64_t)b.misc[4] << 32) | b.misc[3]) + xbits;
    // ---- the dynamic block's codes and size
    const uint64_t cost_ll = build_code<N>(lds, f, kLitLen, 15u);
    const uint64_t cost_d = build_code<N>(lds, f + kLitLen, kDist, 15u);
    SIMT_BEGIN(t, N)
        if (t == 0) {
            uint32_t hlit = kLitLen, hdist = kDist;
            while (hlit > 257u && f[hlit - 1u] == 0u) hlit--;
            while (hdist > 1u && f[kLitLen + hdist - 1u] == 0u) hdist--;
            for (uint32_t k = 0; k < kCodeLens; k++) b.cl[k] = 0u;
            uint32_t xb = 0;
            uint32_t nt = rle_lengths(f, hlit, b.tok, 0, b.cl, xb);        // each table on its own: no run crosses between them
            nt = rle_lengths(f + kLitLen, hdist, b.tok, nt, b.cl, xb);
            b.misc[3] = hlit; b.misc[4] = hdist; b.misc[5] = nt; b.misc[6] = xb;
        }
    SIMT_END_WAVE
    const uint32_t hlit = b.misc[3], hdist = b.misc[4], ntok = b.misc[5], tok_xb = b.misc[6];
    const uint64_t cost_cl = build_code<N>(lds, b.cl, kCodeLens, 7u);
    uint32_t hclen = kCodeLens;
    while (hclen > 4u && b.cl[cl_order(hclen - 1u)] == 0u) hclen--;
    const uint64_t bits_d = 3u + 14u + 3u * hclen + cost_cl + tok_xb + cost_ll + cost_d + xbits;
    const uint64_t size_s = unit_bytes(bits_s, nonfinal), size_d = unit_bytes(bits_d, nonfinal);
    const bool dyn = size_d < size_s;
    uint64_t size = dyn ? size_d : size_s;
    // Deflate+Compress.swift:30-45 applied to the better of the two Huffman blocks
    const bool stored = 5 + n <= size && 5 + n <= 65535;
    if (stored) size = 5 + n;
    job.out_len = size;
    job.in_consumed = job.in_len;
    if (size > job.out_cap) { job.status = SWC_E_CAPACITY; return; }
    if (stored) {
        write_stored<N>((gptr)job.out, (gcptr)job.in, (uint32_t)n, job.out_cap, nonfinal);
        job.status = SWC_OK;
        return;
    }
    if (!dyn) {   // the static codes as a table: pass 2 then writes the static kernel's bits
        SIMT_BEGIN(t, N)
            for (uint32_t s = (uint32_t)t; s < kSyms; s += (uint32_t)N) {
                uint32_t c, ln;
                if (s < 256u) literal_code(s, c, ln);
                else if (s < kLitLen) litlen_code(s, c, ln);
                else { c = rev_bits(s - kLitLen, 5); ln = 5; }
                f[s] = c | (ln << 16);
            }
        SIMT_END_WAVE
    }
    // ---- pass 2: the parse again, emitted
    Compressor<N, kTable> c2;
    c2.src = (gcptr)job.in;
    c2.n = n;
    c2.out = (gptr)job.out;
    c2.cap = job.out_cap;
    c2.l = &lds->parse;
    c2.nonfinal = nonfinal;
    c2.sym = f;
    c2.dyn = dyn;
    c2.tok = b.tok;
    c2.clc = b.cl;
    c2.hlit = hlit; c2.hdist = hdist; c2.hclen = hclen; c2.ntok = ntok;
    c2.run();
    // (the sizes above are exact: a difference is a defect of this file, reported rather than handed on as a stream)
    job.status = (c2.obits + 7) >> 3 == size ? SWC_OK : SWC_E_DEVICE;
}

}  // namespace defc
}  // namespace swc
#endif
