// lzma_comp.h -- LZMA2 COMPRESSION, one unit per WAVEFRONT: the last codec of the engine that could only be read.
//
// An extension: the reference has no LZMA encoder.  The contract of this path is decode(compress(x)) == x under the reference's
// LZMA2 decoder (LZMA2Decoder.swift:36-74, the oracle), liblzma and the engine's own decoder (lzma_wave.h), and a STREAM CONTRACT
// that the CPU and the GPU tier meet byte for byte (tests/test_lzma2_compress.py replays every stream through the
// range encoder of tests/_lzma_build.py):
//
//   unit     job.in / job.in_len = n raw bytes -> ONE run: it starts with a dictionary reset and refers to nothing in front of
//            itself.  Properties lc 3, lp 0, pb 2 (0x5D); the dictionary-size byte that belongs to the stream is 8 (64 KiB): match
//            distances are 1 .. 65,535.  job.aux bit 0: the unit is a SEGMENT of a longer stream -- no end marker behind it.
//   chunks   chunk k covers the bytes [65536 k, min(n, 65536 (k + 1))): at most 65,536 of them, so a chunk always fits the stored
//            form and every cut is a multiple of 16.  No packet crosses a chunk end: a match is cut there, a rest of one byte is a
//            literal.  LZMA form (control, u - 1, p - 1, properties with 0xC0 / 0xE0, p bytes of the range coder with its five-byte
//            flush) iff header + p < 3 + u, else stored (control, u - 1, the bytes).  Controls: first chunk 0xE0 / 0x01; an LZMA
//            chunk right behind a stored one 0xC0 (model, state and reps reset); any other chunk 0x80 (they go on) / 0x02.
//   packets  literals (matched where the state asks for it), matches of 2 .. 273 bytes, long rep0 matches: a match whose distance is
//            rep0 + 1 is always the rep0 form.  The parse is lz4_comp.h's: a hash table of 16-bit entries in LDS over the four bytes
//            at every position, 64 positions looked up at once, the highest lane of equal hashes enters (found by ballots: the
//            stream does not depend on the order of the lanes), the matches of a window taken greedily from the left.
//   sizes    bound(n) = n + 3 ceil(n / 65536) + 1; with less room SWC_E_CAPACITY and out_len = the size needed; no byte at or
//            behind out + min(out_len, out_cap) is ever written -- an abandoned LZMA attempt and the staged flush included.
//
// How the wave codes a packet.  The ENCODER knows every decision of a packet before it codes the first: a literal is nine (cell,
// bit) pairs, a match up to 32, and the cells of one packet are all different.  So lane k takes decision k: it works out its cell
// from the packet (closed forms of the tree walks), reads the probability, writes the adapted one back -- one LDS round trip for
// the whole packet, not one per bit.  What stays serial is the range coder's arithmetic: low / range over the probabilities, read
// lane by lane (v_readlane), in code that is the same in every lane and touches no memory but the payload stage.
//   stage    the payload's bytes gather in 1,024 bytes of LDS and leave as one 16-byte row per lane; a row that the capacity or the
//            stored form's size cuts, and the last rows of a chunk, leave byte by byte (once per chunk, not in the loop).
//   abandon  as soon as header + bytes written >= 3 + u the chunk can only be stored: the attempt ends, the rest of the chunk's
//            positions still enter the hash table, the stored form overwrites what the attempt wrote (never more than 3 + u bytes).
#ifndef SWC_LZMA_COMP_H
#define SWC_LZMA_COMP_H

#include "swc_common.h"
#include "simt.h"
#include "lzma_wave.h"

namespace swc {
namespace lzmac {

#ifndef SWC_LZMAC_HASH_BITS
#define SWC_LZMAC_HASH_BITS 12
#endif
#ifndef SWC_LZMAC_LC
#define SWC_LZMAC_LC 3
#endif
constexpr uint32_t kHashBits = SWC_LZMAC_HASH_BITS, kHashSize = 1u << kHashBits;
constexpr uint32_t kLc = SWC_LZMAC_LC, kPb = 2;                      // lp = 0
constexpr uint32_t kPropsByte = (kPb * 5 + 0) * 9 + kLc;             // 0x5D
constexpr uint32_t kChunk = 65536, kMaxLen = 273, kMinHash = 4;   // (distances: the 16-bit table entries keep them below 65,536)
constexpr uint32_t kStage = 1024;                                    // 64 lanes x one 16-byte row
constexpr uint32_t kCells = (uint32_t)lzma::lds_bytes_for((int)kLc) / 2;
static_assert(kLc <= (uint32_t)lzma::kMaxLdsLitBits, "the literal coders live in LDS");

struct Lds {
    uint16_t probs[kCells];          // lzma_wave.h's cell layout (P_*), 0x300 << lc literal cells
    uint16_t table[kHashSize];       // the low 16 bits of the most recent position of a hash
    uint32_t stage[kStage / 4];      // payload bytes on their way out
};

SWC_HD uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32 - kHashBits); }
SWC_HD uint64_t bound(uint64_t n) { return n + 3 * ((n + kChunk - 1) / kChunk) + 1; }

SWC_HD uint32_t pos_slot_of(uint32_t rep0) {
    if (rep0 < 4) return rep0;
    const uint32_t nb = log2u(rep0) + 1;
    return 2 * (nb - 1) + ((rep0 >> (nb - 2)) & 1u);
}
// decision i of a bit tree of `nbits` over `v`, most significant bit first: the cell's index in the tree and the bit
SWC_HD void tree_step(uint32_t nbits, uint32_t v, uint32_t i, uint32_t& m, uint32_t& bit) {
    m = (1u << i) | (v >> (nbits - i));
    bit = (v >> (nbits - 1 - i)) & 1u;
}
// ... least significant bit first
SWC_HD void rtree_step(uint32_t v, uint32_t i, uint32_t& m, uint32_t& bit) {
    m = (1u << i) | (i == 0 ? 0u : brev32(v & ((1u << i) - 1u)) >> (32 - i));
    bit = (v >> i) & 1u;
}

template <int N>
struct Compressor {
    gcptr src;
    uint32_t n;             // bytes of the unit
    gptr out;
    uint64_t cap, opos;     // output capacity, bytes written (keeps counting past the capacity)
    Lds* lds;

    // the range coder of the open chunk (tests/_lzma_build.py: RangeEncoder)
    uint64_t low;
    uint32_t range, cache, cache_size;
    uint32_t fill;          // bytes in the stage
    uint64_t sbase;         // where in `out` the stage's first byte goes
    uint64_t limit;         // no payload byte of this chunk is written at or behind it
    uint32_t emitted;       // payload bytes so far
    // the model's registers
    uint32_t state, rep0;

    // the first k bytes of the stage -> out + sbase: whole rows where nothing cuts them
    SWC_D void flush(uint32_t k) {
        const uint8_t* sb = (const uint8_t*)lds->stage;
        SIMT_BEGIN(t, N)
            for (uint32_t lo = 16u * (uint32_t)t; lo < k; lo += 16u * N) {
                const uint32_t want = k - lo < 16u ? k - lo : 16u;
                const uint64_t g = sbase + lo;
                const uint32_t ok = limit > g ? (limit - g < want ? (uint32_t)(limit - g) : want) : 0u;
                if (ok == 16u) store_u128_a4(out + g, lds->stage[lo / 4], lds->stage[lo / 4 + 1], lds->stage[lo / 4 + 2], lds->stage[lo / 4 + 3]);
                else for (uint32_t j = 0; j < ok; j++) out[g + j] = sb[lo + j];
            }
        SIMT_END_WAVE
        sbase += k;
        fill = 0;
    }
    SWC_D void put(uint32_t b) {
        ((uint8_t*)lds->stage)[fill] = (uint8_t)b;   // (the same byte from every lane)
        fill++;
        emitted++;
        if (fill == kStage) { simt::wave_fence(); flush(kStage); }
    }
    SWC_D void shift_low() {
        if ((uint32_t)low < 0xFF000000u || (low >> 32) != 0) {
            const uint32_t carry = (uint32_t)(low >> 32);
            put(cache + carry);
            for (uint32_t i = 1; i < cache_size; i++) put(0xFFu + carry);   // (at most the chunk's bytes)
            cache_size = 0;
            cache = (uint32_t)(low >> 24) & 0xFFu;
        }
        cache_size++;
        low = (low & 0x00FFFFFFull) << 8;
    }
    // The decisions of one packet: lane k holds decision k < cnt -- cell[k] (an index into probs) with bit[k], or a direct bit.
    // The cells are read and adapted by their lanes, then the arithmetic runs over the probabilities in order.
    // That loop is SCALAR code on the device (s_lshr / v_readlane / s_mul_i32 / s_add_u32 / s_addc_u32 / s_cselect, a scalar branch
    // into the normalisation) only because the compiler can prove low, range, cache and cache_size uniform: each is made of
    // constants, readlane results and ballots alone.  Nothing pins that.  After an edit that lets a per-lane value into the
    // chain, look at the assembly again and at the figures of profiles/lzma2_compress_codegen.txt (106 SGPRs, 56 VGPRs).
    SWC_D void code(const simt::PT<uint32_t, N>& cell, const simt::PT<bool, N>& bit, const simt::PT<bool, N>& direct, uint32_t cnt) {
        simt::PT<uint32_t, N> p;
        SIMT_BEGIN(t, N)
            p[t] = 0;
            if ((uint32_t)t < cnt && !direct[t]) {
                const uint32_t v = lds->probs[cell[t]];
                p[t] = v;
                lds->probs[cell[t]] = (uint16_t)(bit[t] ? v - (v >> 5) : v + ((2048u - v) >> 5));
            }
        SIMT_END_WAVE
        const uint64_t bits = simt::wave_ballot<N>(bit), dirs = simt::wave_ballot<N>(direct);
        for (uint32_t k = 0; k < cnt; k++) {
            const uint32_t one = (uint32_t)(bits >> k) & 1u;
            if ((dirs >> k) & 1ull) {
                range >>= 1;
                if (one) low += range;
            } else {
                const uint32_t bnd = (range >> 11) * simt::wave_read<N>(p, (int)k);
                if (one) { low += bnd; range -= bnd; }
                else range = bnd;
            }
            if (range < (1u << 24)) { range <<= 8; shift_low(); }
        }
    }
    // a literal `b` at `pos` behind the byte `prev`; `mb`: the byte rep0 + 1 back (read only where the state says matched)
    SWC_D void literal(uint32_t pos, uint32_t b, uint32_t prev, uint32_t mb) {
        simt::PT<uint32_t, N> cell;
        simt::PT<bool, N> bit, direct;
        const bool matched = state >= 7;
        const uint32_t base = (uint32_t)lzma::P_LITERAL + 0x300u * (prev >> (8 - kLc)) * (kLc ? 1u : 0u);
        const uint32_t im = (uint32_t)lzma::P_IS_MATCH + (state << 4) + (pos & ((1u << kPb) - 1u));
        SIMT_BEGIN(t, N)
            const uint32_t j = (uint32_t)t - 1u;   // lanes 1 .. 8: the literal's bits, the highest first
            uint32_t c = im, one = 0;
            if (t >= 1 && t <= 8) {
                const uint32_t sym = (1u << j) | (b >> (8 - j));
                one = (b >> (7 - j)) & 1u;
                const uint32_t off = matched && ((b ^ mb) >> (8 - j)) == 0 ? (1u + ((mb >> (7 - j)) & 1u)) << 8 : 0u;
                c = base + off + sym;
            }
            cell[t] = c; bit[t] = one != 0; direct[t] = false;
        SIMT_END
        code(cell, bit, direct, 9);
        state = state < 4 ? 0 : state < 10 ? state - 3 : state - 6;
    }
    // a match of `len` bytes `dist` back at `pos`; dist == rep0 + 1: the long rep0 form
    SWC_D void match(uint32_t pos, uint32_t len, uint32_t dist) {
        simt::PT<uint32_t, N> cell;
        simt::PT<bool, N> bit, direct;
        const bool rep = dist - 1 == rep0;
        const uint32_t ps = pos & ((1u << kPb) - 1u), sp = (state << 4) + ps, l = len - 2, st = state;
        const uint32_t nh = rep ? 4u : 2u;
        const uint32_t lbase = (uint32_t)(rep ? lzma::P_REP_LEN : lzma::P_LEN);
        const uint32_t kind = l < 8 ? 0u : l < 16 ? 1u : 2u, nl = kind == 0 ? 1u : 2u, tb = kind == 2 ? 8u : 3u;
        const uint32_t tbase = kind == 2 ? (uint32_t)lzma::P_LEN_HIGH + (rep ? 256u : 0u)
                                         : lbase + (kind == 0 ? (uint32_t)lzma::LEN_LOW : (uint32_t)lzma::LEN_MID) + ps * 8u;
        const uint32_t tv = kind == 0 ? l : kind == 1 ? l - 8 : l - 16;
        const uint32_t r0 = dist - 1, slot = pos_slot_of(r0), ndb = slot >= 4 ? (slot >> 1) - 1 : 0u;
        const uint32_t sb = slot >= 4 ? (2u | (slot & 1u)) << ndb : 0u, rem = r0 - sb;
        const uint32_t nr = slot >= 4 && slot < 14 ? ndb : 0u, nd = slot >= 14 ? ndb - 4 : 0u, na = slot >= 14 ? 4u : 0u;
        const uint32_t sbase_cell = (uint32_t)lzma::P_POS_SLOT + 64u * (l < 3 ? l : 3u);
        const uint32_t cnt = nh + nl + tb + (rep ? 0u : 6u + nr + nd + na);
        SIMT_BEGIN(t, N)
            uint32_t k = (uint32_t)t, c = 0, one = 0, m = 0;
            bool dir = false;
            if (k < nh) {
                if (k == 0) { c = (uint32_t)lzma::P_IS_MATCH + sp; one = 1; }
                else if (k == 1) { c = (uint32_t)lzma::P_IS_REP + st; one = rep ? 1u : 0u; }
                else if (k == 2) { c = (uint32_t)lzma::P_IS_REP_G0 + st; one = 0; }
                else { c = (uint32_t)lzma::P_IS_REP0_LONG + sp; one = 1; }
            } else if ((k -= nh) < nl) {
                c = lbase + k; one = k == 0 ? (kind > 0) : (kind > 1);
            } else if ((k -= nl) < tb) {
                tree_step(tb, tv, k, m, one); c = tbase + m;
            } else if ((k -= tb) < 6) {
                tree_step(6, slot, k, m, one); c = sbase_cell + m;
            } else if ((k -= 6) < nr) {
                rtree_step(rem, k, m, one); c = (uint32_t)lzma::P_POS_DEC + sb - slot + m;
            } else if ((k -= nr) < nd) {
                dir = true; one = ((rem >> 4) >> (nd - 1 - k)) & 1u;
            } else if ((k -= nd) < na) {
                rtree_step(rem & 15u, k, m, one); c = (uint32_t)lzma::P_ALIGN + m;
            }
            cell[t] = c; bit[t] = one != 0; direct[t] = dir;
        SIMT_END
        code(cell, bit, direct, cnt);
        rep0 = r0;
        state = rep ? (state < 7 ? 8u : 11u) : (state < 7 ? 7u : 10u);
    }

    simt::PT<uint32_t, N> cand, word, hsh;
    simt::PT<bool, N> pb, last;
    // of the lanes that hold the same hash, the highest: one ballot per bit of the hash narrows the set of equals (lz4_comp.h)
    SWC_D void highest_of_equals(uint64_t valid) {
        simt::PT<uint32_t, N> mlo, mhi;
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
    }
    // The window at `pos`: lane t looks position pos + t (inside the chunk, four bytes of the unit behind it) up and enters it.
    // Returns the lanes with a candidate; cand[t]: its distance.
    SWC_D uint64_t window(uint32_t pos, uint32_t cend) {
        SIMT_BEGIN(t, N)
            const uint32_t p = pos + (uint32_t)t;
            const bool ok = p < cend && p + kMinHash <= n;
            const uint32_t w = ok ? load_u32(src + p) : 0u;
            word[t] = w;
            hsh[t] = ok ? hash4(w) : 0u;
            cand[t] = ok ? (uint32_t)lds->table[hsh[t]] : 0u;
            pb[t] = ok;
        SIMT_END_WAVE
        const uint64_t valid = simt::wave_ballot<N>(pb);
        highest_of_equals(valid);
        SIMT_BEGIN(t, N)
            const uint32_t p = pos + (uint32_t)t;
            if (last[t]) lds->table[hsh[t]] = (uint16_t)p;
            const uint32_t d = (p - cand[t]) & 0xFFFFu;   // the entry is the low half of a position: this is the distance
            pb[t] = ((valid >> t) & 1ull) != 0ull && d != 0u && d <= p && load_u32(src + p - d) == word[t];
            cand[t] = d;
        SIMT_END_WAVE
        return simt::wave_ballot<N>(pb);
    }
    // the literals [from, to) of the open chunk; false: the chunk can only be stored
    SWC_D bool literals(uint32_t from, uint32_t to, uint32_t room) {
        simt::PT<uint32_t, N> lit, prv, mbv;
        for (uint32_t a = from; a < to; a += N) {
            const uint32_t cnt = to - a < (uint32_t)N ? to - a : (uint32_t)N;
            const uint32_t r0 = rep0;
            SIMT_BEGIN(t, N)
                const uint32_t p = a + (uint32_t)t;
                const bool ok = (uint32_t)t < cnt;
                lit[t] = ok ? (uint32_t)src[p] : 0u;
                prv[t] = ok && p > 0 ? (uint32_t)src[p - 1] : 0u;
                mbv[t] = ok && p > r0 ? (uint32_t)src[p - r0 - 1] : 0u;
            SIMT_END
            for (uint32_t j = 0; j < cnt; j++) {
                literal(a + j, simt::wave_read<N>(lit, (int)j), simt::wave_read<N>(prv, (int)j), simt::wave_read<N>(mbv, (int)j));
                if (emitted >= room) return false;
            }
        }
        return true;
    }
    // The packets of the chunk [cstart, cend) into the range coder; false: abandoned (header + payload reached 3 + u).
    // room: the payload bytes at which that happens.
    SWC_D bool chunk_packets(uint32_t cstart, uint32_t cend, uint32_t room) {
        uint32_t pos = cstart, anchor = cstart;
        bool alive = true;
        while (pos < cend) {
            const uint64_t m = window(pos, cend);
            uint32_t cur = 0;
            while (alive && cur < (uint32_t)N) {
                const uint64_t m2 = m & ~((cur == 0 ? 0ull : (1ull << cur) - 1ull));
                if (m2 == 0) break;
                const uint32_t f = (uint32_t)simt::ctz64(m2);
                const uint32_t mp = pos + f;
                if (mp < anchor) { cur = f + 1; continue; }     // (inside the match just written)
                const uint32_t d = simt::uniform(simt::wave_read<N>(cand, (int)f));
                const uint32_t c = mp - d, maxlen = cend - mp < kMaxLen ? cend - mp : kMaxLen;
                uint32_t len = maxlen < kMinHash ? maxlen : kMinHash;
                while (len < maxlen) {   // all lanes extend the match, 64 bytes per step
                    SIMT_BEGIN(t, N)
                        const uint32_t i = len + (uint32_t)t;
                        pb[t] = !(i < maxlen && src[mp + i] == src[c + i]);
                    SIMT_END
                    const uint64_t mm = simt::wave_ballot<N>(pb);
                    if (mm) { len += (uint32_t)simt::ctz64(mm); break; }
                    len += N;
                }
                if (len < 2) { cur = f + 1; continue; }         // (one byte in front of the chunk's end: a literal)
                alive = literals(anchor, mp, room);
                if (alive) {
                    match(mp, len, d);
                    alive = emitted < room;
                }
                anchor = mp + len;
                cur = anchor - pos >= (uint32_t)N ? (uint32_t)N : anchor - pos;
            }
            pos = anchor > pos + N ? anchor : pos + N;           // (abandoned: the windows go on, the table is the next chunk's too)
        }
        if (alive) alive = literals(anchor, cend, room);
        return alive;
    }
    SWC_D void put_header(uint64_t at, uint32_t control, uint32_t u, uint32_t p, uint32_t bytes) {
        SIMT_BEGIN(t, N)
            if ((uint32_t)t < bytes && at + (uint32_t)t < cap) {
                const uint32_t v = t == 0 ? control : t == 1 ? (u - 1) >> 8 : t == 2 ? (u - 1) & 0xFFu
                                 : bytes == 3 ? 0u : t == 3 ? (p - 1) >> 8 : t == 4 ? (p - 1) & 0xFFu : kPropsByte;
                out[at + (uint32_t)t] = (uint8_t)v;
            }
        SIMT_END
    }
    // `cnt` bytes src[from ..] -> out + at, all lanes, cut at the capacity
    SWC_D void copy_out(uint64_t at, uint32_t from, uint32_t cnt) {
        const uint32_t keep = at >= cap ? 0u : (cap - at < cnt ? (uint32_t)(cap - at) : cnt);
        SIMT_BEGIN(t, N)
            for (uint32_t i = 8u * (uint32_t)t; i < keep; i += 8u * N) {
                if (i + 8 <= keep) store_u64(out + at + i, load_u64(src + from + i));
                else for (uint32_t j = i; j < keep; j++) out[at + j] = src[from + j];
            }
        SIMT_END
    }

    SWC_D void run(bool segment) {
        SIMT_BEGIN(t, N) for (uint32_t i = (uint32_t)t; i < kHashSize / 2; i += N) ((uint32_t*)lds->table)[i] = 0; SIMT_END_WAVE
        bool fresh = true;   // the next LZMA chunk resets the model: the unit's first, or the one behind a stored chunk
        state = 0; rep0 = 0;
        for (uint32_t cstart = 0; cstart < n; cstart += kChunk) {
            const uint32_t u = n - cstart < kChunk ? n - cstart : kChunk, cend = cstart + u;
            const uint32_t hdr = fresh ? 6u : 5u;
            if (fresh) {
                SIMT_BEGIN(t, N) for (uint32_t i = (uint32_t)t; i < kCells / 2; i += N) ((uint32_t*)lds->probs)[i] = 0x04000400u; SIMT_END_WAVE
                state = 0; rep0 = 0;
            }
            low = 0; range = 0xFFFFFFFFu; cache = 0; cache_size = 1;
            fill = 0; emitted = 0;
            sbase = opos + hdr;
            limit = opos + 3 + u < cap ? opos + 3 + u : cap;
            const uint32_t room = 3 + u > hdr ? 3 + u - hdr : 0u;   // payload bytes at which header + payload reaches 3 + u
            bool lzma_form = chunk_packets(cstart, cend, room);
            if (lzma_form) {
                for (int i = 0; i < 5; i++) shift_low();
                lzma_form = emitted < room;
            }
            if (lzma_form) {
                simt::wave_fence();
                flush(fill);
                put_header(opos, cstart == 0 ? 0xE0u : fresh ? 0xC0u : 0x80u, u, emitted, hdr);
                opos += hdr + emitted;
                fresh = false;
            } else {
                fill = 0;             // (what the attempt still had staged goes nowhere)
                simt::vmem_fence();   // the rows the attempt has stored have arrived: the stored form goes over them
                put_header(opos, cstart == 0 ? 1u : 2u, u, 0, 3);
                copy_out(opos + 3, cstart, u);
                opos += 3 + u;
                fresh = true;
            }
        }
        if (!segment) {
            SIMT_BEGIN(t, N) if (t == 0 && opos < cap) out[opos] = 0; SIMT_END
            opos++;
        }
    }
};

// One wavefront = one job: job.in = the unit, job.aux bit 0 = a segment of a longer stream.  job.out_len = bytes of the run
// (SWC_E_CAPACITY with the size needed if it does not fit out_cap).
template <int N>
SWC_D void lzma2_compress_job(Job& job, Lds* lds) {
    Compressor<N> c;
    c.src = (gcptr)job.in;
    c.out = (gptr)job.out;
    c.cap = simt::uniform(job.out_cap);
    c.opos = 0;
    c.lds = lds;
    int st = SWC_OK;
    if (job.in_len > 0x7E000000ull) st = SWC_E_INVALID_ARGUMENT;
    else {
        c.n = simt::uniform((uint32_t)job.in_len);
        c.run((simt::uniform((uint32_t)job.aux) & 1u) != 0u);
    }
    if (st == SWC_OK && c.opos > c.cap) st = SWC_E_CAPACITY;
    job.out_len = c.opos;
    job.in_consumed = job.in_len;
    job.status = st;
}

}  // namespace lzmac
}  // namespace swc
#endif
