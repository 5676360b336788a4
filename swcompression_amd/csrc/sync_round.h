// sync_round.h -- what a sub-chunk-parallel ROUND does whatever the codec: the pieces inflate_sync.h (Deflate) and
// lz4_wave.h (LZ4) share.
//
// A round has 64 lanes decode (parse) 64 sub-chunks of the input speculatively, every lane from where its left neighbour's
// walk ended, into the wave's row-major scratch in the workspace (lz_resolve.h: row k = the k-th record / literal group of all
// 64 lanes).  What follows is the same for both codecs and lives here:
//   chain_check   how far does the chain of (my start == my left neighbour's end) hold, and does a lane inside it stop?
//   lane_offsets  three wave scans give every lane of the chain its offsets, and the round its totals;
//   copy_prov     a lane's rows move from the scratch to their final place.
// In the vocabulary of simt.h: PT values in and out, called BETWEEN regions (copy_prov: inside one, per lane).  Everything is
// force-inlined and takes its PT values by reference: the Deflate kernel has no register to spare.
#ifndef SWC_SYNC_ROUND_H
#define SWC_SYNC_ROUND_H

#include "swc_common.h"
#include "simt.h"
#include "lz_resolve.h"

namespace swc {
namespace sround {

constexpr uint32_t kProvRow = 64u * 4u;   // bytes from one row of the scratch to the next (records and literal groups alike)

// the lanes [0, nv)
SWC_D uint64_t lanes_below(uint32_t nv) { return nv == 64u ? ~0ull : (1ull << nv) - 1ull; }

struct Chain {
    int b;         // lanes [0, b) are on the true sequence: each was decoded from the end of its left neighbour (64: all)
    int E;         // the first stopped lane among them (64: none)
    uint32_t nv;   // the lanes the round can commit: up to and including the stopped one, or the chain
};
// `pe`: the ends shifted up one lane, `first` -- where the round begins -- entering at lane 0.  A lane is final when it HAS been
// decoded (`have`) from the end of a final left neighbour; a lane counts as stopped when (flg & stop_bits) != 0.  A stop inside
// the chain beats the break behind it; a stop at or behind the break does not count.
template <int N>
SWC_D Chain chain_check(simt::PT<uint32_t, N>& pe, const simt::PT<uint32_t, N>& start, const simt::PT<uint32_t, N>& endp,
                        const simt::PT<bool, N>& have, const simt::PT<uint32_t, N>& flg, uint32_t first, uint32_t stop_bits) {
    simt::PT<bool, N> pb;
    simt::wave_shift_up<N>(pe, endp, first);
    SIMT_BEGIN(t, N) pb[t] = !(have[t] && (t == 0 || start[t] == pe[t])); SIMT_END
    const uint64_t m_bad = simt::wave_ballot<N>(pb);
    Chain c;
    c.b = m_bad ? simt::ctz64(m_bad) : 64;
    SIMT_BEGIN(t, N) pb[t] = (flg[t] & stop_bits) != 0u; SIMT_END
    const uint64_t m_stop = simt::wave_ballot<N>(pb) & lanes_below((uint32_t)c.b);
    c.E = m_stop ? simt::ctz64(m_stop) : 64;
    c.nv = (uint32_t)(c.E < 64 ? c.E + 1 : c.b);
    return c;
}

struct Totals {
    uint32_t lit, rec, out;
};
// Inclusive sums of the counts of the lanes [first_lane, nv) -- a lane's exclusive offset is x[t] - c[t] -- and their totals.
// The lanes outside count as zero in the sums; their counts stay as they are.
template <int N>
SWC_D Totals lane_offsets(uint32_t first_lane, uint32_t nv, const simt::PT<uint32_t, N>& c_lit, const simt::PT<uint32_t, N>& c_rec,
                          const simt::PT<uint32_t, N>& c_out, simt::PT<uint32_t, N>& x_lit, simt::PT<uint32_t, N>& x_rec,
                          simt::PT<uint32_t, N>& x_out) {
    SIMT_BEGIN(t, N)
        const bool v = (uint32_t)t >= first_lane && (uint32_t)t < nv;
        x_lit[t] = v ? c_lit[t] : 0u; x_rec[t] = v ? c_rec[t] : 0u; x_out[t] = v ? c_out[t] : 0u;
    SIMT_END
    simt::wave_scan_incl<N>(x_lit);
    simt::wave_scan_incl<N>(x_rec);
    simt::wave_scan_incl<N>(x_out);
    return Totals{simt::wave_read<N>(x_lit, N - 1), simt::wave_read<N>(x_rec, N - 1), simt::wave_read<N>(x_out, N - 1)};
}

// A lane's piece of the round moves from its column of the scratch to its final place: `nrec` records to `rdst` (dword
// aligned), `nlit` literal bytes to `ldst` (any alignment).  The loads of a step read one row: coalesced.  The last,
// incomplete literal group holds its bytes at the top of its dword (TOP) or at the bottom.  LIT == 0: records only.
template <uint32_t REC, uint32_t LIT, bool TOP>
SWC_D void copy_prov(gcptr plit, gcptr prec, uint32_t nlit, uint32_t nrec, gptr ldst, SWC_AS_GLOBAL uint32_t* rdst) {
    // REC records and LIT literal groups are loaded per step, all before the first store (the scratch of all
    // resident waves exceeds the L2, so a load takes its several hundred cycles: one load per step would expose that latency
    // forty times per round; a step lasts as long as the slowest lane's, so the sizes aim at ONE step for a sub-chunk of text --
    // 23 records and 19 literals on average).  Rows past the lane's count hold something and exist (the scratch is sized for
    // the worst case): they are loaded and not stored.
    static_assert(REC % 4u == 0 && LIT % 4u == 0 && REC != 0, "wide stores take four records or four groups");
    const uint32_t ngrp = LIT != 0 ? (nlit + 3u) >> 2 : 0u;
    for (uint32_t i = 0, g = 0; i < nrec || g < ngrp; i += REC, g += LIT) {
        uint32_t v[REC], w[LIT != 0 ? LIT : 1u];
#pragma unroll
        for (uint32_t k = 0; k < REC; k++) {
            const uint32_t row = i + k + 1u < (uint32_t)lzr::kProvRecRows ? i + k + 1u : (uint32_t)lzr::kProvRecRows - 1u;
            v[k] = load_u32(prec + (size_t)row * kProvRow);
        }
#pragma unroll
        for (uint32_t k = 0; k < LIT; k++) {
            const uint32_t row = g + k + 1u < (uint32_t)lzr::kProvLitRows ? g + k + 1u : (uint32_t)lzr::kProvLitRows - 1u;
            w[k] = load_u32(plit + (size_t)row * kProvRow);
        }
        // (wide stores: the lanes' destinations lie apart, so the memory pipeline takes a store lane by lane -- four records or
        // four groups per lane and instruction instead of one)
#pragma unroll
        for (uint32_t k = 0; k < REC; k += 4) {
            if (i + k + 4u <= nrec) store_u128_a4((gptr)(rdst + i + k), v[k], v[k + 1], v[k + 2], v[k + 3]);
            else {
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) if (i + k + q < nrec) rdst[i + k + q] = v[k + q];
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < LIT; k += 4) {
            const uint32_t at = 4u * (g + k);
            if (at + 16u <= nlit) store_u128_a4(ldst + at, w[k], w[k + 1], w[k + 2], w[k + 3]);
            else {
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) {
                    const uint32_t aq = at + 4u * q;
                    if (aq + 4u <= nlit) store_u32(ldst + aq, w[k + q]);
                    else if (aq < nlit) {
                        uint32_t x = TOP ? w[k + q] >> (8u * (4u - (nlit - aq))) : w[k + q];
                        for (uint32_t z = aq; z < nlit; z++, x >>= 8) ldst[z] = (uint8_t)x;
                    }
                }
            }
        }
    }
}

}  // namespace sround
}  // namespace swc
#endif
