// huffman_wave.h -- a length-limited Huffman code built by one wavefront, shared by the bzip2 encoder (bzip2_comp.h, its
// `Huff` stage: up to 258 symbols, 17 bits) and the Deflate encoder's dynamic blocks (deflate_comp.h: 286 lit/len symbols
// and 30 distance symbols at 15 bits, 19 code-length symbols at 7 bits).
//
// The caller fills l->w[0 .. alpha) with the weights of the symbols it wants codes for (every weight >= 1, alpha >= 2 for a
// complete code) and gets l->len[s] and, in l->wt[s], the canonical code of symbol s in the order of (length, symbol) --
// RFC 1951 3.2.2, and what bzip2 assigns -- as (code | length << 24), most significant code bit first.
#ifndef SWC_HUFFMAN_WAVE_H
#define SWC_HUFFMAN_WAVE_H

#include "swc_common.h"
#include "simt.h"

namespace swc {
namespace huff {

// LDS of one build for an alphabet of up to CAP symbols (7 x CAP + 48 words)
template <uint32_t CAP>
struct HuffLds {
    uint32_t w[CAP];                 // weights
    uint32_t order[CAP];             // symbols by weight
    uint32_t wt[CAP];                // inner nodes, in order of creation (= of weight)
    uint32_t parent_leaf[CAP];
    uint32_t parent_inner[CAP];
    uint32_t depth_inner[CAP];
    uint32_t len[CAP];
    uint32_t count[24], base[24];
};
// Code lengths (no code longer than max_len: weights halved until that holds, as bzip2's hbMakeCodeLengths does) and canonical
// codes of one table from the weights of its symbols.
template <int N, uint32_t CAP>
SWC_D void huffman_wave(HuffLds<CAP>* l, uint32_t alpha, uint32_t max_len) {
    using simt::PT;
    for (;;) {
        // ---- the symbols in order of weight (ties: by symbol): every lane ranks its symbols against all
        SIMT_BEGIN(t, N)
            for (uint32_t s = (uint32_t)t; s < alpha; s += (uint32_t)N) {
                const uint32_t ws = l->w[s];
                uint32_t r = 0;
                for (uint32_t k = 0; k < alpha; k++) { const uint32_t wk = l->w[k]; r += wk < ws || (wk == ws && k < s) ? 1u : 0u; }
                l->order[r] = s;
            }
        SIMT_END_WAVE
        // ---- two queues: the lightest two of (next leaf, next inner node) are joined; inner nodes come into being in order of weight
        uint32_t made = 0;
        SIMT_BEGIN(t, N)
            if (t == 0) {
                uint32_t nl = 0, ni = 0, m = 0;
                while (alpha - nl + m - ni > 1u) {
                    uint32_t sum = 0;
                    for (int k = 0; k < 2; k++) {
                        if (nl < alpha && (ni >= m || l->w[l->order[nl]] <= l->wt[ni])) { const uint32_t s = l->order[nl++]; l->parent_leaf[s] = m; sum += l->w[s]; }
                        else { l->parent_inner[ni] = m; sum += l->wt[ni++]; }
                    }
                    l->wt[m] = sum;
                    l->parent_inner[m] = 0xFFFFFFFFu;
                    m++;
                }
                for (uint32_t k = m; k-- > 0u;) l->depth_inner[k] = l->parent_inner[k] == 0xFFFFFFFFu ? 0u : l->depth_inner[l->parent_inner[k]] + 1u;
                l->count[23] = m;
            }
        SIMT_END_WAVE
        made = l->count[23];
        PT<uint32_t, N> mx;
        SIMT_BEGIN(t, N)
            uint32_t m = 0;
            for (uint32_t s = (uint32_t)t; s < alpha; s += (uint32_t)N) {
                const uint32_t d = made ? l->depth_inner[l->parent_leaf[s]] + 1u : 1u;
                l->len[s] = d;
                m = d > m ? d : m;
            }
            mx[t] = m;
        SIMT_END_WAVE
        simt::wave_scan_max_incl<N>(mx);
        if (simt::wave_read<N>(mx, N - 1) <= max_len) break;
        SIMT_BEGIN(t, N) for (uint32_t s = (uint32_t)t; s < alpha; s += (uint32_t)N) l->w[s] = l->w[s] / 2u + 1u; SIMT_END_WAVE
    }
    // ---- canonical codes: in order of (length, symbol)
    SIMT_BEGIN(t, N) if (t < 24) l->count[t] = 0u; SIMT_END_WAVE
    SIMT_BEGIN(t, N) for (uint32_t s = (uint32_t)t; s < alpha; s += (uint32_t)N) simt::lds_add(&l->count[l->len[s]], 1u); SIMT_END_WAVE
    SIMT_BEGIN(t, N)
        if (t == 0) {
            uint32_t next = 0;
            for (uint32_t k = 1; k <= max_len; k++) { l->base[k] = next; next = (next + l->count[k]) << 1; }
        }
    SIMT_END_WAVE
    SIMT_BEGIN(t, N)
        for (uint32_t s = (uint32_t)t; s < alpha; s += (uint32_t)N) {
            const uint32_t ls = l->len[s];
            uint32_t r = 0;
            for (uint32_t k = 0; k < s; k++) r += l->len[k] == ls ? 1u : 0u;
            l->wt[s] = (l->base[ls] + r) | (ls << 24);        // (the inner weights are not needed any more)
        }
    SIMT_END_WAVE
}

}  // namespace huff
}  // namespace swc
#endif
