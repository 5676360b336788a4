// deflate_place.h -- where the joined units of a Deflate launch go (include/swc_hip.h: SWC_DEFLATE_JOINED).
//
// A stream cut at its flush points is a RUN of jobs: a head and the joined jobs behind it.  Phase 1 (inflate_sync.h) never reads
// or writes `out`, and when it has run every job knows its exact length -- so the units of a run can be laid out back to back
// before a byte is copied: out of a joined job = out of its run's head + the bytes of the jobs in between that exist,
// min(out_len, out_cap) each.  That is a segmented exclusive scan over the job list, done here by one wavefront per TILE of 64
// consecutive jobs between the two phases; the copy kernels then find every job's `out` in its record as they always did.
//
// A tile without a joined job ends after one ballot.  A run that began in an earlier tile is found by looking back tile by tile,
// summing what phase 1 left there: everything read here was written by the previous kernel (or never changes), so no wave waits
// for another and there are no atomics.  Joined jobs with no head in front of them -- job 0 and what is joined to it -- report
// SWC_E_INVALID_ARGUMENT with nothing produced; with out_len = 0 the copy kernels store nothing for them.
#ifndef SWC_DEFLATE_PLACE_H
#define SWC_DEFLATE_PLACE_H

#include "swc_common.h"
#include "simt.h"

namespace swc {
namespace defp {

constexpr int kTile = 64;
// sizes are scanned in two 32-bit halves that need no carry between them: the sum of the tile's (size >> 20) and of its
// (size & 0xFFFFF) -- 64 x 2^20 and 64 x 2^26 fit.  A job's bytes are below 2^46 because made() takes the minimum WITH out_len, which
// phase 1 counted: in_len < 2^32, and Deflate expands 1032 : 1 at most.  Nothing bounds out_cap, and nothing here depends on it.
constexpr uint32_t kLoBits = 20, kLoMask = (1u << kLoBits) - 1u;

SWC_D uint64_t made(const Job* jobs, uint32_t g) {
    const uint64_t a = jobs[g].out_len, b = jobs[g].out_cap;
    return a < b ? a : b;
}

SWC_D void place_tile(Job* jobs, uint32_t n, uint32_t tile) {
    using simt::PT;
    constexpr int N = kTile;
    const uint32_t g0 = tile * (uint32_t)N;
    PT<bool, N> joined;
    PT<uint32_t, N> lo, hi, slo, shi;
    SIMT_BEGIN(t, N)
        const uint32_t g = g0 + (uint32_t)t;
        joined[t] = g < n && (jobs[g].aux & kDeflateJoined) != 0;
    SIMT_END
    const uint64_t jm = simt::wave_ballot<N>(joined);
    if (jm == 0) return;
    SIMT_BEGIN(t, N)
        const uint32_t g = g0 + (uint32_t)t;
        const uint64_t s = g < n ? made(jobs, g) : 0u;
        lo[t] = (uint32_t)s & kLoMask;
        hi[t] = (uint32_t)(s >> kLoBits);
    SIMT_END
    slo = lo;
    shi = hi;
    simt::wave_scan_incl<N>(slo);
    simt::wave_scan_incl<N>(shi);
    // the bytes of the tile in front of every job, and those of the lane its run starts at -- the highest lane below it that is not joined
    PT<uint32_t, N> head, elo, ehi, hlo, hhi, olo, ohi, plo, phi;
    SIMT_BEGIN(t, N)
        const uint64_t e = ((uint64_t)(shi[t] - hi[t]) << kLoBits) + (uint64_t)(slo[t] - lo[t]);
        elo[t] = (uint32_t)e;
        ehi[t] = (uint32_t)(e >> 32);
        const uint64_t below = ~jm & ((1ull << t) - 1ull);   // (lanes past n are not joined, and no joined lane has one below it)
        head[t] = below != 0 ? (uint32_t)simt::top64(below) : (uint32_t)N;
        const uint32_t g = g0 + (uint32_t)t;
        const uint64_t o = g < n ? (uint64_t)(uintptr_t)jobs[g].out : 0u;
        olo[t] = (uint32_t)o;
        ohi[t] = (uint32_t)(o >> 32);
    SIMT_END
    simt::wave_gather<N>(hlo, elo, head);
    simt::wave_gather<N>(hhi, ehi, head);
    simt::wave_gather<N>(plo, olo, head);
    simt::wave_gather<N>(phi, ohi, head);
    // A run that began in an earlier tile (lane 0 is joined): back tile by tile to the one that holds its head.  `base`: where this
    // tile's first job goes.
    uint64_t base = 0;
    bool found = false;
    if ((jm & 1ull) != 0) {
        uint64_t acc = 0;
        for (uint32_t b = tile; b > 0 && !found;) {
            b--;
            const uint32_t p0 = b * (uint32_t)N;   // (a tile in front of this one is full)
            PT<bool, N> pj;
            PT<uint32_t, N> qlo, qhi;
            SIMT_BEGIN(t, N)
                pj[t] = (jobs[p0 + (uint32_t)t].aux & kDeflateJoined) != 0;
            SIMT_END
            const uint64_t heads = ~simt::wave_ballot<N>(pj);
            const int h = heads != 0 ? simt::top64(heads) : 0;   // what counts: the last head of the tile and the jobs behind it, or the whole tile
            SIMT_BEGIN(t, N)
                const uint64_t s = t >= h ? made(jobs, p0 + (uint32_t)t) : 0u;
                qlo[t] = (uint32_t)s & kLoMask;
                qhi[t] = (uint32_t)(s >> kLoBits);
            SIMT_END
            simt::wave_scan_incl<N>(qlo);
            simt::wave_scan_incl<N>(qhi);
            acc += ((uint64_t)simt::wave_read<N>(qhi, N - 1) << kLoBits) + (uint64_t)simt::wave_read<N>(qlo, N - 1);
            if (heads != 0) {
                base = (uint64_t)(uintptr_t)jobs[p0 + (uint32_t)h].out + acc;
                found = true;
            }
        }
    }
    SIMT_BEGIN(t, N)
        if (joined[t]) {
            const uint32_t g = g0 + (uint32_t)t;
            const uint64_t e = ((uint64_t)ehi[t] << 32) | elo[t];
            if (head[t] != (uint32_t)N) {
                const uint64_t eh = ((uint64_t)hhi[t] << 32) | hlo[t], oh = ((uint64_t)phi[t] << 32) | plo[t];
                jobs[g].out = (uint8_t*)(uintptr_t)(oh + (e - eh));
            } else if (found) {
                jobs[g].out = (uint8_t*)(uintptr_t)(base + e);
            } else {   // no head: nothing of this job exists
                jobs[g].out_len = 0;
                jobs[g].in_consumed = 0;
                jobs[g].status = SWC_E_INVALID_ARGUMENT;
            }
        }
    SIMT_END
}

}  // namespace defp
}  // namespace swc
#endif
