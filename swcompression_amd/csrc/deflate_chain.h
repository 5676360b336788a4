// deflate_chain.h -- the copy phase of Deflate units that share history (include/swc_hip.h: SWC_DEFLATE_LINKED).
//
// A stream cut at its sync-flush points -- default pigz, Z_SYNC_FLUSH -- is a run of units each of which may refer to the 32,768
// bytes in front of it (Deflate.swift:216-232 reads `out`, which holds everything the stream has produced).  Only the COPY of a unit
// depends on its predecessor: phase 1 (inflate_sync.h) never reads output, so all units are parsed in one launch, a linked unit with
// a full history taken for granted and the furthest reach in front of its first byte noted in its stream header (pad0).  The placing
// scan (deflate_place.h) then puts every unit directly behind its predecessor, so a unit's history is simply the bytes in front of
// its `out`.  Here ONE wave takes a chain -- a job without the bit and the linked jobs behind it -- through the copier (lz_copy.h) in
// order: the wave that wrote the history is the wave that reads it, through the path that already reads its own earlier output,
// after its stores have arrived (s_waitcnt vmcnt(0)).  Nothing waits on another wave.
//
// Every job keeps its own status, as joined jobs do: a failed or over-capacity unit still occupies min(out_len, out_cap) bytes, and
// the units behind it are copied against whatever lies there -- the history never leaves the run's buffer, because it is measured
// from where the chain's head stands.  What phase 1 could not know is checked here: a reach beyond the history that came to be is
// SWC_E_REF_TRAP (the reference's `out[count - distance]` with distance > count), whatever phase 1 reported -- a recorded reach lies
// in front of whatever stopped the parse, so it is what the reference meets first -- with the sizes as phase 1 left them and no byte
// of the unit written.
#ifndef SWC_DEFLATE_CHAIN_H
#define SWC_DEFLATE_CHAIN_H

#include "swc_common.h"
#include "simt.h"
#include "lz_resolve.h"

namespace swc {
namespace defch {

constexpr uint32_t kHistory = 32768;   // the furthest a Deflate distance reaches

// Does job g belong to a chain with a linked member?  (Its copy is the wave copier's then, whatever the size of the launch.)
SWC_HD bool chain_job(const Job* jobs, uint32_t g, uint32_t n) {
    return (jobs[g].aux & kDeflateLinked) != 0 || (g + 1u < n && (jobs[g + 1u].aux & kDeflateLinked) != 0);
}
// nothing of this job exists: joined to nothing (deflate_place.h), linked without being joined (inflate_sync.h), or too long to address
SWC_HD bool absent(const Job& job) { return job.status == SWC_E_INVALID_ARGUMENT && job.out_len == 0; }

// The wave of job g: nothing for a linked job (the wave of its chain's head carries it; a linked job 0 has no head and carries itself
// and what is linked to it: there is nothing of them); else the job, then the linked jobs behind it in order.
// WS: area(g) / bytes(g), a job's piece of the workspace as phase 1 left it.  one(job, j, hist, copy): the copy of job j with `hist`
// bytes of history in place in front of job.out -- copy false: no byte of it is to be written -- and whatever ends the job's wave.
template <typename WS, typename ONE>
SWC_D void copy_chain(Job* jobs, uint32_t g, uint32_t n, const WS& wm, ONE&& one) {
    Job job = jobs[g];
    if ((job.aux & kDeflateLinked) != 0 && g != 0u) return;
    const uint8_t* base = job.out;   // nothing in front of the chain's head is history
    for (uint32_t j = g;;) {
        uint32_t hist = 0;
        bool copy = !absent(job);
        if (j != g) {
            simt::vmem_fence();      // the predecessor's stores have arrived: the far loads and the seam of this job read them
            if ((job.aux & kDeflateJoined) == 0) base = job.out;   // (linked but not joined: it stands somewhere else, with nothing)
            if (copy) {
                const uint64_t behind = (uint64_t)(job.out - base);
                hist = behind < kHistory ? (uint32_t)behind : kHistory;
                // phase 1 took 32,768 for granted: what it reached for must lie inside the history that came to be
                const uint8_t* area = wm.area(j);
                const uint32_t reach = area == nullptr || wm.bytes(j) < sizeof(lzr::StreamHeader) ? 0u
                                     : simt::uniform(((const SWC_AS_GLOBAL lzr::StreamHeader*)area)->pad0);
                if (reach > hist) {
                    copy = false;
                    job.status = SWC_E_REF_TRAP;
                    SIMT_BEGIN(t, 64)
                        if (t == 0) jobs[j].status = SWC_E_REF_TRAP;
                    SIMT_END
                }
            }
        }
        one(job, j, hist, copy);
        if (++j >= n || (jobs[j].aux & kDeflateLinked) == 0) break;   // (one load of `aux`: all a job without a chain pays)
        job = jobs[j];
    }
}

}  // namespace defch
}  // namespace swc
#endif
