// lz4_chain.h -- the copy phase of LZ4 jobs that have history: chains of linked blocks, stored blocks, adjacent prefixes.
//
// The reference decodes the dependent blocks of a frame one after the other, each against the last 64 KiB of what the frame has
// produced so far (Sources/LZ4/LZ4.swift:306-313; `out` starts as the prefix, :334).  Only the COPY of a block depends on its
// predecessor: the parse (lz4_wave.h) never reads output, so all blocks of all chains are parsed in one launch, with a history
// of 65,536 assumed -- no offset exceeds it -- and the furthest reach in front of the block noted in the stream header.  Here ONE
// wave takes a chain through the copier (lz_copy.h) in order: a block is written directly behind its predecessor, so its history
// is simply the bytes in front of its output, and the wave that wrote them is the wave that reads them -- through the path that
// already reads its own earlier output, after its stores have arrived (s_waitcnt vmcnt(0)).  Nothing waits on another wave.
//
// The job contract is in include/swc_hip.h (SWC_LZ4_LINKED, SWC_LZ4_STORED).
#ifndef SWC_LZ4_CHAIN_H
#define SWC_LZ4_CHAIN_H

#include "swc_common.h"
#include "simt.h"
#include "lz_resolve.h"
#include "lz_copy.h"
#include "lz4_wave.h"

namespace swc {
namespace lz4w {

// n bytes from s to d (both in HBM, any alignment, not overlapping) by all lanes
SWC_D void stored_copy(gptr d, gcptr s, uint64_t n) {
    SIMT_BEGIN(t, 64)
        for (uint64_t i = 8u * (uint64_t)t; i < n; i += 8u * 64u) {
            if (i + 8u <= n) store_u64(d + i, load_u64(s + i));
            else for (uint64_t j = i; j < n; j++) d[j] = s[j];
        }
    SIMT_END_WAVE
}

// The wave of job g: nothing for a linked job (its head's wave carries it); else the job, then the linked jobs behind it in order.
// WS: area(g) / bytes(g), a job's piece of the workspace as the parse left it.
// Linked jobs that NO head can carry -- job 0 with SWC_LZ4_LINKED and the linked jobs behind it; the linked jobs behind a head whose
// prefix is not in place (the lane decoder's job: its output is not where a chain's history has to be) -- report
// SWC_E_INVALID_ARGUMENT with nothing produced, written by the wave of job 0 / of that head: no job keeps the parse's SWC_OK for
// bytes nobody wrote.
// After a failed job every job behind it in the chain reports that job's status with nothing produced: callers take the first
// error in order, which is what the reference throws.
template <typename CFG, int RM, typename WS>
SWC_D void copy_chain(Job* jobs, uint32_t g, uint32_t n, const WS& wm, lzc::Lds<CFG::kWin>* lds) {
    Job job = jobs[g];
    const bool orphan = (job.aux & kLz4Linked) != 0 && g == 0;
    if ((job.aux & kLz4Linked) != 0 && !orphan) return;
    if (orphan || lane_job(job)) {
        for (uint32_t j = orphan ? g : g + 1u; j < n && (jobs[j].aux & kLz4Linked) != 0; j++) {
            SIMT_BEGIN(t, 64)
                if (t == 0) { jobs[j].out_len = 0; jobs[j].in_consumed = 0; jobs[j].status = SWC_E_INVALID_ARGUMENT; }
            SIMT_END
        }
        return;
    }
    // What the chain has produced so far is the next job's history; as long as that is nothing, the head's adjacent prefix is
    // (LZ4.swift:306-313: `out.isEmpty` -- the dictionary counts until the frame has output, and not at all afterwards).
    uint64_t total = 0, prefix = 0;
    int32_t failed = SWC_OK;
    uint8_t* next_out = job.out;
    for (uint32_t j = g;;) {
        const bool head = j == g;
        SWC_LZ4_STAT(5, 1);
        if (head) {
            if (adjacent_prefix(job)) prefix = job.dict_len;
        } else {
            simt::vmem_fence();          // the predecessor's stores have arrived: the far loads and the seam of this job read them
            job.out = next_out;
        }
        const uint64_t behind = total != 0 ? total : prefix;
        const uint32_t hist = behind < 65536u ? (uint32_t)behind : 65536u;
        if (failed != SWC_OK) {
            job.status = failed; job.out_len = 0; job.in_consumed = 0;
        } else if (job.status == SWC_OK && (job.aux & kLz4Stored) != 0) {
            stored_copy((gptr)job.out, (gcptr)job.in, job.in_len);
        } else if ((job.aux & kLz4Stored) == 0 && !(job.status == SWC_E_INVALID_ARGUMENT && job.dict != nullptr && !head)) {
            const uint8_t* area = wm.area(j);
            const size_t bytes = wm.bytes(j);
            // the parse took 65,536 for a linked job's history: what it reached for must lie inside the history that came to be (:382)
            // (whatever the parse's status: the copier trusts every record it finds to stay inside the history)
            const uint32_t reach = head || bytes < sizeof(lzr::StreamHeader) ? 0u
                                 : (uint32_t)(((const SWC_AS_GLOBAL lzr::StreamHeader*)area)->nlit >> 32);
            if (reach > hist) { job.status = SWC_E_DATA_CORRUPTED; job.out_len = 0; job.in_consumed = 0; }
            else lzc::copy_job<CFG, RM>(job, area, bytes, lds, hist);
        }
        if (job.status != SWC_OK) failed = job.status;
        const uint64_t made = job.out_len < job.out_cap ? job.out_len : job.out_cap;
        if (!head) {
            SIMT_BEGIN(t, 64)
                if (t == 0) { jobs[j].out = job.out; jobs[j].out_len = job.out_len; jobs[j].in_consumed = job.in_consumed; jobs[j].status = job.status; }
            SIMT_END
        }
        total += made;
        next_out = job.out + made;
        if (++j >= n) break;
        job = jobs[j];
        if ((job.aux & kLz4Linked) == 0) break;
    }
}

}  // namespace lz4w
}  // namespace swc
#endif
