// job_kernels.h -- what every kernel of kernels.hip and inflate_team.hip that takes a job list does once it knows its job index g:
// which jobs it skips, with which template arguments the codec header runs, what goes back into the job record, when the fused
// CRC is taken.  Written once: a __global__ function declares its LDS, finds g and calls its body here; the host emulation
// (tests/host_emu, g++ -DSWC_HOST_EMULATION) calls the same bodies in the order the launchers issue the kernels, with `lane` in
// place of threadIdx.x and a wave width of 1 where the codec header takes one.  The launchers -- which kernels, in which order, with
// which flags -- are kernels.hip's.
//
// WS: a job's area of the workspace, area(g) / bytes(g) -- WsMap on the device; the emulation brings a map of its own that keeps one
// exact allocation per job.
#ifndef SWC_JOB_KERNELS_H
#define SWC_JOB_KERNELS_H

#include "swc_common.h"
#include "simt.h"
#include "inflate_lane.h"
#include "inflate_sync.h"
#include "lz_resolve.h"
#include "lz_copy.h"
#include "deflate_chain.h"
#include "lz4_lane.h"
#include "lz4_wave.h"
#include "lz4_chain.h"
#include "lz4_comp.h"
#include "deflate_comp.h"
#include "lzma_comp.h"
#include "lzma_wave.h"
#include "bzip2_block.h"
#include "bzip2_team.h"
#include "crc32_group.h"
#include "crc32_wave.h"
#include "crc32_tail.h"
#include "sha256_lane.h"

namespace swc {

// A job's area of the workspace: equal strides, or -- `ws_off` given -- prefix-summed per-job sizes (ws_off[n] = total),
// so that one large unit among many small ones does not size everybody's area.
// (The members are NOT forced inline, as before they moved here: forced, they change the order in which the inliner takes the
// callers' code, and swc_inflate_team_kernel comes out as another kernel -- 153 registers and no scratch against 217 and 32 bytes.
// That other kernel may well be the better one; it is a change of its own, to be measured on launches of few streams, and with it
// this macro goes.)
#if defined(__HIPCC__) && !defined(SWC_HOST_EMULATION)
#define SWC_WSMAP_HD __host__ __device__
#else
#define SWC_WSMAP_HD
#endif
struct WsMap {
    uint8_t* base;
    size_t stride;
    const uint64_t* off;
    SWC_WSMAP_HD uint8_t* area(uint32_t g) const { return base ? base + (off ? (size_t)off[g] : (size_t)g * stride) : nullptr; }
    SWC_WSMAP_HD size_t bytes(uint32_t g) const { return off ? (size_t)(off[g + 1] - off[g]) : stride; }
};

// Which job does workgroup `b` of an n-job launch take?  The hardware hands consecutive workgroups to the eight XCDs in turn
// (workgroup b runs on XCD b % 8), so a job list whose cost has a period that divides 8 -- every fourth unit an incompressible
// one, say -- would put all the expensive jobs on two XCDs and the launch would last as long as if every job were expensive
// (measured: 192 text + 64 P-mix LZ4 blocks interleaved 3 : 1 took exactly the time of 256 P-mix blocks).  Here XCD x works
// through the contiguous range [x n/8, (x + 1) n/8) of the list instead, in order: any eighth of the list costs about the same.
SWC_HD uint32_t xcd_job(uint32_t b, uint32_t n) {
    const uint32_t per = n >> 3;
    return b < (per << 3) ? (b & 7u) * per + (b >> 3) : b;
}

// the bytes of a job's output that exist: what it produced, or its capacity if it needed more
SWC_HD uint64_t made_bytes(uint64_t out_len, uint64_t out_cap) { return out_len < out_cap ? out_len : out_cap; }

// Deflate phase 2 by a workgroup: 512 threads, 64 KiB LDS ring (32 KiB of history + span + cells) -> 2 workgroups per CU
constexpr int kInflateResolveThreads = 512, kInflateRingLog2 = 16;
constexpr uint32_t kInflateKeep = 32768;
constexpr uint64_t kCrcGroupLen = 1u << 20;   // CRC-32 of a stream: by one wave below, by a 256-thread group from here on
// how the LZ4 parse tells the copy kernel where a record's literals lie in the block (lz4_wave.h): 1 = eight-byte records with the
// offset in the upper dword, 2 = four-byte records, the offset derived by a running sum, anchors where the rule breaks
#ifndef SWC_LZ4_RECORD_MODE
#define SWC_LZ4_RECORD_MODE 2
#endif
// LZMA: every literal coder of lc + lp <= 12, then the two `high` length trees
constexpr size_t kLzmaSpillBytes = (size_t)(0x300u << 12) * 2 + 1024;
// BZip2: the three stages' LDS areas share one allocation
constexpr size_t kBzLdsBytes = bzip2::kStage1LdsBytes > sizeof(bzip2::Stage3Lds) ? (size_t)bzip2::kStage1LdsBytes : sizeof(bzip2::Stage3Lds);
static_assert(kBzLdsBytes >= 256 * sizeof(uint32_t), "stage 2 counters");

namespace jobk {

SWC_HD uint64_t* prof_of(uint64_t* prof, uint32_t g, int phase) { return prof ? prof + 32 * (size_t)g + 16 * phase : nullptr; }
// what some lanes wrote to global memory is read by all of them from here on
SWC_D void block_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
    __threadfence_block();
#endif
}

// ---- Deflate ------------------------------------------------------------------------------------------------------------------
// swc_inflate_sync_kernel: phase 1, one stream per wavefront
template <int WAVE, typename WS>
SWC_D void inflate_sync(Job* __restrict__ jobs, uint32_t g, const WS& wm, inflate::SyncLds* lds, int lane, uint64_t* prof) {
    Job job = jobs[g];
    inflate::inflate_sync_job(job, lds, wm.area(g), wm.bytes(g), lane, WAVE, prof_of(prof, g, 0));
    if (lane == 0) put_result<true>(jobs, g, job);   // (aux: SWC_DEFLATE_OPEN is an OUT bit)
}

// swc_inflate_team_kernel: phase 1 by a team of wavefronts -- wave 0 the master on the job, the others the helpers on the rounds
// behind the master's.  `scratch`: (kTeamWaves - 1) * kTeamProvBytes per stream, the helpers' rows.
constexpr size_t kTeamScratchBytes = (size_t)(inflate::kTeamWaves - 1) * inflate::kTeamProvBytes;
template <int WAVE, typename WS>
SWC_D void inflate_team(Job* __restrict__ jobs, uint32_t g, const WS& wm, uint8_t* __restrict__ scratch, inflate::SyncLds* team_lds,
                        inflate::TeamShared* team_shared, int lane, int wave) {
    inflate::Team tm;
    tm.sh = team_shared;
    tm.lds = team_lds;
    tm.scratch = (gptr)(scratch + (size_t)g * kTeamScratchBytes);
    tm.helpers = inflate::kTeamWaves - 1;
    tm.gen = 0;
    if (wave == 0) {
        SIMT_BEGIN(t, 64)
            if (t < inflate::kTeamWaves) team_shared->hgen[t] = 0u;   // (the master's first barrier comes later)
            if (t == 0) team_shared->cmd = 0u;
        SIMT_END
        Job job = jobs[g];
        inflate::inflate_sync_job<true>(job, &team_lds[0], wm.area(g), wm.bytes(g), lane, WAVE, nullptr, &tm);
        if (lane == 0) put_result<true>(jobs, g, job);   // (aux: SWC_DEFLATE_OPEN is an OUT bit)
    } else {
        inflate::team_helper_loop(tm, wave);
    }
}

// swc_lz_resolve_kernel: phase 2 by a workgroup, byte cells in LDS
template <typename WS>
SWC_D void lz_resolve(const Job* __restrict__ jobs, uint32_t g, const WS& wm, lzr::Lds<kInflateResolveThreads, kInflateRingLog2>* lds, uint64_t* prof) {
    Job job = jobs[g];
    lzr::resolve_job<kInflateResolveThreads, kInflateRingLog2, kInflateKeep>(job, wm.area(g), wm.bytes(g), lds, prof_of(prof, g, 1));
}
// ... as a launch below the wave copier's threshold runs it: the chains with a linked member are the wave copier's, behind this kernel
template <typename WS>
SWC_D void lz_resolve_unlinked(const Job* __restrict__ jobs, uint32_t g, uint32_t n, const WS& wm, lzr::Lds<kInflateResolveThreads, kInflateRingLog2>* lds, uint64_t* prof) {
    if (defch::chain_job(jobs, g, n)) return;
    lz_resolve(jobs, g, wm, lds, prof);
}

// swc_lz_copy_kernel and, CRC, swc_lz_copy_crc32_kernel: phase 2 by a wavefront.  CRC: when copy_job has returned -- on whichever
// path: no literal stream, no records, a failed stream -- the window is dead, and the wave ends with the CRC-32 of its own output
// in crcs[g] (crc32_tail.h).
template <typename CFG, bool CRC, typename WS>
SWC_D void lz_copy(const Job* __restrict__ jobs, uint32_t g, const WS& wm, lzc::Lds<CFG::kWin>* lds, int lane, uint32_t* __restrict__ crcs = nullptr,
                   const crcw::WaveConsts* consts = nullptr) {
    Job job = jobs[g];
    if constexpr (!CRC) {
        if (job.dict != nullptr) return;   // (LZ4 blocks with a dictionary prefix were decoded by the lane kernel)
        lzc::copy_job<CFG>(job, wm.area(g), wm.bytes(g), lds);
    } else {
        static_assert(sizeof(crct::TailConsts) <= CFG::kWin, "the constants of the tail go where the window was");
        if (job.dict == nullptr) lzc::copy_job<CFG>(job, wm.area(g), wm.bytes(g), lds);
        // what swc_batch_crc32 covers; streams of a megabyte and more (the 64-bit positions among them) are left to
        // swc_crc32_group_kernel, which the launch puts behind this kernel
        const uint64_t len = made_bytes(job.out_len, job.out_cap);
        if (len >= kCrcGroupLen) return;
        simt::vmem_fence();   // every store of this wave has arrived (what drain() waits for)
        const uint32_t c = crct::crc32_tail((gcptr)job.out, simt::uniform((uint32_t)len), (crct::TailConsts*)lds->win, consts);
        if (lane == 0) crcs[g] = c;
    }
}

// ... as swc_lz_copy_kernel and swc_lz_copy_crc32_kernel run it: the chains with a linked member are swc_deflate_chain_kernel's
template <typename CFG, bool CRC, typename WS>
SWC_D void lz_copy_unlinked(const Job* __restrict__ jobs, uint32_t g, uint32_t n, const WS& wm, lzc::Lds<CFG::kWin>* lds, int lane, uint32_t* __restrict__ crcs = nullptr,
                            const crcw::WaveConsts* consts = nullptr) {
    if (defch::chain_job(jobs, g, n)) return;
    lz_copy<CFG, CRC>(jobs, g, wm, lds, lane, crcs, consts);
}

// The chain copy of swc_deflate_chain_kernel and, CRC, swc_deflate_chain_crc32_kernel, behind the copy kernels of every Deflate launch
// (deflate_chains below finds the heads): the wave of a job takes the linked jobs behind it along, one after the other (deflate_chain.h: SWC_DEFLATE_LINKED); it writes the status of those that
// reached beyond their history, so the job list is not read-only here.  A job without a chain is copied as lz_copy copies it.
// CRC: crcs[j] for every job the wave carried -- the window is dead between two jobs of a chain just as it is at the end.
// only_chain: the launch's other jobs are another kernel's -- swc_lz_copy_kernel's or swc_lz_resolve_kernel's -- as in every launch.
template <typename CFG, bool CRC, typename WS>
SWC_D void deflate_copy(Job* jobs, uint32_t g, uint32_t n, const WS& wm, lzc::Lds<CFG::kWin>* lds, int lane, int only_chain, uint32_t* __restrict__ crcs = nullptr,
                        const crcw::WaveConsts* consts = nullptr) {
    if (only_chain && !defch::chain_job(jobs, g, n)) return;
    defch::copy_chain(jobs, g, n, wm, [&](const Job& job, uint32_t j, uint32_t hist, bool copy) {
        if (copy && job.dict == nullptr) lzc::copy_job<CFG, 0, true>(job, wm.area(j), wm.bytes(j), lds, hist);
        if constexpr (CRC) {
            static_assert(sizeof(crct::TailConsts) <= CFG::kWin, "the constants of the tail go where the window was");
            const uint64_t len = made_bytes(job.out_len, job.out_cap);
            if (len >= kCrcGroupLen) return;   // (swc_crc32_group_kernel's, behind this kernel)
            simt::vmem_fence();   // every store of this wave has arrived (what drain() waits for)
            const uint32_t c = crct::crc32_tail((gcptr)job.out, simt::uniform((uint32_t)len), (crct::TailConsts*)lds->win, consts);
            if (lane == 0) crcs[j] = c;
        }
    });
}

// What a wave of swc_deflate_chain_kernel does: it looks at the tiles of 64 consecutive jobs tile, tile + step, ... -- one load of `aux`
// per lane and one of its right neighbour's -- and copies every chain that begins there, one after the other.  A launch without a
// linked job (every launch of section 5) costs a few hundred waves a ballot each, not a wave per job.
template <typename CFG, bool CRC, typename WS>
SWC_D void deflate_chains(Job* jobs, uint32_t tile, uint32_t step, uint32_t n, const WS& wm, lzc::Lds<CFG::kWin>* lds, int lane, uint32_t* __restrict__ crcs = nullptr,
                          const crcw::WaveConsts* consts = nullptr) {
    constexpr int N = 64;
    for (uint64_t g0 = (uint64_t)tile * N; g0 < n; g0 += (uint64_t)step * N) {
        simt::PT<bool, N> head;
        SIMT_BEGIN(t, N)
            const uint32_t g = (uint32_t)g0 + (uint32_t)t;
            const bool linked = g < n && (jobs[g].aux & kDeflateLinked) != 0;
            const bool next = g + 1u < n && (jobs[g + 1u].aux & kDeflateLinked) != 0;
            head[t] = g < n && (linked ? g == 0u : next);   // (a linked job 0 has no head: its wave carries what there is of it)
        SIMT_END
        for (uint64_t m = simt::wave_ballot<N>(head); m; m &= m - 1u)
            deflate_copy<CFG, CRC>(jobs, (uint32_t)g0 + (uint32_t)simt::ctz64(m), n, wm, lds, lane, 0, crcs, consts);
    }
}

// ---- LZ4: each kernel skips the jobs of the other kinds -----------------------------------------------------------------------
SWC_HD int32_t lz4_next_aux(const Job* jobs, uint32_t g, uint32_t n) { return g + 1u < n ? jobs[g + 1u].aux : 0; }

// swc_lz4_lane_kernel: one block per LANE.  only_dict: the launch has a workspace, and only the jobs whose prefix lies somewhere
// else are this kernel's.
SWC_D void lz4_lane(Job* __restrict__ jobs, uint32_t g, int only_dict) {
    Job job = jobs[g];
    if (only_dict) {
        if (!lz4w::lane_job(job)) return;
    } else if ((job.aux & (kLz4Linked | kLz4Stored)) != 0) {   // (no workspace: nowhere to leave the records of a chain)
        job.status = SWC_E_NEED_WORKSPACE; job.out_len = 0; job.in_consumed = 0;
        put_result(jobs, g, job);
        return;
    }
    SWC_LZ4_STAT(5, 1);
    lz4::lz4_block_job(job);
    put_result(jobs, g, job);
}

// swc_lz4_parse_kernel<RM>.  which: 0 = every job that is not the lane decoder's, 1 = only the jobs of lz4w::chain_job (chains,
// stored blocks, adjacent prefixes: always RM != 0 and the wave copier), 2 = only the others.
template <int WAVE, int RM, typename WS>
SWC_D void lz4_parse(Job* __restrict__ jobs, uint32_t g, uint32_t n, const WS& wm, uint8_t* stage, int lane, uint64_t* prof, int which) {
    Job job = jobs[g];
    if (lz4w::lane_job(job)) return;
    if (which != 0 && lz4w::chain_job(job, lz4_next_aux(jobs, g, n)) != (which == 1)) return;
    uint64_t hist = 0;
    if (RM == 0 || !lz4w::parse_preset(job, hist))
        lz4w::lz4_parse_job<WAVE, RM>(job, wm.area(g), wm.bytes(g), lane, stage, prof_of(prof, g, 0), RM == 0 ? 0u : hist);
    if (lane == 0) put_result(jobs, g, job);
}

// swc_lz4_resolve_kernel: the jobs without history of a launch below the copier's threshold
template <typename WS>
SWC_D void lz4_resolve(const Job* __restrict__ jobs, uint32_t g, uint32_t n, const WS& wm, lzr::Lds<lz4w::kResolveThreads, lz4w::kRingLog2>* lds, uint64_t* prof) {
    Job job = jobs[g];
    if (lz4w::lane_job(job) || lz4w::chain_job(job, lz4_next_aux(jobs, g, n))) return;
    SWC_LZ4_STAT(5, 1);
    lzr::resolve_job<lz4w::kResolveThreads, lz4w::kRingLog2, lz4w::kKeep, true>(job, wm.area(g), wm.bytes(g), lds, prof_of(prof, g, 1));
}

// swc_lz4_copy_kernel: the wave of a job takes the linked jobs behind it along, one after the other (lz4_chain.h); it writes their
// `out` and their results, so the job list is not read-only here.  only_chain: the launch's other jobs are swc_lz4_resolve_kernel's.
// (CFG, RM: the shipped window and record form; the emulation's tests swap them)
template <typename WS, typename CFG = lzc::CfgLz4, int RM = SWC_LZ4_RECORD_MODE>
SWC_D void lz4_copy(Job* jobs, uint32_t g, uint32_t n, const WS& wm, lzc::Lds<CFG::kWin>* lds, int only_chain) {
    if (only_chain && !lz4w::chain_job(jobs[g], lz4_next_aux(jobs, g, n))) return;
    lz4w::copy_chain<CFG, RM>(jobs, g, n, wm, lds);   // (the literals come from the block itself)
}

// ---- compression: swc_lz4_compress_kernel, swc_deflate_compress_kernel, swc_deflate_compress_dynamic_kernel -------------------
template <int WAVE>
SWC_D void lz4_compress(Job* __restrict__ jobs, uint32_t g, uint16_t* table, int lane) {
    Job job = jobs[g];
    lz4c::lz4_compress_job<WAVE>(job, table);
    if (lane == 0) put_result(jobs, g, job);
}
template <int WAVE>
SWC_D void deflate_compress(Job* __restrict__ jobs, uint32_t g, defc::Lds* lds, int lane) {
    Job job = jobs[g];
    defc::deflate_compress_job<WAVE>(job, lds);
    if (lane == 0) put_result(jobs, g, job);
}
template <int WAVE>
SWC_D void deflate_compress_dynamic(Job* __restrict__ jobs, uint32_t g, defc::DynLds* lds, int lane) {
    Job job = jobs[g];
    defc::deflate_compress_dynamic_job<WAVE>(job, lds);
    if (lane == 0) put_result(jobs, g, job);
}

// swc_lzma2_compress_kernel (lzma_compress.hip)
template <int WAVE>
SWC_D void lzma2_compress(Job* __restrict__ jobs, uint32_t g, lzmac::Lds* lds, int lane) {
    Job job = jobs[g];
    lzmac::lzma2_compress_job<WAVE>(job, lds);
    if (lane == 0) put_result(jobs, g, job);
}

// ---- swc_lzma_kernel<LZMA2, LDSBITS>; `spill` holds kLzmaSpillBytes per job ---------------------------------------------------
template <int WAVE, bool LZMA2, int LDSBITS>
SWC_D void lzma_stream(Job* __restrict__ jobs, uint32_t g, uint8_t* spill, uint16_t* lds, int lane, uint64_t* prof) {
    Job job = jobs[g];
    SWC_AS_GLOBAL uint16_t* sp = spill ? (SWC_AS_GLOBAL uint16_t*)(spill + (size_t)g * kLzmaSpillBytes) : nullptr;
    lzma::lzma_job<WAVE>(job, LZMA2, lds, sp, lane, LDSBITS < 0 ? 0 : LDSBITS, prof_of(prof, g, 0), LDSBITS < 0);
    if (lane == 0) {
        // (aux: SWC_LZMA2_OPEN is an OUT bit.  Read again from the record, so that the decode keeps nothing of it but the dictionary byte)
        if (LZMA2) job.aux = lzma::lzma2_end(job, *(const volatile int32_t*)&jobs[g].aux);
        put_result<LZMA2>(jobs, g, job);
    }
}

// ---- BZip2 --------------------------------------------------------------------------------------------------------------------
// swc_bzip2_block_kernel<CXX>: stage 1, 2 and 3a back to back; team != 0: stage 1 and 2 only.  `lds`: kBzLdsBytes.
template <int WAVE, bool CXX>
SWC_D void bzip2_block(Job* __restrict__ jobs, uint32_t g, uint8_t* ws, size_t lcap, uint8_t* lds, int lane, int team) {
    Job job = jobs[g];
    const bzip2::Workspace w = bzip2::carve(ws, g, lcap);
    bzip2::stage1_job<WAVE, CXX>(job, reinterpret_cast<bzip2::Stage1Lds*>(lds), w, lane);
    block_fence();   // L and the block header, written by some lanes, are read by all of them from here on
    bzip2::stage2_job(w, reinterpret_cast<uint32_t*>(lds));
    if (team) return;
    block_fence();   // likewise the pointer array P
    bzip2::stage3_walk_job<WAVE>(job, w, reinterpret_cast<bzip2::Stage3Lds*>(lds), lane);
    if (lane == 0 && !bzip2::stage3_expand_needed(w)) put_result<true>(jobs, g, job);
}
// swc_bzip2_team_finish_kernel: the lay-out and the RLE1 undo behind the team walk
template <int WAVE>
SWC_D void bzip2_team_finish(Job* __restrict__ jobs, uint32_t g, uint8_t* ws, size_t lcap, bzip2::FinishLds* lds, int lane) {
    Job job = jobs[g];
    const bzip2::Workspace w = bzip2::carve(ws, g, lcap);
    bzip2::team_finish<WAVE>(job, w, lds, lane);
    if (lane == 0 && !bzip2::stage3_expand_needed(w)) put_result<true>(jobs, g, job);
}
// swc_bzip2_expand_kernel, stage 3b: one block per LANE, only what stage 3a could not finish (serial walk + RLE1 undo); false: nothing to do
SWC_D bool bzip2_expand(Job* __restrict__ jobs, uint32_t g, uint8_t* ws, size_t lcap) {
    const bzip2::Workspace w = bzip2::carve(ws, g, lcap);
    if (!bzip2::stage3_expand_needed(w)) return false;
    Job job = jobs[g];
    bzip2::stage3_expand_job(job, w);
    put_result<true>(jobs, g, job);
    return true;
}

// ---- swc_crc32_kernel behind its copy of the constants into LDS: one stream per wave, the streams below kCrcGroupLen ------------
SWC_D void crc32_wave(const Job* __restrict__ jobs, uint32_t g, uint32_t* __restrict__ crcs, const crcw::WaveConsts* consts, int lane) {
    const uint64_t len = made_bytes(jobs[g].out_len, jobs[g].out_cap);
    if (len >= kCrcGroupLen) return;
    const uint32_t c = crcw::crc32_wave((gcptr)jobs[g].out, simt::uniform(len), consts);
    if (lane == 0) crcs[g] = c;
}

// ---- swc_sha256_kernel: one job per LANE.  digests + 32 g: the SHA-256 of what exists of job g's output, whatever its status, in
// the standard's byte order; `digests` at any alignment
SWC_D void sha256_lane(const Job* __restrict__ jobs, uint32_t g, uint8_t* __restrict__ digests) {
    uint32_t h[8];
    sha::sha256_lane((gcptr)jobs[g].out, made_bytes(jobs[g].out_len, jobs[g].out_cap), h);
    gptr d = (gptr)digests + 32 * (size_t)g;
    store_u128_a4(d, sha::be32(h[0]), sha::be32(h[1]), sha::be32(h[2]), sha::be32(h[3]));
    store_u128_a4(d + 16, sha::be32(h[4]), sha::be32(h[5]), sha::be32(h[6]), sha::be32(h[7]));
}

}  // namespace jobk
}  // namespace swc
#endif
