// emu.cpp -- TEST INFRASTRUCTURE.  Builds the device decoders of swcompression_amd/csrc for the HOST
// (g++ -DSWC_HOST_EMULATION): the uniform parts run once, the threads of every SIMT region (csrc/simt.h) one
// after another in a selectable order.  Lets the CPU-only test tier exercise
// the exact source the gfx950 kernels are compiled from against the oracle.  Never shipped, never
// linked into libswc_hip.so.  A driver that emulates a launch calls the kernel bodies of csrc/job_kernels.h -- what the __global__
// functions call -- in the order the launcher issues the kernels; the other entry points test one header function alone.  This
// file is the whole library: the drivers that have a source of their own (emu_bgzf.cpp, emu_crc_tail.cpp, emu_lz4_linked.cpp --
// every LZ4 decode launch --, emu_deflate_units.cpp -- every Deflate decode launch --, emu_deflate_linked.cpp, emu_sha256.cpp and
// the probes of emu_deflate_phase1.cpp) are included at its end, so that one compile shares the template instantiations.  A
// differential variant is this file under one more -D (tests/_emu.py: VARIANTS).
#include <algorithm>
#include <memory>
#include "emu_util.h"
#include "../../swcompression_amd/csrc/huffman_wave.h"
#include "../../swcompression_amd/csrc/bzip2_comp.h"

// phase 2 alone on a workspace area a test has laid out (emu_copy_records*): lz_copy.h in either window
template <typename CFG, int RM = 0>
static void emu_copy(swc::Job& job, const uint8_t* ws, size_t wsb) {
    swc::lzc::copy_job<CFG, RM>(job, ws, wsb, emu_lds<swc::lzc::Lds<CFG::kWin>>());
}

extern "C" void emu_lz4_stats(uint64_t* out, int reset) {
    for (int i = 0; i < 8; i++) { out[i] = swc::lz4w::g_lz4_stats[i]; if (reset) swc::lz4w::g_lz4_stats[i] = 0; }
}
extern "C" void emu_sync_wave(uint64_t* out) { for (int i = 0; i < 4; i++) { out[i] = swc::inflate::g_sync_wave[i]; swc::inflate::g_sync_wave[i] = 0; } }
extern "C" void emu_sync_stats(uint64_t* out, int reset) {
    for (int i = 0; i < 8; i++) { out[i] = swc::inflate::g_sync_stats[i]; if (reset) swc::inflate::g_sync_stats[i] = 0; }
}

// The chain check of a sub-chunk round on its own (sync_round.h): 64 lanes' starts, ends, `have` and flags in, out = {b, E, nv}
extern "C" void emu_chain_check(const uint32_t* start, const uint32_t* endp, const uint8_t* have, const uint32_t* flg, uint32_t first,
                                uint32_t stop_bits, uint32_t* out) {
    constexpr int N = swc::kWave;
    swc::simt::PT<uint32_t, N> s, e, f, pe;
    swc::simt::PT<bool, N> h;
    for (int t = 0; t < N; t++) { s[t] = start[t]; e[t] = endp[t]; f[t] = flg[t]; h[t] = have[t] != 0; pe[t] = 0xDEADBEEFu; }
    const swc::sround::Chain c = swc::sround::chain_check<N>(pe, s, e, h, f, first, stop_bits);
    out[0] = (uint32_t)c.b; out[1] = (uint32_t)c.E; out[2] = c.nv;
}

// LZ4 block compression (lz4_comp.h): job.in = prefix ++ block, job.dict_len = length of the prefix
extern "C" void emu_lz4_compress(swc::Job* jobs, size_t n) {
    for (size_t g = 0; g < n; g++) swc::jobk::lz4_compress<64>(jobs, (uint32_t)g, emu_lds<std::array<uint16_t, swc::lz4c::kHashSize>>()->data(), 0);
}

// Deflate compression (deflate_comp.h): job.in = the buffer
extern "C" void emu_deflate_compress(swc::Job* jobs, size_t n) {
    for (size_t g = 0; g < n; g++) swc::jobk::deflate_compress<64>(jobs, (uint32_t)g, emu_lds<swc::defc::Lds>(), 0);
}

// Deflate compression with dynamic blocks: job.in = the buffer, job.aux bit 0 = a segment of a longer stream
extern "C" void emu_deflate_compress_dynamic(swc::Job* jobs, size_t n) {
    for (size_t g = 0; g < n; g++) swc::jobk::deflate_compress_dynamic<64>(jobs, (uint32_t)g, emu_lds<swc::defc::DynLds>(), 0);
}

// the shared builder on its own: weights w[0 .. alpha) (alpha <= 288) -> code lengths and canonical codes (MSB first)
extern "C" void emu_huffman(const uint32_t* w, uint32_t alpha, uint32_t max_len, uint32_t* len, uint32_t* code) {
    alignas(16) static swc::huff::HuffLds<swc::defc::kHuffCap> l;
    std::memset(&l, 0xEE, sizeof l);
    for (uint32_t s = 0; s < alpha; s++) l.w[s] = w[s];
    swc::huff::huffman_wave<64>(&l, alpha, max_len);
    for (uint32_t s = 0; s < alpha; s++) { len[s] = l.len[s]; code[s] = l.wt[s] & 0xFFFFFFu; }
}

// LZMA: the wave-uniform decode chain is run as a single logical lane (WAVE = 1); the literal-coder
// spill (lc+lp > 4) is always available, as the single-shot C ABI guarantees on the device.
// mode 0: every literal coder in LDS up to lc + lp = 4, larger models cell by cell from the spill (the kernel without a
// workspace, and the old spill path); mode 1: LDS as a cache of kCoderSlots literal coders, long-length trees in the spill (the kernel with a workspace).
// TEST-ONLY choices of the kernel's template arguments: mode 0 is swc_lzma_kernel<LZMA2, 4> WITH a spill buffer, which launch_lzma
// hands that instantiation never (it gets nullptr), and <LZMA2, 3> -- launch_lzma's choice with a workspace and the cache off -- is not run here.
template <bool LZMA2, int LDSBITS>
static void emu_lzma_launch(swc::Job* jobs, size_t n) {
    std::vector<uint16_t> probs(swc::lzma::kProbCells + 8);
    std::vector<uint16_t> spill(swc::kLzmaSpillBytes / 2);
    for (size_t g = 0; g < n; g++) {
        std::fill(probs.begin(), probs.end(), (uint16_t)0xBEEF);
        std::fill(spill.begin(), spill.end(), (uint16_t)0xDEAD);
        swc::jobk::lzma_stream<1, LZMA2, LDSBITS>(jobs + g, 0, (uint8_t*)spill.data(), probs.data(), 0, nullptr);
    }
}
extern "C" void emu_lzma_mode(swc::Job* jobs, size_t n, int is_lzma2, int mode) {
    static_assert(swc::lzma::kMaxLdsLitBits == 4, "mode 0 is swc_lzma_kernel<LZMA2, 4>");
    if (mode == 1) is_lzma2 ? emu_lzma_launch<true, -1>(jobs, n) : emu_lzma_launch<false, -1>(jobs, n);
    else is_lzma2 ? emu_lzma_launch<true, 4>(jobs, n) : emu_lzma_launch<false, 4>(jobs, n);
}
extern "C" void emu_lzma(swc::Job* jobs, size_t n, int is_lzma2) { emu_lzma_mode(jobs, n, is_lzma2, 0); }

// stage 3c (swc_bzip2_crc_kernel keeps its body in kernels.hip: restated here)
static void emu_bzip2_crc(swc::Job& job) {
    static swc::crc::Lds<1, uint32_t> crc_lds;
    if (job.status == SWC_OK) swc::bzip2::stage3_check_crc(job, swc::crc::crc_group<1, uint32_t, true>(job.out, job.out_len, &crc_lds, 0));
}
using BzLds = std::array<uint8_t, swc::kBzLdsBytes>;

// BZip2 as launch_bzip2 issues it without the team walk: block kernel | expand | CRC, job by job in one workspace.
static uint64_t g_fused_finished = 0;   // blocks whose output came from stage 3a inside the block kernel, not from the serial fallback
extern "C" uint64_t emu_bzip2_fused_finished(int reset) { const uint64_t v = g_fused_finished; if (reset) g_fused_finished = 0; return v; }
extern "C" void emu_bzip2_block(swc::Job* jobs, size_t n, size_t lcap) {
    std::vector<uint8_t> ws(swc::bzip2::ws_bytes_per_job(lcap) + 64);
    for (size_t g = 0; g < n; g++) {
        std::fill(ws.begin(), ws.end(), (uint8_t)0xCD);
        swc::jobk::bzip2_block<1, false>(jobs + g, 0, ws.data(), lcap, emu_lds<BzLds>()->data(), 0, 0);
        if (!swc::jobk::bzip2_expand(jobs + g, 0, ws.data(), lcap)) g_fused_finished++;
        emu_bzip2_crc(jobs[g]);
    }
}

// BZip2 with stage 3a as kernels of its own (bzip2_team.h): stage 1 + 2 of ALL jobs, then the segment counts and their prefixes
// per team, the walk (every team's tickets drawn by one thread; `start_team`: the team whose thread goes first and, with the
// work stealing, through the others' tickets too when `one_thread` is set), the finish per job, the serial fallback, the CRC.
// The workspace geometry of stage 3 for a block of n bytes inside a workspace cut for lcap: what the two walks need against what
// the layout gives them (tests/test_lane_emulation_bzip2.py walks through many (lcap, n) pairs).
extern "C" void emu_bzip2_layout(size_t lcap, uint32_t n, uint64_t* out) {
    using namespace swc::bzip2;
    Cut c;
    c.set(n, n / 3u + 1u < n ? n / 3u + 1u : 0u);                       // an origin pointer off the marks where there is room
    const uint32_t m = seg_mbits(n), regs = (n + (1u << m) - 1u) >> m;
    out[0] = team_seg_slots(lcap);                                      // slots of the per-segment arrays
    out[1] = c.segs;                                                    // segments the team walk cuts the block into
    out[2] = segbuf_bytes(lcap);                                        // bytes of segment buffers
    out[3] = (uint64_t)(c.regs + 1u) * c.cap;                           // ... the team walk needs
    out[4] = (uint64_t)(regs + 1u) * ((uint64_t)kSegCapFactor << m);    // ... the walk inside the block's wavefront needs
    out[5] = seg_info_bytes(lcap);
    out[6] = (2ull * (kSegs + 1) > 4ull * out[0] ? 2ull * (kSegs + 1) : 4ull * out[0]) * 4 + kTeamWords * 4;   // ... and what must fit in it
    out[7] = ws_bytes_per_job(lcap);
}
static uint64_t g_team_finished = 0;   // blocks whose output came from team_finish, not from the serial fallback
extern "C" uint64_t emu_bzip2_team_finished(int reset) { const uint64_t v = g_team_finished; if (reset) g_team_finished = 0; return v; }
extern "C" void emu_bzip2_block_team(swc::Job* all_jobs, size_t n_all, size_t lcap, int start_team, int one_thread) {
    using namespace swc::bzip2;
    const size_t per = ws_bytes_per_job(lcap), kAtOnce = 24;          // (the workspaces of a launch exist side by side: 24 jobs at a time)
    std::vector<uint8_t> ws(per * std::min(n_all, kAtOnce) + 64);
    for (size_t j0 = 0; j0 < n_all; j0 += kAtOnce) {
        swc::Job* jobs = all_jobs + j0;
        const size_t n = std::min(kAtOnce, n_all - j0);
        std::fill(ws.begin(), ws.end(), (uint8_t)0xCD);
        for (uint32_t g = 0; g < n; g++) swc::jobk::bzip2_block<1, false>(jobs, g, ws.data(), lcap, emu_lds<BzLds>()->data(), 0, 1);
        for (uint32_t t = 0; t < kTeams; t++) team_prep<1>(ws.data(), lcap, (uint32_t)n, t, 0);
        for (uint32_t d = 0; d < (one_thread ? 1u : kTeams); d++) team_walk(ws.data(), lcap, (uint32_t)n, ((uint32_t)start_team + d) % kTeams);
        for (uint32_t g = 0; g < n; g++) swc::jobk::bzip2_team_finish<1>(jobs, g, ws.data(), lcap, emu_lds<FinishLds>(), 0);
        for (uint32_t g = 0; g < n; g++) if (!swc::jobk::bzip2_expand(jobs, g, ws.data(), lcap)) g_team_finished++;
        for (uint32_t g = 0; g < n; g++) emu_bzip2_crc(jobs[g]);
    }
}

// Phase 2 alone (tests/test_lz_copy_records.py): a record list and a literal stream made by the test, laid out as phase 1 lays
// them out in a workspace area, through lz_copy.h (copier != 0) or lz_resolve.h; `out` may sit at any alignment.
extern "C" void emu_copy_records(const uint32_t* recs, uint32_t nrec, const uint8_t* lits, size_t nlit, uint8_t* out, size_t cap, size_t out_len, int copier) {
    const size_t wsb = swc::lzr::ws_bytes_per_job(cap);
    std::vector<uint8_t> ws(wsb + 16, (uint8_t)0xCD);
    swc::lzr::StreamHeader* h = (swc::lzr::StreamHeader*)ws.data();
    h->nrec = nrec;
    h->nlit = nlit;
    std::memcpy(ws.data() + sizeof(swc::lzr::StreamHeader), recs, 4 * (size_t)nrec);
    std::memcpy(ws.data() + swc::lzr::lit_offset(wsb, cap), lits, nlit);
    swc::Job j{};
    j.out = out; j.out_cap = cap; j.out_len = out_len;
    if (copier == 3) emu_copy<swc::lzc::CfgDeflate>(j, ws.data(), wsb);
    else if (copier) emu_copy<swc::lzc::CfgLz4>(j, ws.data(), wsb);
    else {
        using namespace swc;   // (FAR: `out` may sit anywhere, so every source is read back from it)
        lzr::resolve_job<kInflateResolveThreads, kInflateRingLog2, kInflateKeep, true>(j, ws.data(), wsb, emu_lds<lzr::Lds<kInflateResolveThreads, kInflateRingLog2>>());
    }
}

// The same with EIGHT-byte records (record | literal offset << 32) whose literals lie in `in` (the LZ4 path): `in` is copied
// into a buffer of exactly in_len bytes, so that a read past the block shows under AddressSanitizer.
extern "C" void emu_copy_records8(const uint32_t* recs2, uint32_t nrec, const uint8_t* in, size_t in_len, uint8_t* out, size_t cap, size_t out_len, int copier) {
    const size_t wsb = swc::lzr::ws_bytes_per_job(cap);
    std::vector<uint8_t> ws(wsb + 16, (uint8_t)0xCD);
    swc::lzr::StreamHeader* h = (swc::lzr::StreamHeader*)ws.data();
    h->nrec = nrec;
    h->nlit = 0;
    std::memcpy(ws.data() + sizeof(swc::lzr::StreamHeader), recs2, 8 * (size_t)nrec);
    std::unique_ptr<uint8_t[]> exact(new uint8_t[in_len ? in_len : 1]);
    std::memcpy(exact.get(), in, in_len);
    swc::Job j{};
    j.in = exact.get(); j.in_len = in_len;
    j.out = out; j.out_cap = cap; j.out_len = out_len;
    if (copier == 3) emu_copy<swc::lzc::CfgDeflate, 1>(j, ws.data(), wsb);
    else emu_copy<swc::lzc::CfgLz4, 1>(j, ws.data(), wsb);
}
// ... and with FOUR-byte records whose literal offsets are derived (lz_copy.h RM == 2): `anchors` = nanc (record index, S) pairs
extern "C" void emu_copy_records4(const uint32_t* recs, uint32_t nrec, const uint32_t* anchors, uint32_t nanc, const uint8_t* in, size_t in_len,
                                  uint8_t* out, size_t cap, size_t out_len, int copier) {
    const size_t wsb = swc::lzr::ws_bytes_per_job(cap);
    std::vector<uint8_t> ws(wsb + 16, (uint8_t)0xCD);
    swc::lzr::StreamHeader* h = (swc::lzr::StreamHeader*)ws.data();
    h->nrec = nrec;
    h->pad0 = nanc;
    h->nlit = 0;
    std::memcpy(ws.data() + sizeof(swc::lzr::StreamHeader), recs, 4 * (size_t)nrec);
    std::memcpy(ws.data() + swc::lzr::lit_offset(wsb, cap), anchors, 8 * (size_t)nanc);
    std::unique_ptr<uint8_t[]> exact(new uint8_t[in_len ? in_len : 1]);
    std::memcpy(exact.get(), in, in_len);
    swc::Job j{};
    j.in = exact.get(); j.in_len = in_len;
    j.out = out; j.out_cap = cap; j.out_len = out_len;
    if (copier == 3) emu_copy<swc::lzc::CfgDeflate, 2>(j, ws.data(), wsb);
    else emu_copy<swc::lzc::CfgLz4, 2>(j, ws.data(), wsb);
}

// The LZ4 parse alone in the derived-offset form (record mode 2): how many records and how many anchors a block needs
extern "C" void emu_lz4_parse_counts(const uint8_t* in, size_t in_len, size_t cap, uint32_t* nrec, uint32_t* nanc) {
    size_t wsb = swc::lzr::ws_bytes_per_job(cap);
    std::vector<uint8_t> ws(wsb + 16, (uint8_t)0xCD), out(cap + 16);
    alignas(16) static uint8_t stage[swc::lz4w::kStageLds];
    swc::Job j{};
    j.in = in; j.in_len = in_len; j.out = out.data(); j.out_cap = cap;
    swc::lz4w::lz4_parse_job<1, 2>(j, ws.data(), wsb, 0, stage);
    const swc::lzr::StreamHeader* h = (const swc::lzr::StreamHeader*)ws.data();
    *nrec = h->nrec;
    *nanc = h->pad0;
}

// Debug/analysis helper (tools/analyze_records.py): phase 1 only, returns the record list of one stream.
extern "C" size_t emu_inflate_records(const uint8_t* in, size_t in_len, uint8_t* out, size_t cap, uint32_t* recs_out, size_t max_out) {
    alignas(16) static swc::inflate::SyncLds sl;
    size_t wsb = swc::lzr::ws_bytes_per_job(cap);
    std::vector<uint8_t> ws(wsb + 16, (uint8_t)0xCD);
    swc::Job j{};
    j.in = in; j.in_len = in_len; j.out = out; j.out_cap = cap;
    swc::inflate::inflate_sync_job(j, &sl, ws.data(), wsb, 0, 1);
    uint32_t n = ((swc::lzr::StreamHeader*)ws.data())->nrec;
    const uint32_t* r = (const uint32_t*)(ws.data() + sizeof(swc::lzr::StreamHeader));
    for (size_t i = 0; i < n && i < max_out; i++) recs_out[i] = r[i];
    return n;
}

// The same for an LZ4 block (tools/analyze_records.py lz4)
extern "C" size_t emu_lz4_records(const uint8_t* in, size_t in_len, uint8_t* out, size_t cap, uint32_t* recs_out, size_t max_out) {
    size_t wsb = swc::lzr::ws_bytes_per_job(cap);
    std::vector<uint8_t> ws(wsb + 16, (uint8_t)0xCD);
    alignas(16) static uint8_t stage[swc::lz4w::kStageLds];
    swc::Job j{};
    j.in = in; j.in_len = in_len; j.out = out; j.out_cap = cap;
    swc::lz4w::lz4_parse_job<1>(j, ws.data(), wsb, 0, stage);
    uint32_t n = ((swc::lzr::StreamHeader*)ws.data())->nrec;
    const uint32_t* r = (const uint32_t*)(ws.data() + sizeof(swc::lzr::StreamHeader));
    for (size_t i = 0; i < n && i < max_out; i++) recs_out[i] = r[i];
    return n;
}

// ---- checksums: the group kernels run with T real host threads and a pthread barrier behind swc::group_sync ----------
#include <thread>
#include <pthread.h>
#include "../../swcompression_amd/csrc/checksum_group.h"

namespace {
pthread_barrier_t* g_barrier;
void barrier_wait() { pthread_barrier_wait(g_barrier); }

template <int T, typename F>
uint64_t run_group(F body) {
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, T);
    g_barrier = &bar;
    uint64_t result = 0;
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++)
        th.emplace_back([&, t] {
            swc::emu_group_sync = barrier_wait;
            uint64_t r = body(t);
            if (t == 0) result = r;
        });
    for (auto& x : th) x.join();
    pthread_barrier_destroy(&bar);
    return result;
}
}  // namespace

// the wave-per-stream CRC-32 (crc32_wave.h): constants built once, the 64 lanes run one after the other
extern "C" uint32_t emu_crc32_wave(const uint8_t* p, size_t n) { return swc::crcw::crc32_wave(p, n, emu_wave_consts()); }

// kind as swc_checksum (include/swc_hip.h); T = 64 emulated threads per group
extern "C" uint64_t emu_checksum(int kind, const uint8_t* p, size_t n) {
    using namespace swc;
    constexpr int T = 64;
    switch (kind) {
        case 1: { static crc::Lds<T, uint32_t> l; return run_group<T>([&](int t) { return (uint64_t)crc::crc_group<T, uint32_t, false>(p, n, &l, t); }); }
        case 2: { static sums::AdlerLds<T> l; return run_group<T>([&](int t) { return (uint64_t)sums::adler32_group<T>(p, n, &l, t); }); }
        case 3: { static crc::Lds<T, uint64_t> l; return run_group<T>([&](int t) { return (uint64_t)crc::crc_group<T, uint64_t, false>(p, n, &l, t); }); }
        case 4: { static crc::Lds<T, uint32_t> l; return run_group<T>([&](int t) { return (uint64_t)crc::crc_group<T, uint32_t, true>(p, n, &l, t); }); }
        case 5: {
            uint32_t acc[4];
            const uint32_t seed = 0;
            for (int j = 0; j < 4; j++) {
                const uint32_t init = j == 0 ? seed + sums::kP1 + sums::kP2 : j == 1 ? seed + sums::kP2 : j == 2 ? seed : seed - sums::kP1;
                acc[j] = sums::xxh32_lane(p, n / 16, j, init);
            }
            return sums::xxh32_quad(p, n, seed, 0, [&](uint32_t, int k) { return acc[k]; });
        }
    }
    return 0;
}

// Delta filter: the group kernel with T real host threads (same barrier plumbing as the checksums; swc_delta_kernel keeps its body
// in kernels.hip)
#include "../../swcompression_amd/csrc/delta_group.h"
extern "C" void emu_delta(const uint8_t* in, uint8_t* out, size_t n, unsigned distance) {
    constexpr int T = 256;
    static swc::delta::Lds<T> l;
    run_group<T>([&](int t) { swc::delta::delta_group<T>(in, out, n, distance, &l, t); return (uint64_t)0; });
}

// BZip2 compression (bzip2_comp.h): the executor of the emulation -- "device memory" is host memory, a kernel is a loop over
// its elements / blocks, std::sort and two serial scans stand in for the three rocPRIM calls of the device executor.
namespace {
struct EmuBz2Exec {
    std::vector<std::unique_ptr<uint8_t[]>> mem;
    void begin_chunk() {}
    void mark(const char*) {}
    uint8_t* result_alloc(size_t n) { uint8_t* q = (uint8_t*)malloc(n ? n : 1); if (q) std::memset(q, 0xEE, n); return q; }
    void result_free(uint8_t* q) { free(q); }
    void note(const char*, uint32_t, uint32_t) {}
    void end_chunk() { mem.clear(); }
    void* alloc(size_t n) { mem.emplace_back(new uint8_t[n ? n : 1]); std::memset(mem.back().get(), 0xEE, n); return mem.back().get(); }   // exact: the ASAN build sees every overrun
    void upload(void* d, const void* h, size_t n) { std::memcpy(d, h, n); }
    void download(void* h, const void* d, size_t n) { std::memcpy(h, d, n); }
    void zero(void* d, size_t n) { std::memset(d, 0, n); }
    template <class F> void each(uint32_t m, const F& f) {
        if (swc::simt::g_order == 1) for (uint32_t i = m; i-- > 0;) f(i);
        else for (uint32_t i = 0; i < m; i++) f(i);
    }
    template <class F> void per_block(uint32_t nb, const F& f) {
        for (uint32_t b = 0; b < nb; b++) {
            alignas(16) static typename F::Lds lds;
            std::memset(&lds, 0xEE, sizeof lds);
            f.template run<64>(b, &lds);
        }
    }
    int sort_pairs(uint64_t* kin, uint64_t* kout, uint32_t* vin, uint32_t* vout, uint32_t m, int bits) {
        const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1ull;
        std::vector<uint32_t> idx(m);
        for (uint32_t i = 0; i < m; i++) { idx[i] = i; if (kin[i] & ~mask) return 1; }   // a key wider than announced: the radix sort would drop bits
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return kin[a] < kin[b]; });
        for (uint32_t i = 0; i < m; i++) { kout[i] = kin[idx[i]]; vout[i] = vin[idx[i]]; }
        return 0;
    }
    int scan_max(uint32_t* x, uint32_t m) { uint32_t a = 0; for (uint32_t i = 0; i < m; i++) { a = x[i] > a ? x[i] : a; x[i] = a; } return 0; }
    int scan_sum(const uint32_t* in, uint32_t* out, uint32_t m) { uint32_t a = 0; for (uint32_t i = 0; i < m; i++) { out[i] = a; a += in[i]; } return 0; }
    int block_crcs(const uint8_t* raw, const uint32_t* off, uint32_t nb, uint32_t* crcs) {
        for (uint32_t b = 0; b < nb; b++) {   // CheckSums.bzip2crc32: polynomial 0x04C11DB7, MSB first
            uint32_t c = 0xFFFFFFFFu;
            for (uint32_t i = off[b]; i < off[b + 1]; i++) {
                c ^= (uint32_t)raw[i] << 24;
                for (int k = 0; k < 8; k++) c = (c & 0x80000000u) ? (c << 1) ^ 0x04C11DB7u : c << 1;
            }
            crcs[b] = ~c;
        }
        return 0;
    }
};
}  // namespace
// returns the status; *out_len = bytes needed (the stream is copied only if it fits `cap`)
extern "C" int emu_bzip2_compress(const uint8_t* data, size_t len, int level, uint8_t* out, size_t cap, size_t* out_len) {
    EmuBz2Exec x;
    uint8_t* res = nullptr;
    size_t n = 0;
    const int st = swc::bz2c::compress_stream(x, data, len, level, &res, &n);
    *out_len = n;
    if (st == 0 && n <= cap) std::memcpy(out, res, n);
    free(res);
    return st;
}

// ---- the drivers that have a source of their own (four of them double as stand-alone sanitizer programs) ---------------------
#include "emu_bgzf.cpp"
#include "emu_crc_tail.cpp"
#include "emu_lz4_linked.cpp"
#include "emu_deflate_units.cpp"
#include "emu_deflate_linked.cpp"
#include "emu_sha256.cpp"
#include "emu_deflate_phase1.cpp"
