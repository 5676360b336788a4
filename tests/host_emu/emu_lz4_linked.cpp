// emu_lz4_linked.cpp -- TEST INFRASTRUCTURE.  A launch of LZ4 blocks with a workspace -- the lane decoder, the parse with and without
// history, the byte-cell resolver, the chain copy -- compiled for the HOST (g++ -DSWC_HOST_EMULATION): the kernel bodies of
// csrc/job_kernels.h in the order launch_lz4 issues the kernels, each over all jobs.  Part of libswc_emu.so (emu.cpp includes it).
// Never shipped.
//
// With -DEMU_LZ4_LINKED_MAIN the file is a stand-alone program (for -fsanitize=address,undefined): it reads chains and what the
// oracle says about them from a file written by tests/test_lz4_linked_emulation.py, runs every chain at the sixteen alignments
// of its buffer in the three lane orders with both copier choices, in allocations of exactly the size the contract asks for, and
// compares.
#include "emu_util.h"

// copier != 0: a launch of kCopierMin jobs and more -- one record-mode parse, the chain copier over all jobs; 0: a smaller one --
// the jobs without history through the plain parse and the byte-cell resolver, the others as above.  CFG, RM: test-only.
template <typename CFG, int RM>
static void emu_lz4_launch(swc::Job* jobs, uint32_t n, int copier) {
    using namespace swc;
    using Stage = std::array<uint8_t, lz4w::kStageLds>;
    std::vector<std::vector<uint8_t>> areas(n);
    for (uint32_t g = 0; g < n; g++) emu_ws_give(areas[g], jobs[g].out_cap);
    const EmuWs ws{areas.data(), 0};
    for (uint32_t g = 0; g < n; g++) jobk::lz4_lane(jobs, g, 1);
    if (copier) {
        for (uint32_t g = 0; g < n; g++) jobk::lz4_parse<1, RM>(jobs, g, n, ws, emu_lds<Stage>()->data(), 0, nullptr, 0);
    } else {
        for (uint32_t g = 0; g < n; g++) jobk::lz4_parse<1, 0>(jobs, g, n, ws, emu_lds<Stage>()->data(), 0, nullptr, 2);
        for (uint32_t g = 0; g < n; g++) jobk::lz4_parse<1, RM>(jobs, g, n, ws, emu_lds<Stage>()->data(), 0, nullptr, 1);
        for (uint32_t g = 0; g < n; g++) jobk::lz4_resolve(jobs, g, n, ws, emu_lds<lzr::Lds<lz4w::kResolveThreads, lz4w::kRingLog2>>(), nullptr);
    }
    for (uint32_t g = 0; g < n; g++) jobk::lz4_copy<EmuWs, CFG, RM>(jobs, g, n, ws, emu_lds<lzc::Lds<CFG::kWin>>(), copier ? 0 : 1);
}

// One launch of SWC_CODEC_LZ4_BLOCK with a workspace; copier: the launch's choice (kernels.hip: wave_copier).
extern "C" void emu_lz4_linked(swc::Job* jobs, size_t n, int copier) {
    using namespace swc;
    const uint32_t m = (uint32_t)n;
    if (g_lz4_mode == 1) g_copier == 3 ? emu_lz4_launch<lzc::CfgDeflate, 1>(jobs, m, copier) : emu_lz4_launch<lzc::CfgLz4, 1>(jobs, m, copier);
    else g_copier == 3 ? emu_lz4_launch<lzc::CfgDeflate, 2>(jobs, m, copier) : emu_lz4_launch<lzc::CfgLz4, 2>(jobs, m, copier);
}
// ... with the copier choice of emu_set_copier (tests/_emu.py: lz4_block)
extern "C" void emu_lz4_block(swc::Job* jobs, size_t n) { emu_lz4_linked(jobs, n, g_copier != 0); }

#ifdef EMU_LZ4_LINKED_MAIN
namespace {
struct JobSpec { int32_t aux; std::vector<uint8_t> in; uint32_t cap; int32_t status; uint32_t out_len; };
}  // namespace

// File: u32 cases; per case: u32 prefix length + bytes (the head's adjacent prefix), u32 jobs, per job i32 aux, u32 length + block,
// u32 capacity, i32 expected status, u32 expected out_len; then u32 length + the bytes the chain must leave behind the prefix.
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    Reader r(argv[1]);
    const uint32_t ncases = r.u32();
    int bad = 0;
    for (uint32_t c = 0; c < ncases; c++) {
        const std::vector<uint8_t> prefix = r.bytes(r.u32());
        std::vector<JobSpec> js(r.u32());
        size_t room = 0;
        for (auto& j : js) { j.aux = (int32_t)r.u32(); j.in = r.bytes(r.u32()); j.cap = r.u32(); j.status = (int32_t)r.u32(); j.out_len = r.u32(); room += j.cap; }
        const std::vector<uint8_t> want = r.bytes(r.u32());
        for (int mode = 0; mode < 6; mode++) {
            const int order = mode % 3, copier = mode < 3;
            for (size_t mis = 0; mis < 16; mis++) {
                emu_set_order(order);
                // exactly the bytes the contract names: the sanitizer sees every access beyond them
                uint8_t* raw = (uint8_t*)aligned_alloc(16, (mis + prefix.size() + room + 15) / 16 * 16 + 16);
                const size_t total = mis + prefix.size() + room;
                memset(raw, 0xA5, (total + 15) / 16 * 16 + 16);
                if (!prefix.empty()) memcpy(raw + mis, prefix.data(), prefix.size());
                std::vector<std::vector<uint8_t>> ins;
                for (auto& j : js) { ins.emplace_back(j.in.size() ? j.in.size() : 1); if (!j.in.empty()) memcpy(ins.back().data(), j.in.data(), j.in.size()); }
                std::vector<swc::Job> jobs(js.size());
                for (size_t i = 0; i < js.size(); i++) {
                    memset(&jobs[i], 0, sizeof(swc::Job));
                    jobs[i].in = ins[i].data();
                    jobs[i].in_len = js[i].in.size();
                    jobs[i].out_cap = js[i].cap;
                    jobs[i].aux = js[i].aux;
                    jobs[i].status = 902;
                }
                jobs[0].out = raw + mis + prefix.size();
                if (!prefix.empty()) { jobs[0].dict = raw + mis; jobs[0].dict_len = prefix.size(); }
                emu_lz4_linked(jobs.data(), jobs.size(), copier);
                bool ok = true;
                for (size_t i = 0; i < js.size(); i++) ok = ok && jobs[i].status == js[i].status && jobs[i].out_len == js[i].out_len;
                ok = ok && memcmp(raw + mis + prefix.size(), want.data(), want.size()) == 0;
                for (size_t i = 0; i < mis; i++) ok = ok && raw[i] == 0xA5;
                ok = ok && (prefix.empty() || memcmp(raw + mis, prefix.data(), prefix.size()) == 0);
                for (size_t i = mis + prefix.size() + want.size(); i < total; i++) ok = ok && raw[i] == 0xA5;   // nothing behind what the chain produced
                if (!ok) { fprintf(stderr, "case %u order %d copier %d misalignment %zu: mismatch\n", c, order, copier, mis); bad++; }
                free(raw);
            }
        }
    }
    printf("%u cases, %d mismatches\n", ncases, bad);
    return bad ? 1 : 0;
}
#endif
