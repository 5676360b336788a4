// emu_lz4_linked.cpp -- TEST INFRASTRUCTURE.  The LZ4 path for jobs with history -- the parse with history (csrc/lz4_wave.h), the
// copier with history (csrc/lz_copy.h) and the chain walk (csrc/lz4_chain.h) -- compiled for the HOST (g++ -DSWC_HOST_EMULATION):
// the three steps of a launch one after the other, as kernels.hip issues them.  Part of libswc_emu.so (emu.cpp includes it).  Never
// shipped.
//
// With -DEMU_LZ4_LINKED_MAIN the file is a stand-alone program (for -fsanitize=address,undefined): it reads chains and what the
// oracle says about them from a file written by tests/test_lz4_linked_emulation.py, runs every chain at the sixteen alignments
// of its buffer in the three lane orders, in allocations of exactly the size the contract asks for, and compares.
#include "emu_util.h"
#include "../../swcompression_amd/csrc/lz4_lane.h"
#include "../../swcompression_amd/csrc/lz4_chain.h"

namespace {
struct Areas {
    std::vector<std::vector<uint8_t>> a;
    uint8_t* area(uint32_t g) const { return const_cast<uint8_t*>(a[g].data()); }
    size_t bytes(uint32_t g) const { return a[g].size() - 16; }
};
}  // namespace

// One launch of SWC_CODEC_LZ4_BLOCK with a workspace: lane decoder | parse | chain copy, each over all jobs.
extern "C" void emu_lz4_linked(swc::Job* jobs, size_t n) {
    using namespace swc;
    alignas(16) static uint8_t stage[lz4w::kStageLds];
    alignas(16) static lzc::Lds<lzc::CfgLz4::kWin> lds;
    Areas ws;
    ws.a.resize(n);
    for (size_t g = 0; g < n; g++) ws.a[g].assign(lzr::ws_bytes_per_job(jobs[g].out_cap) + 16, (uint8_t)0xCD);
    for (size_t g = 0; g < n; g++)
        if (lz4w::lane_job(jobs[g])) lz4::lz4_block_job(jobs[g]);
    for (size_t g = 0; g < n; g++) {
        if (lz4w::lane_job(jobs[g])) continue;
        Job job = jobs[g];
        uint64_t hist = 0;
        if (!lz4w::parse_preset(job, hist)) {
            std::memset(stage, 0xEE, sizeof stage);
            lz4w::lz4_parse_job<1, 2>(job, ws.area((uint32_t)g), ws.bytes((uint32_t)g), 0, stage, nullptr, hist);
        }
        put_result(jobs, (uint32_t)g, job);
    }
    for (size_t g = 0; g < n; g++) {
        std::memset(&lds, 0xEE, sizeof lds);
        lz4w::copy_chain<lzc::CfgLz4, 2>(jobs, (uint32_t)g, (uint32_t)n, ws, &lds);
    }
}

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
        for (int order = 0; order < 3; order++) {
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
                emu_lz4_linked(jobs.data(), jobs.size());
                bool ok = true;
                for (size_t i = 0; i < js.size(); i++) ok = ok && jobs[i].status == js[i].status && jobs[i].out_len == js[i].out_len;
                ok = ok && memcmp(raw + mis + prefix.size(), want.data(), want.size()) == 0;
                for (size_t i = 0; i < mis; i++) ok = ok && raw[i] == 0xA5;
                ok = ok && (prefix.empty() || memcmp(raw + mis, prefix.data(), prefix.size()) == 0);
                for (size_t i = mis + prefix.size() + want.size(); i < total; i++) ok = ok && raw[i] == 0xA5;   // nothing behind what the chain produced
                if (!ok) { fprintf(stderr, "case %u order %d misalignment %zu: mismatch\n", c, order, mis); bad++; }
                free(raw);
            }
        }
    }
    printf("%u cases, %d mismatches\n", ncases, bad);
    return bad ? 1 : 0;
}
#endif
