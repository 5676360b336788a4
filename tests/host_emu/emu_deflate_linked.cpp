// emu_deflate_linked.cpp -- TEST INFRASTRUCTURE.  A Deflate launch with units that share history (SWC_DEFLATE_LINKED) compiled for the
// HOST (g++ -DSWC_HOST_EMULATION): phase 1 -- one wave or the team --, the placing scan, and phase 2 as launch_inflate_phase2 issues
// it: the copy kernel (or, below the wave copier's threshold, the resolver), each skipping the chains, then the chain kernel
// (csrc/deflate_chain.h), with or without the CRC tail; the bodies of csrc/job_kernels.h called first-to-last or last-to-first.  Part
// of libswc_emu.so (emu.cpp includes it; tests/_emu_deflate_linked.py); it takes phase 1 and the scan from emu_deflate_units.cpp.
// Never shipped.
//
// With -DEMU_DEFLATE_LINKED_MAIN the file is a stand-alone program (for -fsanitize=address,undefined): it reads runs and what is
// expected of them from a file written by tests/test_deflate_linked_emulation.py and runs every case in the three lane orders, with
// both forms of phase 1, the three arrangements of phase 2 and both orders of the bodies, in allocations of exactly the lines the
// contract names.
#include "emu_deflate_units.cpp"

// arrangement: 0 = swc_lz_resolve_kernel | swc_deflate_chain_kernel (| swc_crc32_kernel): a launch below the wave copier's threshold;
//              1 = swc_lz_copy_kernel | swc_deflate_chain_kernel, with `crcs` the CRC forms of both;
//              2 = the chain body over every job (only_chain = 0): what it does with jobs that have no chain
static void emu_linked_phase2(swc::Job* jobs, size_t n, const EmuWs& ws, int arrangement, int reversed, uint32_t* crcs) {
    using namespace swc;
    using CFG = lzc::CfgDeflate;
    auto each = [&](auto&& body) { for (size_t i = 0; i < n; i++) body((uint32_t)(reversed ? n - 1 - i : i)); };
    // swc_deflate_chain_kernel: a wave per tile of 64 jobs, or -- reversed -- a grid of two waves that stride over the tiles, the second first
    const uint32_t tiles = (uint32_t)((n + 63) / 64), grid = reversed && tiles > 2 ? 2u : tiles;
    auto chains = [&](uint32_t* c) {
        for (uint32_t i = 0; i < grid; i++) {
            const uint32_t w = reversed ? grid - 1 - i : i;
            if (c) jobk::deflate_chains<CFG, true>(jobs, w, grid, (uint32_t)n, ws, emu_lds<lzc::Lds<CFG::kWin>>(), 0, c, emu_wave_consts());
            else jobk::deflate_chains<CFG, false>(jobs, w, grid, (uint32_t)n, ws, emu_lds<lzc::Lds<CFG::kWin>>(), 0);
        }
    };
    if (arrangement == 0) {
        each([&](uint32_t g) { jobk::lz_resolve_unlinked(jobs, g, (uint32_t)n, ws, emu_lds<lzr::Lds<kInflateResolveThreads, kInflateRingLog2>>(), nullptr); });
        chains(nullptr);
        if (crcs) each([&](uint32_t g) { jobk::crc32_wave(jobs, g, crcs, emu_wave_consts(), 0); });
        return;
    }
    if (arrangement == 1) {
        if (crcs) each([&](uint32_t g) { jobk::lz_copy_unlinked<CFG, true>(jobs, g, (uint32_t)n, ws, emu_lds<lzc::Lds<CFG::kWin>>(), 0, crcs, emu_wave_consts()); });
        else each([&](uint32_t g) { jobk::lz_copy_unlinked<CFG, false>(jobs, g, (uint32_t)n, ws, emu_lds<lzc::Lds<CFG::kWin>>(), 0); });
        return chains(crcs);
    }
    if (crcs) each([&](uint32_t g) { jobk::deflate_copy<CFG, true>(jobs, g, (uint32_t)n, ws, emu_lds<lzc::Lds<CFG::kWin>>(), 0, 0, crcs, emu_wave_consts()); });
    else each([&](uint32_t g) { jobk::deflate_copy<CFG, false>(jobs, g, (uint32_t)n, ws, emu_lds<lzc::Lds<CFG::kWin>>(), 0, 0); });
}

// One launch of SWC_CODEC_DEFLATE.  reach: nullptr, or n words that get what phase 1 left in every job's stream header (pad0).
extern "C" void emu_deflate_linked(swc::Job* jobs, size_t n, int arrangement, int team, int reversed, uint32_t* crcs, uint32_t* reach) {
    std::vector<std::vector<uint8_t>> areas(n);
    const EmuWs ws{areas.data(), 0};
    for (size_t g = 0; g < n; g++) {
        emu_ws_give(areas[g], jobs[g].out_cap);
        emu_inflate_phase1(jobs, (uint32_t)g, ws, team);
        if (reach) reach[g] = ((const swc::lzr::StreamHeader*)ws.area((uint32_t)g))->pad0;
    }
    emu_deflate_place(jobs, n, reversed);
    emu_linked_phase2(jobs, n, ws, arrangement, reversed, crcs);
}

#ifdef EMU_DEFLATE_LINKED_MAIN
namespace {
// pin: 0 = the status and aux only, 1 = the sizes as well, 2 = and the bytes
struct LinkedSpec { int32_t aux; std::vector<uint8_t> in; uint32_t cap; int32_t status; uint32_t pin, out_len; int32_t aux_out; uint32_t consumed; std::vector<uint8_t> want; };
struct LinkedBuf { uint8_t* raw; size_t mis, room, alloc, end; };
uint32_t bitwise_crc32(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}
}  // namespace

// File: u32 cases; per case: u32 jobs -- every job without SWC_DEFLATE_JOINED starts a run with a buffer of its own -- and per job
// i32 aux, u32 length + unit, u32 capacity, i32 expected status, u32 pin, u32 expected out_len, i32 expected aux, u32 expected
// in_consumed, u32 length + the bytes the job must leave at its `out`.
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    Reader r(argv[1]);
    int bad = 0;
    const uint32_t ncases = r.u32();
    for (uint32_t c = 0; c < ncases; c++) {
        std::vector<LinkedSpec> js(r.u32());
        size_t in_bytes = 0;
        for (auto& j : js) {
            j.aux = (int32_t)r.u32(); j.in = r.bytes(r.u32()); j.cap = r.u32(); j.status = (int32_t)r.u32(); j.pin = r.u32(); j.out_len = r.u32();
            j.aux_out = (int32_t)r.u32(); j.consumed = r.u32(); j.want = r.bytes(r.u32());
            in_bytes += j.in.size();
        }
        const bool large = in_bytes > 20000 || js.size() > 64;
        // modes: 3 lane orders x (one wave | team) x (resolver + chain | copy + chain | copy + chain with CRC tails) x both orders of the bodies
        for (int mode = 0; mode < 36; mode++) {
            const int order = mode % 3, team = (mode / 3) & 1, arr = (mode / 6) % 3, reversed = mode / 18;
            const int arrangement = arr == 0 ? 0 : 1, crc = arr == 2;
            if (large && order != (team + arr + reversed) % 3) continue;   // (the long cases: every combination once, the lane order rotating)
            for (size_t mis : {(size_t)0, (size_t)1, (size_t)7, (size_t)15}) {
                if (large && mis != 7) continue;
                emu_set_order(order);
                std::vector<uint32_t> crcs(js.size(), 0xA5A5A5A5u);
                std::vector<std::vector<uint8_t>> ins;
                for (auto& j : js) { ins.emplace_back(j.in.size() ? j.in.size() : 1); if (!j.in.empty()) memcpy(ins.back().data(), j.in.data(), j.in.size()); }
                std::vector<swc::Job> jobs(js.size());
                std::vector<LinkedBuf> bufs;
                std::vector<int> buf_of(js.size(), -1);
                for (size_t i = 0; i < js.size(); i++) {
                    memset(&jobs[i], 0, sizeof(swc::Job));
                    jobs[i].in = ins[i].data();
                    jobs[i].in_len = js[i].in.size();
                    jobs[i].out_cap = js[i].cap;
                    jobs[i].aux = js[i].aux;
                    jobs[i].status = 902;
                    if (!(js[i].aux & 1)) {
                        size_t room = js[i].cap;
                        for (size_t k = i + 1; k < js.size() && (js[k].aux & 1); k++) room += js[k].cap;
                        const size_t alloc = (mis + room + 15) / 16 * 16 + 16;   // the lines the contract names: the sanitizer sees every access beyond them
                        uint8_t* raw = (uint8_t*)aligned_alloc(16, alloc);
                        memset(raw, 0xA5, alloc);
                        bufs.push_back(LinkedBuf{raw, mis, room, alloc, 0});
                        jobs[i].out = raw + mis;
                    }
                    buf_of[i] = (int)bufs.size() - 1;
                }
                emu_deflate_linked(jobs.data(), jobs.size(), arrangement, team, reversed, crc ? crcs.data() : nullptr, nullptr);
                bool ok = true;
                for (size_t i = 0; i < js.size(); i++) {
                    ok = ok && jobs[i].status == js[i].status && jobs[i].aux == js[i].aux_out;
                    if (buf_of[i] < 0) { ok = ok && jobs[i].out_len == 0 && jobs[i].in_consumed == 0 && (!crc || crcs[i] == 0u); continue; }   // (no head)
                    LinkedBuf& b = bufs[(size_t)buf_of[i]];
                    if (!(js[i].aux & 1)) b.end = 0;
                    ok = ok && jobs[i].out == b.raw + b.mis + b.end;                                   // right behind what its predecessor says exists
                    const size_t made = (size_t)(jobs[i].out_len < jobs[i].out_cap ? jobs[i].out_len : jobs[i].out_cap);
                    ok = ok && b.end + made <= b.room;
                    if (js[i].pin >= 1) ok = ok && jobs[i].out_len == js[i].out_len && jobs[i].in_consumed == js[i].consumed;
                    if (js[i].pin >= 2) ok = ok && made == js[i].want.size() && (made == 0 || memcmp(b.raw + b.mis + b.end, js[i].want.data(), made) == 0);
                    if (crc && ok) ok = crcs[i] == bitwise_crc32(b.raw + b.mis + b.end, made);   // (every case is far below kCrcGroupLen)
                    b.end += made;
                }
                for (LinkedBuf& b : bufs) {
                    for (size_t i = 0; i < b.mis; i++) ok = ok && b.raw[i] == 0xA5;
                    for (size_t i = b.mis + b.end; i < b.alloc; i++) ok = ok && b.raw[i] == 0xA5;   // nothing behind what the run produced
                    free(b.raw);
                }
                if (!ok) { fprintf(stderr, "case %u order %d team %d arrangement %d crc %d reversed %d misalignment %zu: mismatch\n", c, order, team, arrangement, crc, reversed, mis); bad++; }
            }
        }
    }
    printf("%u cases, %d mismatches\n", ncases, bad);
    return bad ? 1 : 0;
}
#endif
