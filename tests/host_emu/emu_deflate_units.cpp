// emu_deflate_units.cpp -- TEST INFRASTRUCTURE.  A Deflate launch -- phase 1 with the OPEN rule, the placing scan
// (csrc/deflate_place.h), the copy, the fused CRC-32 -- compiled for the HOST (g++ -DSWC_HOST_EMULATION): the kernel bodies of
// csrc/job_kernels.h in the order launch_inflate issues the kernels.  Part of libswc_emu.so (emu.cpp includes it).  Never shipped.
//
// With -DEMU_DEFLATE_UNITS_MAIN the file is a stand-alone program (for -fsanitize=address,undefined): it reads runs and what is
// expected of them from a file written by tests/test_deflate_units_emulation.py, runs every case at the sixteen alignments of its
// buffers, in the three lane orders, with both copiers, both copy orders, the team instantiation of phase 1 and the CRC form of the
// copy, and compares; the placing scan runs on the size lists of the same test as well.
#ifndef EMU_DEFLATE_UNITS_CPP   // (not #pragma once: this is also the main file of its own program)
#define EMU_DEFLATE_UNITS_CPP
#include "emu_util.h"
#include "../../swcompression_amd/csrc/deflate_place.h"

// phase 1 of job g: swc_inflate_team_kernel (its helpers' rows in an allocation of their own) or swc_inflate_sync_kernel
static void emu_inflate_phase1(swc::Job* jobs, uint32_t g, const EmuWs& ws, int team) {
    using namespace swc;
    if (team) {
        std::vector<uint8_t> rows(jobk::kTeamScratchBytes + 16, (uint8_t)0xCD);
        jobk::inflate_team<1>(jobs + g, 0, ws.from(g), rows.data(), emu_lds<std::array<inflate::SyncLds, inflate::kTeamWaves>>()->data(),
                              emu_lds<inflate::TeamShared>(), 0, 0);
    } else {
        jobk::inflate_sync<1>(jobs, g, ws, emu_lds<inflate::SyncLds>(), 0, nullptr);
    }
}
// phase 2 of job g.  copier: 0 = swc_lz_resolve_kernel (then, with `crcs`, swc_crc32_kernel), else swc_lz_copy_kernel or, with
// `crcs`, swc_lz_copy_crc32_kernel (2: in the 7 KiB window).  The streams of kCrcGroupLen and more are swc_crc32_group_kernel's.
template <typename CFG>
static void emu_lz_copy(const swc::Job* jobs, uint32_t g, const EmuWs& ws, uint32_t* crcs) {
    using namespace swc;
    if (crcs) jobk::lz_copy<CFG, true>(jobs, g, ws, emu_lds<lzc::Lds<CFG::kWin>>(), 0, crcs, emu_wave_consts());
    else jobk::lz_copy<CFG, false>(jobs, g, ws, emu_lds<lzc::Lds<CFG::kWin>>(), 0);
}
static void emu_inflate_phase2(const swc::Job* jobs, uint32_t g, const EmuWs& ws, int copier, uint32_t* crcs) {
    using namespace swc;
    if (copier == 2) return emu_lz_copy<lzc::CfgLz4>(jobs, g, ws, crcs);
    if (copier) return emu_lz_copy<lzc::CfgDeflate>(jobs, g, ws, crcs);
    jobk::lz_resolve(jobs, g, ws, emu_lds<lzr::Lds<kInflateResolveThreads, kInflateRingLog2>>(), nullptr);
    if (crcs) jobk::crc32_wave(jobs, g, crcs, emu_wave_consts(), 0);
}

// Deflate, every job through both phases before the next (one workspace at a time; no joined units: the scan has nothing to place)
extern "C" uint64_t emu_team_adopted(int reset) { const uint64_t v = swc::inflate::g_team_adopted; if (reset) swc::inflate::g_team_adopted = 0; return v; }
extern "C" void emu_inflate_sync(swc::Job* jobs, size_t n) {
    std::vector<uint8_t> one;
    for (size_t g = 0; g < n; g++) {
        emu_ws_give(one, jobs[g].out_cap);
        emu_inflate_phase1(jobs + g, 0, EmuWs{&one, 0}, g_team);
        emu_inflate_phase2(jobs + g, 0, EmuWs{&one, 0}, g_copier, nullptr);
    }
}

// The placing scan alone over a job list whose out_len / out_cap / aux are given: tiles in forward (0) or reverse (1) order.
extern "C" void emu_deflate_place(swc::Job* jobs, size_t n, int tiles_reversed) {
    const uint32_t tiles = (uint32_t)((n + swc::defp::kTile - 1) / swc::defp::kTile);
    for (uint32_t i = 0; i < tiles; i++) swc::defp::place_tile(jobs, (uint32_t)n, tiles_reversed ? tiles - 1 - i : i);
}

// One launch of SWC_CODEC_DEFLATE: phase 1 | place | copy.  copier: 1 = the wave kernel, 0 = the workgroup kernel; team: phase 1 by
// a team of wavefronts; reversed: the tiles and the copies from the last job to the first; crcs: nullptr, or n words the launch
// leaves as launch_inflate does.
extern "C" void emu_deflate_units(swc::Job* jobs, size_t n, int copier, int team, int reversed, uint32_t* crcs) {
    std::vector<std::vector<uint8_t>> areas(n);
    const EmuWs ws{areas.data(), 0};
    for (size_t g = 0; g < n; g++) {
        emu_ws_give(areas[g], jobs[g].out_cap);
        emu_inflate_phase1(jobs, (uint32_t)g, ws, team);
    }
    emu_deflate_place(jobs, n, reversed);
    for (size_t i = 0; i < n; i++) emu_inflate_phase2(jobs, (uint32_t)(reversed ? n - 1 - i : i), ws, copier, crcs);
}

#ifdef EMU_DEFLATE_UNITS_MAIN
namespace {
struct JobSpec { int32_t aux; std::vector<uint8_t> in; uint32_t cap; int32_t status; uint32_t pinned, out_len; int32_t aux_out; uint32_t consumed; std::vector<uint8_t> want; };
struct Buf { uint8_t* raw; size_t mis, room, alloc, end; };
uint32_t plain_crc32(const uint8_t* p, size_t n) {   // bit by bit: the reference of the CRC modes
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

// The placing scan on job lists given by their sizes (the lists of tests/test_deflate_units_emulation.py), against the serial rule.
int check_place() {
    int bad = 0;
    std::vector<uint64_t> sizes, caps;
    std::vector<int32_t> aux;
    auto add = [&](uint64_t s, uint64_t c, int32_t a) { sizes.push_back(s); caps.push_back(c); aux.push_back(a); };
    for (int i = 0; i < 70; i++) add(10, 10, 1);                                   // no head: a tile of orphans and six more
    for (int i = 0; i < 200; i++) add(300, 300, i == 0 ? 2 : i == 199 ? 1 : 3);     // a run over three tile borders
    add(17, 17, 2); add(5, 5, 3); add(9, 9, 1); add(40, 64, 2); add(41, 64, 1);     // two runs inside one tile
    add(1, 1, 2); add(0, 1, 3); add(70001, 70001, 3); add(0, 8, 3); add(1, 1, 1);
    add(5000, 100, 0); add(10, 10, 3); add(3, 3, 1);                                // over capacity: the capacity counts
    for (int order = 0; order < 3; order++)
        for (int rev = 0; rev < 2; rev++) {
            emu_set_order(order);
            std::vector<swc::Job> jobs(sizes.size());
            for (size_t i = 0; i < jobs.size(); i++) {
                memset(&jobs[i], 0, sizeof(swc::Job));
                jobs[i].out_len = sizes[i]; jobs[i].out_cap = caps[i]; jobs[i].aux = aux[i]; jobs[i].status = 902; jobs[i].in_consumed = 7;
                if (!(aux[i] & 1)) jobs[i].out = (uint8_t*)(uintptr_t)(0x10000u + ((uint64_t)i << 32));
            }
            emu_deflate_place(jobs.data(), jobs.size(), rev);
            uint64_t head = 0, at = 0;
            bool have = false, ok = true;
            for (size_t i = 0; i < jobs.size(); i++) {
                if (!(aux[i] & 1)) { have = true; head = 0x10000u + ((uint64_t)i << 32); at = 0; }
                if (!have) { ok = ok && jobs[i].status == SWC_E_INVALID_ARGUMENT && jobs[i].out_len == 0 && jobs[i].in_consumed == 0 && jobs[i].out == nullptr; continue; }
                ok = ok && (uint64_t)(uintptr_t)jobs[i].out == head + at && jobs[i].status == 902 && jobs[i].out_len == sizes[i];
                at += sizes[i] < caps[i] ? sizes[i] : caps[i];
            }
            if (!ok) { fprintf(stderr, "place scan: order %d reversed %d: mismatch\n", order, rev); bad++; }
        }
    return bad;
}
}  // namespace

// File: u32 cases; per case: u32 jobs -- every job without SWC_DEFLATE_JOINED starts a run with a buffer of its own -- and per job
// i32 aux, u32 length + unit, u32 capacity, i32 expected status, u32 pinned (0: only the status and aux are compared -- a failed
// unit), u32 expected out_len, i32 expected aux, u32 expected in_consumed, u32 length + the bytes the job must leave at its `out`.
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    Reader r(argv[1]);
    int bad = check_place();
    const uint32_t ncases = r.u32();
    for (uint32_t c = 0; c < ncases; c++) {
        std::vector<JobSpec> js(r.u32());
        for (auto& j : js) {
            j.aux = (int32_t)r.u32(); j.in = r.bytes(r.u32()); j.cap = r.u32(); j.status = (int32_t)r.u32(); j.pinned = r.u32(); j.out_len = r.u32();
            j.aux_out = (int32_t)r.u32(); j.consumed = r.u32(); j.want = r.bytes(r.u32());
        }
        // modes: 3 lane orders x 2 copiers x 2 copy orders with one wave per unit, the team of wavefronts once per lane order, and
        // the wave copier that ends with the CRC-32 of its output once per lane order
        for (int mode = 0; mode < 18; mode++) {
            const int order = mode % 3, team = mode >= 12 && mode < 15, crc = mode >= 15, copier = mode >= 12 ? 1 : (mode / 3) & 1, reversed = mode >= 12 ? 0 : mode / 6;
            std::vector<uint32_t> crcs(js.size(), 0xA5A5A5A5u);
            for (size_t mis = 0; mis < 16; mis++) {
                if (js.size() > 64 && mis != 0 && mis != 7) continue;   // (the long lists: two alignments)
                emu_set_order(order);
                std::vector<std::vector<uint8_t>> ins;
                for (auto& j : js) { ins.emplace_back(j.in.size() ? j.in.size() : 1); if (!j.in.empty()) memcpy(ins.back().data(), j.in.data(), j.in.size()); }
                std::vector<swc::Job> jobs(js.size());
                std::vector<Buf> bufs;
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
                        // the bytes the contract names, rounded up to the 16-byte lines they lie in: the sanitizer sees every access beyond them
                        const size_t alloc = (mis + room + 15) / 16 * 16 + 16;
                        uint8_t* raw = (uint8_t*)aligned_alloc(16, alloc);
                        memset(raw, 0xA5, alloc);
                        bufs.push_back(Buf{raw, mis, room, alloc, 0});
                        jobs[i].out = raw + mis;
                    }
                    buf_of[i] = (int)bufs.size() - 1;
                }
                emu_deflate_units(jobs.data(), jobs.size(), copier, team, reversed, crc ? crcs.data() : nullptr);
                bool ok = true;
                for (size_t i = 0; i < js.size(); i++) {
                    ok = ok && jobs[i].status == js[i].status && jobs[i].aux == js[i].aux_out;
                    if (buf_of[i] < 0) { ok = ok && jobs[i].out_len == 0 && jobs[i].in_consumed == 0 && (!crc || crcs[i] == 0u); continue; }   // (joined to nothing)
                    Buf& b = bufs[(size_t)buf_of[i]];
                    if (!(js[i].aux & 1)) b.end = 0;
                    ok = ok && jobs[i].out == b.raw + b.mis + b.end;                                   // right behind what its predecessor says exists
                    const size_t made = (size_t)(jobs[i].out_len < jobs[i].out_cap ? jobs[i].out_len : jobs[i].out_cap);
                    if (js[i].pinned)
                        ok = ok && jobs[i].out_len == js[i].out_len && jobs[i].in_consumed == js[i].consumed && made == js[i].want.size() && b.end + made <= b.room &&
                             (made == 0 || memcmp(b.raw + b.mis + b.end, js[i].want.data(), made) == 0);
                    if (crc) ok = ok && crcs[i] == plain_crc32(b.raw + b.mis + b.end, made);   // (every case is far below kCrcGroupLen)
                    b.end += made;
                }
                for (Buf& b : bufs) {
                    for (size_t i = 0; i < b.mis; i++) ok = ok && b.raw[i] == 0xA5;
                    for (size_t i = b.mis + b.end; i < b.alloc; i++) ok = ok && b.raw[i] == 0xA5;   // nothing behind what the run produced
                    free(b.raw);
                }
                if (!ok) { fprintf(stderr, "case %u order %d copier %d team %d reversed %d crc %d misalignment %zu: mismatch\n", c, order, copier, team, reversed, crc, mis); bad++; }
            }
        }
    }
    printf("%u cases, %d mismatches\n", ncases, bad);
    return bad ? 1 : 0;
}
#endif
#endif   // EMU_DEFLATE_UNITS_CPP
