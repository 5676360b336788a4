// emu_util.h -- TEST INFRASTRUCTURE.  What the sources of the host emulation share.  libswc_emu.so is ONE translation unit
// (emu.cpp, which includes the other emu_*.cpp at its end); a stand-alone sanitizer program is one of those sources alone with its
// -D..._MAIN.  Either way this header is read once per link, so the one emu_set_order is defined here.  Never shipped.
#pragma once
#include <vector>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include "../../swcompression_amd/csrc/inflate_sync.h"
#include "../../swcompression_amd/csrc/crc32_wave.h"

// thread order of every SIMT region (csrc/simt.h): 0 forward, 1 reverse, 2 shuffled
extern "C" void emu_set_order(int o) { swc::simt::g_order = o; }

// the constants of the wave CRC-32 (crc32_wave.h), built at the first call
inline const swc::crcw::WaveConsts* emu_wave_consts() {
    static swc::crcw::WaveConsts consts;
    static bool built = false;
    if (!built) { swc::crcw::build_consts<1>(&consts, 0); built = true; }
    return &consts;
}

// A team of wavefronts for phase 1 of one Deflate stream (inflate_sync.h) as a launch hands it over: the waves' LDS and what they
// share filled with 0xEE, no tables held, no command; the helpers' rows 0xCD.  One at a time.
struct EmuTeam {
    std::vector<uint8_t> rows;
    swc::inflate::Team tm;
    EmuTeam() : rows((swc::inflate::kTeamWaves - 1) * swc::inflate::kTeamProvBytes + 16, (uint8_t)0xCD) {
        alignas(16) static swc::inflate::SyncLds tl[swc::inflate::kTeamWaves];
        alignas(16) static swc::inflate::TeamShared tsh;
        std::memset(tl, 0xEE, sizeof tl);
        std::memset(&tsh, 0xEE, sizeof tsh);
        for (auto& h : tsh.hgen) h = 0;
        tsh.cmd = 0;
        tm.sh = &tsh; tm.lds = tl; tm.scratch = rows.data(); tm.helpers = swc::inflate::kTeamWaves - 1; tm.gen = 0;
    }
};

// the case file of a stand-alone program: read whole, then taken apart front to back; a short file ends the program
struct Reader {
    std::vector<uint8_t> d;
    size_t at = 0;
    explicit Reader(const char* path) {
        FILE* f = fopen(path, "rb");
        if (!f) { perror(path); exit(2); }
        uint8_t buf[65536];
        size_t k;
        while ((k = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + k);
        fclose(f);
    }
    void need(size_t n) const { if (at + n > d.size()) { fprintf(stderr, "case file too short\n"); exit(2); } }
    uint32_t u32() { uint32_t v; need(4); memcpy(&v, d.data() + at, 4); at += 4; return v; }
    std::vector<uint8_t> bytes(size_t n) { need(n); std::vector<uint8_t> v(d.begin() + (long)at, d.begin() + (long)(at + n)); at += n; return v; }
};
