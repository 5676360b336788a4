// emu_util.h -- TEST INFRASTRUCTURE.  What the sources of the host emulation share.  libswc_emu.so, like each of its
// variants, is ONE translation unit (emu.cpp, which includes the other emu_*.cpp at its end); a stand-alone sanitizer program is one
// of those sources alone with its -D..._MAIN.  Either way this header is read once per link, so the one emu_set_order is defined here.  Never shipped.
#pragma once
#include <vector>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <array>
#include "../../swcompression_amd/csrc/job_kernels.h"

// thread order of every SIMT region (csrc/simt.h): 0 forward, 1 reverse, 2 shuffled
extern "C" void emu_set_order(int o) { swc::simt::g_order = o; }

// the constants of the wave CRC-32 (crc32_wave.h), built at the first call
inline const swc::crcw::WaveConsts* emu_wave_consts() {
    static swc::crcw::WaveConsts consts;
    static bool built = false;
    if (!built) { swc::crcw::build_consts<1>(&consts, 0); built = true; }
    return &consts;
}

// ---- test-only switches: which of the product's alternatives a driver hands to the bodies of job_kernels.h ----------------------
// phase 2: 1 = the record-granular copier of lz_copy.h as the library ships it (Deflate: 6 KiB window, LZ4: 7 KiB), 3 = the 6 KiB
// window for both, 2 = the 7 KiB window for both, 0 = the byte-cell resolver of lz_resolve.h (a launch below kCopierMin)
inline int g_copier = 1;
extern "C" void emu_set_copier(int on) { g_copier = on; }
// how the LZ4 parse tells the copier where the literals lie: 1 = eight-byte records, 2 = derived + anchors
inline int g_lz4_mode = SWC_LZ4_RECORD_MODE;
extern "C" void emu_set_lz4_record_mode(int m) { g_lz4_mode = m; }
// Deflate phase 1 with a team of wavefronts per stream (launches of few streams): 0 = one wavefront
inline int g_team = 0;
extern "C" void emu_set_deflate_team(int on) { g_team = on; }

// The workspace map of the emulation (the WS of job_kernels.h): ONE allocation per job, 0xCD-filled, of exactly the bytes the
// contract names + 16, so that a sanitizer sees an overrun of an area.  Job g of the bodies is a[first + g].
struct EmuWs {
    std::vector<uint8_t>* a;
    uint32_t first;
    uint8_t* area(uint32_t g) const { return a[first + g].data(); }
    size_t bytes(uint32_t g) const { return a[first + g].size() - 16; }
    EmuWs from(uint32_t g) const { return EmuWs{a, first + g}; }
};
inline void emu_ws_give(std::vector<uint8_t>& area, uint64_t out_cap) { area.assign(swc::lzr::ws_bytes_per_job(out_cap) + 16, (uint8_t)0xCD); }

// the LDS of a workgroup as a launch hands it over: 0xEE.  One object per type, filled again at every call.
template <typename T>
T* emu_lds() {
    alignas(16) static T l;
    std::memset(static_cast<void*>(&l), 0xEE, sizeof l);
    return &l;
}

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
