// emu_bzip2_marks.cpp -- TEST INFRASTRUCTURE.  The scan for bzip2 marks (swcompression_amd/csrc/bzip2_scan.h) built for the HOST
// (g++ -DSWC_HOST_EMULATION): the four bodies as launch_bzip2_index runs them, the 64 threads of every SIMT region one after
// another in the order emu_set_order selects, the waves of a launch in that order too.  A small library of its own
// (tests/_emu_bzip2_marks.py).  Never shipped.
//
// With -DEMU_BZIP2_MARKS_MAIN the file is a stand-alone program (for -fsanitize=address,undefined): it reads buffers and the refs
// the rule expects of them from a file written by tests/test_bzip2_marks_emulation.py and indexes each in all three thread orders,
// the buffer the LAST bytes of a heap allocation at the residue the case names, the refs in an allocation of exactly the refs that
// are to be written: a read outside the buffer or a ref too many is a heap overflow the sanitizer reports.
#include "emu_util.h"
#include "../../swcompression_amd/csrc/bzip2_scan.h"

namespace bz = swc::bzscan;

extern "C" uint32_t emu_bzip2_scan_tile_bytes() { return bz::kTile; }

// One call of swc_batch_bzip2_index: *n = the marks found, refs[0 .. min(*n, cap)) written.  The workspace is an allocation of
// exactly the plan's bytes, 0xEE-filled.
extern "C" void emu_bzip2_index(const uint8_t* src, uint64_t len, bz::Ref* refs, uint64_t cap, uint64_t* n) {
    const bz::Plan p = bz::plan(len, cap);
    uint8_t* ws = (uint8_t*)malloc(p.bytes ? p.bytes : 1);
    memset(ws, 0xEE, p.bytes);
    uint64_t* prefix = reinterpret_cast<uint64_t*>(ws + p.prefix);
    uint64_t* starts = reinterpret_cast<uint64_t*>(ws + p.starts);
    uint32_t* counts = reinterpret_cast<uint32_t*>(ws + p.counts);
    const uint64_t tiles = bz::tiles(len, (uint32_t)((uintptr_t)src & 15u)), blocks = (p.slots - 1 + 63) / 64;
    auto wave = [](uint64_t i, uint64_t of) { return swc::simt::g_order == 1 ? of - 1 - i : i; };
    for (uint64_t i = 0; i < tiles; i++) bz::count_tile<64>(wave(i, tiles), src, len, counts);
    swc::gzscan::scan_tiles<64>(counts, tiles, prefix, n);
    for (uint64_t i = 0; i < tiles; i++) bz::write_tile<64>(wave(i, tiles), src, len, counts, prefix, starts, p.slots);
    for (uint64_t i = 0; i < blocks; i++) bz::mark_refs<64>(wave(i, blocks), src, len, starts, n, cap, refs);
    free(ws);
}

#ifdef EMU_BZIP2_MARKS_MAIN
// File: u32 cases; per case u32 residue, u32 cap, u32 length, the bytes, u32 n expected, min(n, cap) refs of 32 bytes.
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    Reader r(argv[1]);
    const uint32_t ncases = r.u32();
    int bad = 0;
    for (uint32_t c = 0; c < ncases; c++) {
        const uint32_t res = r.u32(), cap = r.u32(), len = r.u32();
        const std::vector<uint8_t> data = r.bytes(len);
        const uint32_t want_n = r.u32(), m = want_n < cap ? want_n : cap;
        const std::vector<uint8_t> want = r.bytes((size_t)m * sizeof(bz::Ref));
        for (int order = 0; order < 3; order++) {
            emu_set_order(order);
            uint8_t* raw = nullptr;
            if (posix_memalign((void**)&raw, 16, res + len ? res + len : 1) != 0) return 2;
            if (len) memcpy(raw + res, data.data(), len);
            bz::Ref* refs = (bz::Ref*)malloc(m ? (size_t)m * sizeof(bz::Ref) : 1);
            memset(refs, 0xA5, (size_t)m * sizeof(bz::Ref));
            uint64_t n = ~0ull;
            emu_bzip2_index(raw + res, len, refs, cap, &n);
            if (n != want_n || (m && memcmp(refs, want.data(), want.size()) != 0)) {
                fprintf(stderr, "case %u (length %u, residue %u, cap %u), order %d: %llu marks, %u expected, or other refs\n", c, len, res, cap, order,
                        (unsigned long long)n, want_n);
                bad++;
            }
            free(refs);
            free(raw);
        }
    }
    printf("%u cases in 3 orders, %d mismatches\n", ncases, bad);
    return bad ? 1 : 0;
}
#endif
