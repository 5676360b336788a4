// emu_deflate_phase1.cpp -- TEST INFRASTRUCTURE.  The probes of Deflate phase 1 (tests/_emu_deflate_phase1.py): which of the
// -DSWC_SYNC_* switches of csrc/inflate_sync.h the library was built under, the direct tables sync_tables_from_lengths builds from
// a set of code lengths, read back, and phase 1 of one stream with what it leaves in the workspace (stream header, record list,
// literal stream).  Part of libswc_emu.so and of each of its variants (emu.cpp includes it).  Never shipped.
#include "emu_deflate_units.cpp"

extern "C" int emu_pairs_enabled() { return SWC_SYNC_NO_PAIRS ? 0 : 1; }
extern "C" int emu_sync_follow() { return SWC_SYNC_FOLLOW; }
extern "C" int emu_pairs_lit_bits() { return swc::inflate::kSyncLitBits; }

// lens[0 .. literals + distances): the code lengths of a block.  lut_out: the (1 << kSyncLitBits) + 256 direct entries.  Returns
// whether the fast path takes the block.
extern "C" int emu_pairs_tables(const uint8_t* lens, int literals, int distances, uint32_t* lut_out) {
    using namespace swc::inflate;
    SyncLds* sl = emu_lds<SyncLds>();
    std::vector<uint32_t> spill(swc::lzr::kProvSpillBytes / 4 + 4, 0xCDCDCDCDu);
    Spill sp{spill.data(), (uint16_t*)((uint8_t*)spill.data() + kSpillSyms), (uint32_t*)((uint8_t*)spill.data() + kSpillSub)};
    std::memset(sl->stage + kHdrLens, 0, 320);
    std::memcpy(sl->stage + kHdrLens, lens, (size_t)(literals + distances));
    SubTab st{nullptr};
    SyncProf pf;
    const bool fast = sync_tables_from_lengths(sl, sp, literals, distances, st, pf);
    std::memcpy(lut_out, sl->lut, sizeof sl->lut);
    return fast ? 1 : 0;
}

// Phase 1 of one stream (one wavefront, or the team form).  res: status, out_len, in_consumed, aux, nrec, reach, nlit.  recs_out /
// lits_out: room for max_rec records / max_lit bytes (more than that is not copied; the counts say so).
extern "C" void emu_pairs_phase1(const uint8_t* in, size_t in_len, size_t cap, int aux, int team, uint64_t* res, uint32_t* recs_out,
                                 size_t max_rec, uint8_t* lits_out, size_t max_lit) {
    std::vector<uint8_t> area, out(cap + 16, (uint8_t)0xA5), inb(in, in + in_len);
    if (inb.empty()) inb.push_back(0);
    emu_ws_give(area, cap);
    swc::Job j{};
    j.in = inb.data(); j.in_len = in_len; j.out = out.data(); j.out_cap = cap; j.aux = aux; j.status = 902;
    emu_inflate_phase1(&j, 0, EmuWs{&area, 0}, team);
    const swc::lzr::StreamHeader* h = (const swc::lzr::StreamHeader*)area.data();
    res[0] = (uint64_t)(int64_t)j.status; res[1] = j.out_len; res[2] = j.in_consumed; res[3] = (uint64_t)(int64_t)j.aux;
    res[4] = h->nrec; res[5] = h->pad0; res[6] = h->nlit;
    const size_t wsb = area.size() - 16;
    const uint32_t* r = (const uint32_t*)(area.data() + sizeof(swc::lzr::StreamHeader));
    for (size_t i = 0; i < h->nrec && i < max_rec; i++) recs_out[i] = r[i];
    const uint8_t* l = area.data() + swc::lzr::lit_offset(wsb, cap);
    for (size_t i = 0; i < h->nlit && i < max_lit; i++) lits_out[i] = l[i];
}
