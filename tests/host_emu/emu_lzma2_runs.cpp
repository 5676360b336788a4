// emu_lzma2_runs.cpp -- TEST INFRASTRUCTURE.  The units of LZMA2 streams cut at their dictionary resets (include/swc_hip.h:
// SWC_LZMA2_OPEN) through emu_lzma_mode -- the body of swc_lzma_kernel compiled for the HOST -- as a stand-alone program for
// -fsanitize=address,undefined (-DEMU_LZMA2_RUNS_MAIN; not part of libswc_emu.so).  Never shipped.
//
// Every stream lies ONCE in an allocation of exactly its length and every unit is a job over its sub-range of it, in place: the next
// unit's control byte follows a unit directly, and a read behind the last unit is a read behind the allocation.  The outputs lie
// back to back in one allocation of exactly the sum of the units' sizes.  The program applies the acceptance rule and compares the
// joined output and the consumed input with what tests/test_lzma2_runs_emulation.py wrote into the case file.
#ifdef EMU_LZMA2_RUNS_MAIN
#include "emu.cpp"

namespace {
struct Unit { uint32_t offset, comp_len, uncomp_len, aux; };
}

// File: u32 cases; per case: u32 length + the chunks of the stream (no dictionary-size byte), u32 units, per unit u32 offset,
// u32 comp_len, u32 uncomp_len, u32 aux, then u32 expected in_consumed and u32 length + the bytes the stream decodes to.
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    Reader r(argv[1]);
    int bad = 0;
    const uint32_t ncases = r.u32();
    for (uint32_t c = 0; c < ncases; c++) {
        const std::vector<uint8_t> stream = r.bytes(r.u32());
        std::vector<Unit> units(r.u32());
        for (Unit& u : units) { u.offset = r.u32(); u.comp_len = r.u32(); u.uncomp_len = r.u32(); u.aux = r.u32(); }
        const uint32_t consumed = r.u32();
        const std::vector<uint8_t> want = r.bytes(r.u32());
        size_t total = 0;
        for (const Unit& u : units) total += u.uncomp_len;
        for (int mode = 0; mode < 2; mode++) {
            uint8_t* in = (uint8_t*)malloc(stream.size() ? stream.size() : 1);
            uint8_t* out = (uint8_t*)malloc(total ? total : 1);
            if (!stream.empty()) memcpy(in, stream.data(), stream.size());
            memset(out, 0xA5, total ? total : 1);
            std::vector<swc::Job> jobs(units.size());
            size_t at = 0;
            for (size_t i = 0; i < units.size(); i++) {
                memset(&jobs[i], 0, sizeof(swc::Job));
                jobs[i].in = in + units[i].offset;
                jobs[i].in_len = units[i].comp_len;
                jobs[i].out = out + at;
                jobs[i].out_cap = units[i].uncomp_len;
                jobs[i].aux = (int32_t)units[i].aux;
                jobs[i].status = 902;
                at += units[i].uncomp_len;
            }
            emu_lzma_mode(jobs.data(), jobs.size(), 1, mode);
            bool ok = !units.empty() && memcmp(in, stream.data(), stream.size()) == 0;
            for (size_t i = 0; ok && i + 1 < units.size(); i++)
                ok = jobs[i].status == SWC_OK && (jobs[i].aux & swc::kLzma2Open) != 0 && jobs[i].in_consumed == jobs[i].in_len && jobs[i].out_len == units[i].uncomp_len;
            if (ok) {
                const swc::Job& last = jobs.back();
                ok = last.status == SWC_OK && (last.aux & swc::kLzma2Open) == 0 && units.back().offset + last.in_consumed == consumed &&
                     at - units.back().uncomp_len + last.out_len == want.size() && at == want.size() && (want.empty() || memcmp(out, want.data(), want.size()) == 0);
            }
            if (!ok) { fprintf(stderr, "case %u mode %d: the units do not give the stream\n", c, mode); bad++; }
            free(in);
            free(out);
        }
    }
    printf("%u cases, %d mismatches\n", ncases, bad);
    return bad ? 1 : 0;
}
#endif
