// emu_compress_built.cpp -- TEST INFRASTRUCTURE.  The LZ4 and Deflate encoders (csrc/lz4_comp.h, csrc/deflate_comp.h, static and
// dynamic) compiled for the HOST (g++ -DSWC_HOST_EMULATION) as a stand-alone program for -fsanitize=address,undefined: with
// -DEMU_COMPRESS_BUILT_MAIN it reads the built cases of tests/_compress_cases.py and what the Python tier got for them from a file
// written by tests/test_compress_built_emulation.py, runs every job in the three lane orders with its input in a heap allocation
// of exactly prefix + in_len bytes and its output in exactly out_cap bytes, and compares status, out_len and bytes.  Not part of
// libswc_emu.so (the library's entry points of the encoders are in emu.cpp).  Never shipped.
#ifdef EMU_COMPRESS_BUILT_MAIN
#include "emu_util.h"

// File: u32 jobs; per job: u32 codec (0 LZ4, 1 Deflate static, 2 Deflate dynamic), u32 prefix length, u32 length of prefix + input,
// the bytes, u32 out_cap, i32 expected status, u32 expected out_len, u32 count + the bytes expected in [out, out + count)
// (count 0xFFFFFFFF: the bytes are not compared).
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    Reader r(argv[1]);
    const uint32_t njobs = r.u32();
    int bad = 0;
    for (uint32_t c = 0; c < njobs; c++) {
        const uint32_t codec = r.u32(), prefix = r.u32();
        const std::vector<uint8_t> in = r.bytes(r.u32());
        const uint32_t cap = r.u32();
        const int32_t status = (int32_t)r.u32();
        const uint32_t out_len = r.u32(), nwant = r.u32();
        const std::vector<uint8_t> want = nwant == 0xFFFFFFFFu ? std::vector<uint8_t>() : r.bytes(nwant);
        for (int order = 0; order < 3; order++) {
            emu_set_order(order);
            // exactly the bytes the contract names: the sanitizer sees every access beyond them
            uint8_t* src = (uint8_t*)malloc(in.size());
            uint8_t* out = (uint8_t*)malloc(cap);
            if (!in.empty()) memcpy(src, in.data(), in.size());
            if (cap) memset(out, 0xA5, cap);
            swc::Job job;
            memset(&job, 0, sizeof job);
            job.in = src;
            job.in_len = in.size();
            job.out = out;
            job.out_cap = cap;
            job.dict_len = prefix;
            job.status = 902;
            if (codec == 0) swc::jobk::lz4_compress<64>(&job, 0, emu_lds<std::array<uint16_t, swc::lz4c::kHashSize>>()->data(), 0);
            else if (codec == 1) swc::jobk::deflate_compress<64>(&job, 0, emu_lds<swc::defc::Lds>(), 0);
            else swc::jobk::deflate_compress_dynamic<64>(&job, 0, emu_lds<swc::defc::DynLds>(), 0);
            bool ok = job.status == status && job.out_len == out_len && job.in_consumed == in.size();
            ok = ok && (in.empty() || memcmp(src, in.data(), in.size()) == 0);
            if (nwant != 0xFFFFFFFFu) ok = ok && want.size() <= cap && (want.empty() || memcmp(out, want.data(), want.size()) == 0);
            if (!ok) { fprintf(stderr, "job %u (codec %u) order %d: status %d out_len %llu, expected %d %u\n", c, codec, order, job.status, (unsigned long long)job.out_len, status, out_len); bad++; }
            free(src);
            free(out);
        }
    }
    printf("%u jobs, %d mismatches\n", njobs, bad);
    return bad ? 1 : 0;
}
#endif
