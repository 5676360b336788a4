// emu_lzma_comp.cpp -- TEST INFRASTRUCTURE.  LZMA2 compression (csrc/lzma_comp.h) compiled for the HOST: emu_lzma2_compress_jobs runs
// the body of swc_lzma2_compress_kernel (csrc/job_kernels.h) job by job.  A small library of its own (tests/_emu_lzma_comp.py).  Never shipped.
//
// With -DEMU_LZMA_COMP_MAIN the file is a stand-alone program (for -fsanitize=address,undefined): it reads a case file written by
// tests/test_lzma2_compress.py and places every input and every output at the END of an allocation of its own, so that a byte
// read or written behind either shows.  One line per case goes out: index, status, out_len and a sum of the bytes that exist.
#include "emu_util.h"

extern "C" void emu_lzma2_compress_jobs(swc::Job* jobs, size_t n) {
    for (size_t g = 0; g < n; g++) swc::jobk::lzma2_compress<64>(jobs, (uint32_t)g, emu_lds<swc::lzmac::Lds>(), 0);
}
extern "C" uint64_t emu_lzma2_compress_bound(uint64_t n) { return swc::lzmac::bound(n); }

#ifdef EMU_LZMA_COMP_MAIN
#include <memory>
// File: u32 cases; per case u32 capacity, u32 aux, u32 thread order (csrc/simt.h), u32 length + the input.
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    Reader r(argv[1]);
    const uint32_t ncases = r.u32();
    for (uint32_t c = 0; c < ncases; c++) {
        const uint32_t cap = r.u32(), aux = r.u32(), order = r.u32();
        const std::vector<uint8_t> data = r.bytes(r.u32());
        std::unique_ptr<uint8_t[]> in(new uint8_t[data.size()]), out(new uint8_t[cap]);   // exact: a sanitizer sees every overrun
        if (!data.empty()) memcpy(in.get(), data.data(), data.size());
        memset(out.get(), 0xA5, cap);
        swc::simt::g_order = (int)order;
        swc::Job j{};
        j.in = in.get(); j.in_len = data.size();
        j.out = out.get(); j.out_cap = cap;
        j.aux = (int32_t)aux;
        j.status = -1;
        emu_lzma2_compress_jobs(&j, 1);
        const uint64_t made = j.out_len < cap ? j.out_len : cap;
        uint64_t sum = 0;
        for (uint64_t i = 0; i < made; i++) sum = (sum * 131 + out[i]) & 0xFFFFFFFFFFFFull;
        for (uint64_t i = made; i < cap; i++) if (out[i] != 0xA5) { printf("case %u: byte %llu behind the output written\n", c, (unsigned long long)i); return 1; }
        printf("%u %d %llu %llu\n", c, j.status, (unsigned long long)j.out_len, (unsigned long long)sum);
    }
    return 0;
}
#endif
