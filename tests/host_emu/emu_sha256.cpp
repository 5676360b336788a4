// emu_sha256.cpp -- TEST INFRASTRUCTURE.  A launch of swc_sha256_kernel (csrc/sha256_lane.h: one job per lane) compiled for the HOST
// (g++ -DSWC_HOST_EMULATION): the body of csrc/job_kernels.h for every lane of every wave of the grid launch_sha256 issues.  Part
// of libswc_emu.so (emu.cpp includes it; tests/_emu_sha256.py).  Never shipped.
//
// With -DEMU_SHA256_MAIN the file is a stand-alone program (for -fsanitize=address,undefined): it reads lengths and the digests
// expected of them from a file written by tests/test_sha256_emulation.py and hashes every message at the sixteen residues of its
// address, each message the LAST bytes of a heap allocation -- a read of one byte behind a message is a heap overflow the sanitizer
// reports -- and the digests in an allocation of exactly 32 n bytes behind an odd number of bytes.
#include "emu_util.h"

// One launch: a grid of ceil(n / 64) waves, lane t of wave b takes job 64 b + t
extern "C" void emu_sha256_jobs(const swc::Job* jobs, size_t n, uint8_t* digests) {
    const size_t waves = (n + 63) / 64;
    for (size_t b = 0; b < waves; b++)
        for (uint32_t t = 0; t < 64; t++) {
            const size_t g = 64 * b + t;
            if (g < n) swc::jobk::sha256_lane(jobs, (uint32_t)g, digests);
        }
}

// the message of a given length that the test and the program agree on
extern "C" void emu_sha256_message(uint8_t* p, size_t len) {
    uint32_t x = 0x9E3779B9u ^ (uint32_t)len;
    for (size_t i = 0; i < len; i++) { x = x * 1664525u + 1013904223u; p[i] = (uint8_t)(x >> 24); }
}

#ifdef EMU_SHA256_MAIN
#include <sanitizer/asan_interface.h>
namespace {
struct Msg { uint8_t* raw; uint8_t* p; size_t front; };
// `len` bytes that end where their allocation ends and start `res` bytes past a 16-byte boundary; the bytes in front of them are
// poisoned as far as the sanitizer's eight-byte granules allow (all of them for res 0 and 8)
Msg place(size_t len, size_t res) {
    Msg m;
    m.front = res;
    m.raw = (uint8_t*)malloc(res + len ? res + len : 1);
    m.p = m.raw + res;
    emu_sha256_message(m.p, len);
    if (res) ASAN_POISON_MEMORY_REGION(m.raw, res);
    return m;
}
void release(Msg& m) {
    if (m.front) ASAN_UNPOISON_MEMORY_REGION(m.raw, m.front);
    free(m.raw);
}
}  // namespace

// File: u32 cases; per case u32 length and the 32 bytes of the digest of emu_sha256_message(length).
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    Reader r(argv[1]);
    const uint32_t ncases = r.u32();
    std::vector<uint32_t> lens(ncases);
    std::vector<std::vector<uint8_t>> want(ncases);
    for (uint32_t c = 0; c < ncases; c++) { lens[c] = r.u32(); want[c] = r.bytes(32); }
    int bad = 0;
    for (size_t res = 0; res < 16; res++) {
        // every message in a launch of its own ...
        for (uint32_t c = 0; c < ncases; c++) {
            Msg m = place(lens[c], res);
            swc::Job job;
            memset(&job, 0, sizeof job);
            job.out = lens[c] ? m.p : nullptr;   // (a message of no bytes: nothing to point at)
            job.out_cap = job.out_len = lens[c];
            uint8_t* dg = (uint8_t*)malloc(32);
            emu_sha256_jobs(&job, 1, dg);
            if (memcmp(dg, want[c].data(), 32) != 0) { fprintf(stderr, "length %u at residue %zu: wrong digest\n", lens[c], res); bad++; }
            free(dg);
            release(m);
        }
        // ... and all of them as the lanes of one launch (message c at residue (res + c) % 16), the digests behind an odd number of bytes
        std::vector<Msg> ms;
        std::vector<swc::Job> jobs(ncases);
        for (uint32_t c = 0; c < ncases; c++) {
            ms.push_back(place(lens[c], (res + c) % 16));
            memset(&jobs[c], 0, sizeof(swc::Job));
            jobs[c].out = lens[c] ? ms[c].p : nullptr;
            jobs[c].out_cap = lens[c];
            jobs[c].out_len = (uint64_t)lens[c] + (c % 3 == 1 ? 1000u : 0u);   // (needed more than its capacity: the capacity is what exists)
            jobs[c].status = c % 5 == 2 ? 103 : 0;
        }
        const size_t odd = 2 * res + 1;
        uint8_t* raw = (uint8_t*)malloc(odd + 32 * (size_t)ncases);
        emu_sha256_jobs(jobs.data(), ncases, raw + odd);
        for (uint32_t c = 0; c < ncases; c++)
            if (memcmp(raw + odd + 32 * (size_t)c, want[c].data(), 32) != 0) { fprintf(stderr, "job %u (length %u) of the launch at residue %zu: wrong digest\n", c, lens[c], res); bad++; }
        free(raw);
        for (Msg& m : ms) release(m);
    }
    printf("%u lengths at 16 residues, %d mismatches\n", ncases, bad);
    return bad ? 1 : 0;
}
#endif
