// frames_main.cpp -- the container layer of the library (csrc/framing_*.cpp) under the host sanitizers, as a program of its own:
// tests/test_frames_build.py compiles the host side of the library's .cpp files with the address and undefined-behaviour sanitizers, links them with the plain device
// objects and runs this on the cases of tests/_frames_cases.py.  No device is needed: a header-stage case is answered before any
// launch, and swc_index_blocks never launches.
//
//   frames_main <case file>
// The file: u32 count, then per case  u32 kind (as swc_unarchive_many: 1 gzip, 2 zlib, 4 lz4, 5 bzip2, 6 xz), u32 header_stage,
// i32 expected status, u32 has_dictionary, i64 dictionary id (-1: none), u32 dictionary length, the dictionary, u32 name length, the
// name, u32 length, the archive.  Every archive is copied into a malloc block of exactly its length, so that a read one byte past
// the end is the sanitizer's to see.
// Exit status 0: every header-stage case gave its stated status through the single-shot call and through swc_unarchive_many, and
// every ref of every swc_index_blocks kind on every case lies inside the archive.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "swc_hip.h"

namespace {

struct Reader {
    std::vector<uint8_t> d;
    size_t p = 0;
    bool ok = true;
    void take(void* to, size_t n) {
        if (d.size() - p < n) { ok = false; memset(to, 0, n); return; }
        memcpy(to, d.data() + p, n);
        p += n;
    }
    uint32_t u32() { uint32_t v; take(&v, 4); return v; }
    int64_t i64() { int64_t v; take(&v, 8); return v; }
    std::vector<uint8_t> bytes() {
        const uint32_t n = u32();
        std::vector<uint8_t> v;
        if (d.size() - p < n) { ok = false; return v; }
        v.assign(d.begin() + (std::ptrdiff_t)p, d.begin() + (std::ptrdiff_t)(p + n));
        p += n;
        return v;
    }
};

// exactly `n` bytes on the heap (a block of one byte for n = 0: the calls take a pointer with a length of 0)
uint8_t* exact(const std::vector<uint8_t>& v) {
    uint8_t* p = static_cast<uint8_t*>(malloc(v.empty() ? 1 : v.size()));
    if (!p) abort();
    if (!v.empty()) memcpy(p, v.data(), v.size());
    return p;
}

bool known_status(int st) {
    return st == 0 || (st >= 101 && st <= 104) || (st >= 201 && st <= 210) || (st >= 301 && st <= 307) || (st >= 401 && st <= 404) ||
           (st >= 501 && st <= 504) || (st >= 601 && st <= 607) || (st >= 701 && st <= 705) || (st >= 801 && st <= 809) ||
           (st >= 851 && st <= 853) || (st >= 861 && st <= 865) || (st >= 900 && st <= 904);
}

int single_shot(uint32_t kind, const uint8_t* in, size_t len, const uint8_t* dict, size_t dict_len, int64_t dict_id) {
    uint8_t* out = nullptr;
    size_t out_len = 0, used = 0;
    int st;
    switch (kind) {
        case 1: st = swc_gzip_unarchive(in, len, &out, &out_len); break;
        case 2: st = swc_zlib_unarchive(in, len, &out, &out_len); break;
        case 4: st = swc_lz4_decompress(in, len, dict, dict_len, dict_id, &out, &out_len, &used); break;
        case 5: st = swc_bzip2_decompress(in, len, &out, &out_len, &used); break;
        case 6: st = swc_xz_unarchive(in, len, &out, &out_len); break;
        default: return -1;
    }
    swc_free(out);
    return st;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: frames_main <case file>\n"); return 2; }
    Reader r;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) r.d.insert(r.d.end(), buf, buf + n);
        fclose(f);
    }
    const uint32_t count = r.u32();
    int bad = 0;
    size_t headers = 0, refs_seen = 0;
    static const int kinds[] = {1, 3, 4, 5, 6, 7, 8, 9, 10};
    for (uint32_t c = 0; c < count && r.ok; c++) {
        const uint32_t kind = r.u32(), header_stage = r.u32();
        const int expected = (int)r.u32();
        const uint32_t has_dict = r.u32();
        const int64_t dict_id = r.i64();
        const std::vector<uint8_t> dict = r.bytes(), name_bytes = r.bytes(), data = r.bytes();
        if (!r.ok) break;
        const std::string name(name_bytes.begin(), name_bytes.end());
        uint8_t* in = exact(data);
        uint8_t* dp = has_dict ? exact(dict) : nullptr;
        const size_t len = data.size();
        if (header_stage) {
            headers++;
            const int st = single_shot(kind, in, len, dp, dict.size(), dict_id);
            if (st != expected) { bad++; fprintf(stderr, "%s: single-shot status %d, stated %d\n", name.c_str(), st, expected); }
            if (!has_dict) {   // (swc_unarchive_many takes no dictionary)
                const uint8_t* archives[1] = {in};
                const size_t lens[1] = {len};
                uint8_t* outs[1] = {nullptr};
                size_t out_lens[1] = {0};
                int32_t statuses[1] = {-1};
                const int rc = swc_unarchive_many((int)kind, archives, lens, 1, outs, out_lens, statuses);
                if (rc != 0 || statuses[0] != expected) { bad++; fprintf(stderr, "%s: swc_unarchive_many returned %d, status %d, stated %d\n", name.c_str(), rc, (int)statuses[0], expected); }
                if (rc == 0) swc_free(outs[0]);
            }
        }
        for (int k : kinds) {
            size_t n = 0;
            int st = swc_index_blocks(k, in, len, nullptr, 0, &n);
            if (!known_status(st)) { bad++; fprintf(stderr, "%s: swc_index_blocks kind %d returned %d\n", name.c_str(), k, st); continue; }
            std::vector<swc_block_ref> refs(n ? n : 1);
            size_t m = 0;
            st = swc_index_blocks(k, in, len, refs.data(), n, &m);
            if (!known_status(st) || m != n) { bad++; fprintf(stderr, "%s: swc_index_blocks kind %d returned %d with %zu refs after %zu\n", name.c_str(), k, st, m, n); continue; }
            const uint64_t limit = (k == 5 || k == 10) ? (uint64_t)len * 8 : (uint64_t)len;
            for (size_t i = 0; i < n; i++) {
                refs_seen++;
                if (refs[i].offset > limit || refs[i].comp_len > limit - refs[i].offset) {
                    bad++;
                    fprintf(stderr, "%s: kind %d ref %zu = (%llu, %llu) leaves the archive of %llu\n", name.c_str(), k, i,
                            (unsigned long long)refs[i].offset, (unsigned long long)refs[i].comp_len, (unsigned long long)limit);
                }
            }
        }
        free(in);
        free(dp);
    }
    if (!r.ok) { fprintf(stderr, "case file cut short\n"); return 2; }
    printf("%u cases, %zu at the header stage, %zu refs, %d mismatches\n", count, headers, refs_seen, bad);
    return bad ? 1 : 0;
}
