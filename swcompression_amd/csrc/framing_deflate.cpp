// framing_deflate.cpp -- host side of the Deflate family: single-shot Deflate, and the GZip / Zlib
// archive framing that stays on the host and feeds the batched HIP launch.
//   Deflate.decompress(data:)            reference Sources/Deflate/Deflate.swift:24-28
//   GzipArchive.unarchive/multiUnarchive reference Sources/GZip/GzipArchive.swift:38-100
//   GzipHeader.init(_:)                  reference Sources/GZip/GzipHeader.swift:68-199
//   ZlibArchive.unarchive                reference Sources/Zlib/ZlibArchive.swift:25-42
//   ZlibHeader.init(_:)                  reference Sources/Zlib/ZlibHeader.swift:47-92
#include <thread>
#include <system_error>
#include <new>
#include <algorithm>
#include <vector>
#include <atomic>
#include "host_util.h"
#include "framing.h"
#include "launch.h"
#include "bgzf_pack.h"
#include "gzip_scan.h"

namespace swc {

// ---- streams cut at their flush points ----------------------------------------------------------------------------------------
// An empty stored block -- what Z_FULL_FLUSH / Z_SYNC_FLUSH, pigz and this library's own segmented encoder (kCompressSegment below)
// put between the pieces of a stream -- ends with 00 00 FF FF on a byte boundary, and the next block starts on the next byte.  So a
// stream is CUT behind every such marker into units that decode in parallel (include/swc_hip.h: SWC_DEFLATE_OPEN,
// SWC_DEFLATE_JOINED), as long as no unit refers to bytes in front of itself.  The marker is only a guess -- the four bytes occur in
// stored data and in codes too -- which the decode checks (framing_runs.cpp: the verdict and the fallback); here the unit that ends
// the stream is the first that met a final block, and a unit that reaches back (Z_SYNC_FLUSH) fails in its unit.
// "deflate_units_linked" = 1: every unit but the first is SWC_DEFLATE_LINKED as well -- it shares the history of the units in front of
// it, which one wave copies as a chain (deflate_chain.h) -- so a unit that reaches back is no reason to fall back any more: default
// pigz and Z_SYNC_FLUSH streams decode as units.  The verdict is the same rule; a false marker or a broken stream still falls back.
// "deflate_unit_bytes": the least compressed size of a unit, 0 = never cut.  The default is 0 -- the host paths decode as they always
// did -- until tools/exp_deflate_units.py has shown on the device what cutting gains; callers opt in with the knob.
static std::atomic<size_t> g_deflate_unit_bytes{0};
void set_deflate_unit_bytes(int v) { g_deflate_unit_bytes = (size_t)v; }
size_t deflate_unit_bytes() { return g_deflate_unit_bytes.load(); }
static std::atomic<int> g_deflate_units_linked{0};
void set_deflate_units_linked(int v) { g_deflate_units_linked = v; }

// The units of one raw stream (swc_index_blocks kind 3): a cut behind every marker, cuts merged until every unit but the last
// holds at least unit_bytes, no cut at the very end.  Always at least one unit; aux = the bits of its job.
void deflate_unit_index(const uint8_t* in, size_t len, size_t unit_bytes, std::vector<BlockRef64>& out) {
    size_t start = 0;
    const uint32_t behind = SWC_DEFLATE_JOINED | (g_deflate_units_linked.load() ? SWC_DEFLATE_LINKED : 0);   // every unit but the first
    if (unit_bytes != 0 && len >= 4) {
        const uint8_t* p = in + 2;   // (the first 0xFF of a marker is at offset 2 or later)
        const uint8_t* const end = in + len;
        while (p < end) {
            p = static_cast<const uint8_t*>(memchr(p, 0xFF, (size_t)(end - p)));
            if (!p || p + 1 >= end) break;
            if (p[1] == 0xFF && p[-1] == 0 && p[-2] == 0) {
                const size_t cut = (size_t)(p - in) + 2;
                if (cut < len && cut - start >= unit_bytes) {
                    out.push_back({start, cut - start, 0, (uint32_t)(SWC_DEFLATE_OPEN | (out.empty() ? 0u : behind))});
                    start = cut;
                }
                p += 2;
            } else p++;
        }
    }
    out.push_back({start, len - start, 0, out.empty() ? 0u : behind});
}

// What Deflate adds to run_streams (framing.h: RunCodec).  The units of a run are a chain: the runner lays their outputs out back to
// back, copies the run out once as its head's output and leaves the verdict on the head (run_ok, run_used, run_bytes).
static void deflate_run_index(const HostUnit& st, size_t unit_bytes, std::vector<BlockRef64>& refs) {
    if (st.aux == 0) deflate_unit_index(st.in, st.in_len, unit_bytes, refs);
}
static void deflate_run_fill(const HostUnit& st, const std::vector<BlockRef64>& refs, HostUnit* run, const HostUnit* again, std::vector<uint8_t>&) {
    for (size_t k = 0; k < refs.size(); k++) {
        HostUnit& u = run[k];
        u.chain = true;
        u.sum_kind = st.sum_kind;
        if (again) {   // every unit has reported its exact size (phase 1 counts on past the capacity): once more with those
            u.cap_hint = (size_t)std::max<uint64_t>(std::min<uint64_t>(again[k].need, (uint64_t)u.in_len * 1032 + 64), 64);
            u.cap_exact = true;
            continue;
        }
        // room: six times the compressed size (the static blocks of this library's own encoder pack text 4.2 : 1; the runner's
        // four would send every such unit round again), never more than the whole stream is said to hold; a unit that needs
        // more says how much, and the run goes once more with exactly that
        u.cap_hint = std::max<size_t>(65536, u.in_len * 6 + 1024);
        if (st.cap_hint) u.cap_hint = std::min(u.cap_hint, std::max<size_t>(st.cap_hint, 64));
    }
    run[0].run_len = refs.size();
    run[0].dst = st.dst;
    run[0].dst_cap = st.dst_cap;
}
static bool deflate_run_lacked_room(const HostUnit* run) {   // (run_used == run_len: every unit ended open, none lacked room)
    return !run[0].run_ok && run[0].run_used < run[0].run_len && run[run[0].run_used].status == SWC_E_CAPACITY;
}
static bool deflate_run_verdict(HostUnit& st, const std::vector<BlockRef64>&, HostUnit* run, std::vector<uint8_t>&, size_t& last) {
    if (!run[0].run_ok) return false;
    last = run[0].run_used;
    st.out = std::move(run[0].out);
    st.in_dst = run[0].in_dst;
    st.out_size = run[0].run_bytes;
    return true;
}
const RunCodec& deflate_runs() {
    static const RunCodec c = {SWC_CODEC_DEFLATE, kStatDeflateUnitFallbacks, 1u << SWC_SUM_CRC32 | 1u << SWC_SUM_ADLER32, deflate_unit_bytes,
                               deflate_run_index, deflate_run_fill, deflate_run_lacked_room, deflate_run_verdict};
    return c;
}

void give(const std::vector<uint8_t>& src, uint8_t** out, size_t* out_len) {
    uint8_t* p = host_result(src.size());
    if (!p) throw std::bad_alloc();   // (host_result is malloc: the entry points' function-try-blocks turn this into SWC_E_DEVICE)
    const size_t n = src.size(), nt = std::min<size_t>(8, n >> 24);         // a thread per 16 MB: one core copies 10 GB/s
    if (nt >= 2) {
        std::vector<std::thread> th;
        const size_t per = (n / nt + 63) & ~(size_t)63;
        size_t done = 0;   // bytes whose copy a thread has taken
        try {
            for (size_t t = 0; t < nt; t++) {
                const size_t lo = std::min(n, t * per), hi = t + 1 == nt ? n : std::min(n, (t + 1) * per);
                th.emplace_back([=, &src] { if (hi > lo) memcpy(p + lo, src.data() + lo, hi - lo); });
                done = hi;
            }
        } catch (const std::system_error&) {}   // no more threads to be had: this one copies the rest
        if (done < n) memcpy(p + done, src.data() + done, n - done);
        for (auto& t : th) t.join();
    } else if (n) memcpy(p, src.data(), n);
    *out = p;
    *out_len = src.size();
}
void give_empty(uint8_t** out, size_t* out_len) {
    *out = host_result(0);
    *out_len = 0;
}
size_t* give_sizes(const std::vector<size_t>& v) {
    size_t* s = static_cast<size_t*>(malloc((v.size() ? v.size() : 1) * sizeof(size_t)));
    for (size_t i = 0; i < v.size(); i++) s[i] = v[i];
    return s;
}

// ---- GZip header (host) ------------------------------------------------------------------------
// Walks one member header starting at `pos`; on success `pos` is the first byte of the Deflate
// stream.  Error taxonomy follows GzipHeader.swift line by line; `trap` marks inputs on which the
// reference would read past the end of its reader (a Swift precondition failure).
int gzip_parse_header(const uint8_t* d, size_t n, size_t& pos, GzipHeaderInfo* info) {
    struct Cursor {
        const uint8_t* d; size_t n; size_t p; bool trap;
        size_t left() const { return n - p; }
        uint8_t u8() { if (p >= n) { trap = true; return 0; } return d[p++]; }
        uint32_t le16() { uint32_t a = u8(); uint32_t b = u8(); return a | (b << 8); }
    } c{d, n, pos, false};
    const size_t start = pos;
    if (c.left() < 10) return SWC_E_GZIP_WRONG_MAGIC;                  // GzipHeader.swift:70
    if (c.le16() != 0x8b1f) return SWC_E_GZIP_WRONG_MAGIC;             // :75
    if (c.u8() != 8) return SWC_E_GZIP_WRONG_COMPRESSION_METHOD;       // :81
    const uint32_t flags = c.u8();
    if (flags & 0xE0) return SWC_E_GZIP_WRONG_FLAGS;                   // :87
    c.p += 6;                                                          // MTIME, XFL, OS
    if (info) { info->bgzf_bsize = 0; }
    if (flags & 0x04) {                                                // FEXTRA :110-156
        if (c.left() < 2) return SWC_E_GZIP_WRONG_MAGIC;
        int64_t xlen = c.le16();
        if (!((int64_t)c.left() >= xlen && xlen >= 4)) return SWC_E_GZIP_WRONG_MAGIC;  // :123
        while (xlen > 0) {
            uint8_t si1 = c.u8();
            uint8_t si2 = c.u8();
            if (c.trap) return SWC_E_REF_TRAP;
            if (si2 == 0) return SWC_E_GZIP_WRONG_FLAGS;               // :131
            int64_t len = c.le16();
            if (c.trap) return SWC_E_REF_TRAP;
            xlen -= 4;
            if (xlen < len) return SWC_E_GZIP_WRONG_MAGIC;             // :145
            if ((int64_t)c.left() < len) return SWC_E_REF_TRAP;
            if (info && si1 == 'B' && si2 == 'C' && len == 2)           // BGZF: BSIZE = member size - 1
                info->bgzf_bsize = (uint32_t)c.d[c.p] | ((uint32_t)c.d[c.p + 1] << 8);
            c.p += (size_t)len;
            xlen -= len;
        }
    }
    for (uint32_t bit : {0x08u, 0x10u}) {                              // FNAME :158-172, FCOMMENT :174-188
        if (flags & bit) {
            for (;;) {
                if (c.p >= c.n) return SWC_E_GZIP_WRONG_MAGIC;
                if (c.d[c.p++] == 0) break;
            }
        }
    }
    if (flags & 0x02) {                                                // FHCRC :190-198
        if (c.left() < 2) return SWC_E_GZIP_WRONG_MAGIC;
        const size_t hend = c.p;
        uint32_t crc16 = c.le16();
        if ((swc_crc32(d + start, hend - start, 0) & 0xFFFF) != crc16) return SWC_E_GZIP_WRONG_HEADER_CRC;
    }
    if (c.trap) return SWC_E_REF_TRAP;
    pos = c.p;
    return SWC_OK;
}

// processMember (GzipArchive.swift:79-100) split in two around the device call.
int gzip_member_prepare(const uint8_t* d, size_t n, size_t pos, HostUnit& u) {
    if (n - pos < 20) return SWC_E_GZIP_WRONG_MAGIC;                   // :83 (members are byte aligned by construction)
    size_t p = pos;
    int st = gzip_parse_header(d, n, p, nullptr);
    if (st) return st;
    u = HostUnit();
    u.in = d + p;
    u.in_len = n - p;
    // ISIZE of a single-member archive is its last four bytes: a good capacity guess, never trusted.
    uint32_t isize = (uint32_t)d[n - 4] | (uint32_t)d[n - 3] << 8 | (uint32_t)d[n - 2] << 16 | (uint32_t)d[n - 1] << 24;
    if ((uint64_t)isize <= (uint64_t)u.in_len * 1100 + 4096) u.cap_hint = std::max<size_t>(isize, 64);
    return SWC_OK;
}
// `u` holds the decoded Deflate stream; `data_pos` = offset of the Deflate stream in `d`.
int gzip_member_finish(const uint8_t* d, size_t n, size_t data_pos, const HostUnit& u, size_t& next_pos, bool& crc_error) {
    crc_error = false;
    if (u.status) return u.status;                                     // DeflateError propagates
    size_t p = data_pos + u.in_consumed;                               // align() already applied by the engine
    if (n - p < 8) return SWC_E_GZIP_WRONG_MAGIC;                      // :91
    uint32_t crc = (uint32_t)d[p] | (uint32_t)d[p + 1] << 8 | (uint32_t)d[p + 2] << 16 | (uint32_t)d[p + 3] << 24;
    uint32_t isize = (uint32_t)d[p + 4] | (uint32_t)d[p + 5] << 8 | (uint32_t)d[p + 6] << 16 | (uint32_t)d[p + 7] << 24;
    if ((uint32_t)(u.size() & 0xFFFFFFFFu) != isize) return SWC_E_GZIP_WRONG_ISIZE;  // :95
    // :99 -- the CRC-32 the device computed behind the decode (HostUnit::sum_kind = 1), else here
    crc_error = (u.sum_valid && u.sum_kind == 1 ? (uint32_t)u.sum : swc_crc32(u.data(), u.size(), 0)) != crc;
    next_pos = p + 8;
    return SWC_OK;
}

// ZlibHeader.init (ZlibHeader.swift:47-92): returns offset of the Deflate stream in `pos`.
int zlib_parse_header(const uint8_t* d, size_t n, size_t& pos) {
    if (n < 2) return SWC_E_ZLIB_WRONG_COMPRESSION_METHOD;             // :49
    const uint32_t cmf = d[0], flg = d[1];
    if ((cmf & 0x0F) != 8) return SWC_E_ZLIB_WRONG_COMPRESSION_METHOD; // :57
    if ((cmf >> 4) > 7) return SWC_E_ZLIB_WRONG_COMPRESSION_INFO;      // :63
    if (((cmf << 8) + flg) % 31 != 0) return SWC_E_ZLIB_WRONG_FCHECK;  // :83
    size_t p = 2;
    if (flg & 0x20) {                                                  // FDICT: skip DICTID :87-90
        if (n - p < 4) return SWC_E_ZLIB_WRONG_FCHECK;
        p += 4;
    }
    pos = p;
    return SWC_OK;
}

}  // namespace swc

using namespace swc;

extern "C" {

int swc_deflate_decompress(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len, size_t* in_consumed) try {
    if (!out || !out_len || (in_len && !in)) return SWC_E_INVALID_ARGUMENT;
    HostUnit u;
    u.in = in; u.in_len = in_len;
    int st = run_one(SWC_CODEC_DEFLATE, u, kCut);
    if (st) { give_empty(out, out_len); return st; }
    if (in_consumed) *in_consumed = u.in_consumed;
    if (u.status) { give_empty(out, out_len); return u.status; }       // DeflateError cases carry no data
    give(u.out, out, out_len);
    return SWC_OK;
} catch (...) {   // std::bad_alloc / length_error from a size taken from the input: never through the C boundary
    if (out && out_len) give_empty(out, out_len);
    return SWC_E_DEVICE;
}

int swc_gzip_unarchive(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len) try {
    if (!out || !out_len || (in_len && !in)) return SWC_E_INVALID_ARGUMENT;
    HostUnit u;
    int st = gzip_member_prepare(in, in_len, 0, u);
    if (st) { give_empty(out, out_len); return st; }
    const size_t data_pos = (size_t)(u.in - in);
    u.sum_kind = 1;                                                    // CRC-32 on the device, behind the decode
    st = run_one(SWC_CODEC_DEFLATE, u, kCut);
    if (st) { give_empty(out, out_len); return st; }
    size_t next; bool crc_error;
    st = gzip_member_finish(in, in_len, data_pos, u, next, crc_error);
    if (st) { give_empty(out, out_len); return st; }
    give(u.out, out, out_len);                                         // wrongCRC carries the member (:44)
    return crc_error ? SWC_E_GZIP_WRONG_CRC : SWC_OK;
} catch (...) {   // std::bad_alloc / length_error from a size taken from the input: never through the C boundary
    if (out && out_len) give_empty(out, out_len);
    return SWC_E_DEVICE;
}

// BGZF (and any multi-member gzip whose members carry the 'BC' extra field): BSIZE = member size - 1 locates every member
// without decoding, so ALL members go to the device in one batch.  The result is used only if every member decoded cleanly
// from exactly the bytes its BSIZE assigns to it -- then the sequential walk of GzipArchive.multiUnarchive (:62-77) would have
// met the same members at the same offsets; anything else (a member without the field, a decode error, a stream that ends
// before or after its BSIZE, a CRC / ISIZE mismatch) falls back to that walk, which alone defines errors and partial results.
}  // extern "C"
namespace swc {
// Every member of a BGZF file: offset / length of its Deflate stream and its ISIZE.  False if a member lacks the field.
bool bgzf_index(const uint8_t* in, size_t in_len, std::vector<BlockRef64>& out) {
    size_t pos = 0;
    while (pos < in_len) {
        if (in_len - pos < 20) return false;
        size_t p = pos;
        GzipHeaderInfo info;
        if (gzip_parse_header(in, in_len, p, &info) != SWC_OK || info.bgzf_bsize == 0) return false;
        const size_t total = (size_t)info.bgzf_bsize + 1;
        if (total > in_len - pos || p - pos + 8 > total) return false;
        const uint8_t* t = in + pos + total - 8;
        const uint32_t isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        out.push_back({p, total - (p - pos) - 8, isize, 0});
        pos += total;
    }
    return true;
}
}  // namespace swc
extern "C" {
// On success *all_out is the malloc()ed concatenation of the members (the caller's result buffer: every member is copied
// from the staging buffer straight to its place in it, and its CRC-32 comes from the device).
static bool bgzf_multi(const uint8_t* in, size_t in_len, uint8_t** all_out, size_t* all_len, std::vector<size_t>& sz) {
    struct Member { size_t data_pos, data_len, trailer; };
    std::vector<Member> members;
    {
        std::vector<BlockRef64> refs;
        if (!bgzf_index(in, in_len, refs)) return false;
        for (const BlockRef64& r : refs) members.push_back({(size_t)r.offset, (size_t)r.comp_len, (size_t)(r.offset + r.comp_len)});
    }
    if (members.size() < 2) return false;
    std::vector<HostUnit> units(members.size());
    size_t total = 0;
    for (size_t k = 0; k < members.size(); k++) {
        const uint8_t* t = in + members[k].trailer;
        const uint32_t isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        units[k].in = in + members[k].data_pos;
        units[k].in_len = members[k].data_len;
        units[k].base = in;                 // one staged copy of the file, every member a sub-range of it
        units[k].base_len = in_len;
        units[k].sum_kind = 1;              // CRC-32 on the device
        if ((uint64_t)isize > (uint64_t)members[k].data_len * 1100 + 4096) return false;   // (not a size this member can have: the walk decides)
        units[k].cap_hint = std::max<size_t>(isize, 64);
        units[k].dst_cap = isize;
        total += isize;
    }
    // (ISIZE is a field of the file: the sum of them sizes ONE host buffer before a byte is decoded.  A file whose trailers claim
    // more than 64 x its own size -- or 64 MiB -- goes the sequential walk, which grows its result with the bytes it decodes.)
    if (total > std::max<size_t>((size_t)64 << 20, in_len * 64)) return false;
    uint8_t* all = host_result(total);
    if (!all) return false;
    {
        size_t o = 0;
        for (HostUnit& u : units) { u.dst = all + o; o += u.dst_cap; }
    }
    bool ok = run_units(SWC_CODEC_DEFLATE, units) == SWC_OK;
    for (size_t k = 0; ok && k < members.size(); k++) {
        const HostUnit& u = units[k];
        size_t next;
        bool crc_error;
        ok = u.status == SWC_OK && u.in_consumed == members[k].data_len && u.in_dst && u.out_size == u.dst_cap &&
             gzip_member_finish(in, in_len, members[k].data_pos, u, next, crc_error) == SWC_OK && !crc_error;
    }
    if (!ok) { host_result_free(all); return false; }
    for (const HostUnit& u : units) sz.push_back(u.out_size);
    *all_out = all;
    *all_len = total;
    return true;
}

// ---- plain members, found ahead of the walk (csrc/gzip_scan.h) ---------------------------------------------------
}  // extern "C"
namespace swc {
static std::atomic<int> g_gzip_member_scan{0};
void set_gzip_member_scan(int v) { g_gzip_member_scan = v; }

// The candidate rule of include/swc_hip.h (swc_index_blocks kind 9) on the host: what launch_gzip_index leaves on the device.
void gzip_member_index(const uint8_t* in, size_t len, std::vector<BlockRef64>& out) {
    if (len < 20) return;
    std::vector<size_t> starts;
    const uint8_t* const end = in + (len - 20) + 1;   // the first byte of a candidate lies in front of this
    for (const uint8_t* p = in; p < end; p++) {
        p = static_cast<const uint8_t*>(memchr(p, 0x1f, (size_t)(end - p)));
        if (!p) break;
        if (p[1] == 0x8b && p[2] == 0x08 && (p[3] & 0xE0) == 0) starts.push_back((size_t)(p - in));
    }
    for (size_t k = 0; k < starts.size(); k++) {
        const size_t p = starts[k], next = k + 1 < starts.size() ? starts[k + 1] : len;
        const uint32_t flags = in[p + 3];
        size_t q = p + 10;
        bool usable = true;
        if (flags & 0x04) {
            if (q + 2 > len) usable = false;
            else q += 2 + ((size_t)in[q] | (size_t)in[q + 1] << 8);
        }
        for (uint32_t bit : {0x08u, 0x10u}) {
            if (!usable || !(flags & bit)) continue;
            const size_t room = q < len ? std::min<size_t>(256, len - q) : 0;
            const uint8_t* z = room ? static_cast<const uint8_t*>(memchr(in + q, 0, room)) : nullptr;
            if (!z) usable = false;
            else q = (size_t)(z - in) + 1;
        }
        if (usable && (flags & 0x02)) q += 2;
        if (usable && q + 10 <= next) {
            const uint8_t* t = in + next - 4;
            out.push_back({q, next - q - 8, (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24, (uint32_t)(q - p), 0});
        } else out.push_back({p, 0, 0, 0, 1});
    }
}

// The file staged once, indexed on the device, and every plausible candidate decoded in ONE launch into `all` (laid out by the
// ISIZEs the candidates would have).  False: nothing to go by -- fewer than two candidates, more than a launch is worth, sizes no
// file of this length has, no device memory -- and the walk decodes every member itself.
struct ScanAhead {
    std::vector<BlockRef64> refs;      // the plausible usable candidates, by offset
    std::vector<HostUnit> units;       // units[k]: refs[k] decoded
    uint8_t* all = nullptr;
    size_t total = 0;
    ~ScanAhead() { host_result_free(all); }
};
static bool gzip_scan_ahead(const uint8_t* in, size_t in_len, ScanAhead& s) {
    if (in_len < 40 || !device_ready()) return false;
    hipStream_t stream = hipStreamPerThread;
    const uint64_t cap = std::max<uint64_t>(4096, in_len / 256);
    const size_t ws_bytes = swc_gzip_index_workspace_bytes(in_len, cap);
    DevBuf d_in(in_len + 16), d_refs(cap * sizeof(swc_block_ref) + sizeof(uint64_t)), d_ws(ws_bytes);
    if (!d_in.ok() || !d_refs.ok() || !d_ws.ok()) return false;
    uint8_t* up = pinned_stage(0, in_len);
    if (up) memcpy(up, in, in_len);
    uint64_t* d_n = reinterpret_cast<uint64_t*>(d_refs.u8() + cap * sizeof(swc_block_ref));
    swc_batch_opts opts = {-1, stream, 0, 0};
    uint64_t n = 0;
    const bool issued = hipMemcpyAsync(d_in.ptr(), up ? up : in, in_len, hipMemcpyHostToDevice, stream) == hipSuccess &&
                        swc_batch_gzip_index(d_in.u8(), in_len, reinterpret_cast<swc_block_ref*>(d_refs.ptr()), cap, d_n, d_ws.ptr(), ws_bytes, &opts) == SWC_OK &&
                        hipMemcpyAsync(&n, d_n, sizeof n, hipMemcpyDeviceToHost, stream) == hipSuccess;
    if (hipStreamSynchronize(stream) != hipSuccess || !issued) return false;   // (the staging buffer is the next call's again: nothing of this one in flight)
    stat_add(kStatLaunches, 1);
    if (n < 2 || n > cap) return false;   // (a file that dense in candidates is not worth a launch)
    std::vector<swc_block_ref> found((size_t)n);
    if (hipMemcpyAsync(found.data(), d_refs.ptr(), (size_t)n * sizeof(swc_block_ref), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) return false;
    for (const swc_block_ref& r : found) {
        // (a ref is checked against the file before it is used: nothing the device says is trusted with an address)
        if ((r.flags & 1) || r.comp_len < 2 || r.offset > in_len || r.comp_len > in_len - r.offset) continue;
        if (r.uncomp_len > r.comp_len * 1100 + 4096) continue;   // (not a size this member can have: the walk decides)
        s.refs.push_back({r.offset, r.comp_len, r.uncomp_len, r.aux, 0});
        s.total += (size_t)r.uncomp_len;
    }
    if (s.refs.empty() || s.total > std::max<size_t>((size_t)64 << 20, in_len * 64)) return false;
    s.all = host_result(s.total);
    if (!s.all) return false;
    s.units.resize(s.refs.size());
    size_t o = 0;
    for (size_t k = 0; k < s.refs.size(); k++) {
        HostUnit& u = s.units[k];
        u.in = in + s.refs[k].offset;
        u.in_len = (size_t)s.refs[k].comp_len;
        u.base = in;
        u.base_len = in_len;
        u.base_dev = d_in.u8();            // the copy the index read
        u.sum_kind = 1;                    // CRC-32 on the device
        u.cap_hint = std::max<size_t>((size_t)s.refs[k].uncomp_len, 64);
        u.cap_exact = true;                // (a member of another size is the walk's)
        u.dst = s.all + o;
        u.dst_cap = (size_t)s.refs[k].uncomp_len;
        o += u.dst_cap;
    }
    return run_units(SWC_CODEC_DEFLATE, s.units) == SWC_OK;
}
}  // namespace swc
extern "C" {

size_t swc_gzip_index_workspace_bytes(uint64_t len, uint64_t cap) { return (size_t)gzscan::plan(len, cap).bytes + 8; }   // (+ 8: cut from the first 8-byte boundary)

int swc_batch_gzip_index(const uint8_t* src, uint64_t len, swc_block_ref* refs, uint64_t cap, uint64_t* n, void* workspace, size_t workspace_bytes,
                         const swc_batch_opts* opts) try {
    static_assert(sizeof(swc_block_ref) == sizeof(gzscan::Ref) && offsetof(swc_block_ref, flags) == offsetof(gzscan::Ref, flags), "layout");
    if ((len && !src) || (cap && !refs) || !n || !workspace) return SWC_E_INVALID_ARGUMENT;
    if (workspace_bytes < swc_gzip_index_workspace_bytes(len, cap)) return SWC_E_NEED_WORKSPACE;
    if (!device_ready()) return SWC_E_DEVICE;
    if (opts && opts->device >= 0 && hipSetDevice(opts->device) != hipSuccess) return SWC_E_DEVICE;
    hipStream_t stream = opts ? static_cast<hipStream_t>(opts->stream) : nullptr;
    uint8_t* ws = reinterpret_cast<uint8_t*>(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
    const hipError_t e = launch_gzip_index(src, len, refs, cap, n, ws, stream);
    if (e == hipErrorInvalidValue) return SWC_E_INVALID_ARGUMENT;
    if (e != hipSuccess) return SWC_E_DEVICE;
    if (opts && opts->synchronize && hipStreamSynchronize(stream) != hipSuccess) return SWC_E_DEVICE;
    return SWC_OK;
} catch (...) {
    return SWC_E_DEVICE;
}

int swc_gzip_multi_unarchive(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len, size_t** sizes, size_t* n_members) try {
    if (!out || !out_len || !sizes || !n_members || (in_len && !in)) return SWC_E_INVALID_ARGUMENT;
    {
        std::vector<size_t> fsz;
        if (bgzf_multi(in, in_len, out, out_len, fsz)) {
            *sizes = give_sizes(fsz);
            *n_members = fsz.size();
            return SWC_OK;
        }
    }
    // Plain multi-member gzip has no compressed-size field: member k+1 can only be located after
    // member k has been inflated, so members are discovered sequentially here.
    // (BGZF and many-archive batches go through swc_unarchive_many, which launches them together.)
    // "gzip_member_scan" = 1: every place a member MAY start has been decoded ahead in one launch (gzip_scan_ahead); the walk below
    // still meets the members one by one, and takes a member from that launch where it is, byte for byte, what the walk's own decode
    // of it would have been checked to be.  Anything else is decoded here as ever: errors and partial results are this loop's.
    std::vector<uint8_t> all;
    std::vector<size_t> sz;
    ScanAhead ahead;
    const bool scanned = g_gzip_member_scan.load() != 0 && gzip_scan_ahead(in, in_len, ahead);
    size_t ui = 0, taken = 0, taken_bytes = 0;
    bool straight = scanned;   // the members so far are the units 0 .. taken - 1: ahead.all holds them as the result wants them
    auto leave_straight = [&] {
        if (straight) all.assign(ahead.all, ahead.all + taken_bytes);
        straight = false;
    };
    size_t pos = 0, walk_bound = (size_t)4 << 20;
    int st = SWC_OK;
    while (pos < in_len) {                                             // :66
        if (scanned) {
            auto start_of = [&](size_t k) { return (size_t)(ahead.refs[k].offset - ahead.refs[k].aux); };
            while (ui < ahead.refs.size() && start_of(ui) < pos) ui++;   // (candidates inside the member in front)
            if (ui < ahead.refs.size() && start_of(ui) == pos) {
                const HostUnit& v = ahead.units[ui];
                HostUnit tmp;
                size_t next = 0;
                bool bad_crc = false;
                if (gzip_member_prepare(in, in_len, pos, tmp) == SWC_OK && tmp.in == v.in && v.status == SWC_OK && v.in_consumed == v.in_len && v.in_dst &&
                    v.out_size == v.dst_cap && gzip_member_finish(in, in_len, (size_t)ahead.refs[ui].offset, v, next, bad_crc) == SWC_OK && !bad_crc) {
                    if (ui != taken) leave_straight();
                    if (straight) { taken++; taken_bytes += v.out_size; }
                    else all.insert(all.end(), v.dst, v.dst + v.out_size);
                    sz.push_back(v.out_size);
                    stat_add(kStatGzipScanMembers, 1);
                    pos = next;
                    ui++;
                    continue;
                }
            }
            leave_straight();
        }
        HostUnit u;
        st = gzip_member_prepare(in, in_len, pos, u);
        if (st) break;
        u.cap_hint = 0;                                                // ISIZE guess only valid for the last member
        const size_t data_pos = (size_t)(u.in - in);
        st = run_one_bounded(SWC_CODEC_DEFLATE, u, walk_bound, kCut);
        if (st) break;
        if (scanned) stat_add(kStatGzipScanWalked, 1);
        walk_bound = std::max<size_t>(walk_bound, 4 * u.in_consumed + 65536);   // the next member is probably of this size
        bool crc_error;
        st = gzip_member_finish(in, in_len, data_pos, u, pos, crc_error);
        if (st) break;
        all.insert(all.end(), u.out.begin(), u.out.end());
        sz.push_back(u.out.size());
        if (crc_error) { st = SWC_E_GZIP_WRONG_CRC; break; }           // :71-72 carries the members so far
    }
    if (st != SWC_OK && st != SWC_E_GZIP_WRONG_CRC) { straight = false; all.clear(); sz.clear(); }
    if (straight && taken == ahead.units.size()) {   // every unit was a member and nothing else was: the launch's buffer is the result
        *out = ahead.all;
        *out_len = ahead.total;
        ahead.all = nullptr;
    } else {
        leave_straight();
        give(all, out, out_len);
    }
    *sizes = give_sizes(sz);
    *n_members = sz.size();
    return st;
} catch (...) {   // std::bad_alloc / length_error from a size taken from the input: never through the C boundary
    if (out && out_len) give_empty(out, out_len);
    if (sizes) *sizes = nullptr;
    if (n_members) *n_members = 0;
    return SWC_E_DEVICE;
}

// Deflate.compress(data:) (Deflate+Compress.swift:22-46): a buffer of up to 1 MiB is one unit of SWC_CODEC_DEFLATE_COMPRESS -- one
// wavefront parses it, as the reference's one loop does (a wavefront's pace is about 5 MB/s: the engine's throughput is in the
// number of units of a launch).  The checksums of the archive writers (Adler-32, CRC-32 of the INPUT) are computed on the host by
// their callers.
// A LARGE buffer is cut into segments of kCompressSegment bytes, one wavefront each, all in one launch: every segment but the
// last comes back as a non-final static block followed by an empty stored block (so that it ends on a byte: job.aux bit 0,
// deflate_comp.h), and the segments one behind the other are one Deflate stream that the reference's decoder reads block by
// block (Deflate.swift:30-249).  What is given up: matches across a segment's start (under 0.1 % of the size at 256 KiB), and
// the reference's "one block" shape -- which SURVEY 8f-4 does not ask to keep.  Buffers of up to kCompressWhole bytes stay ONE
// block, as the reference writes them.
// `codec`: SWC_CODEC_DEFLATE_COMPRESS, or SWC_CODEC_DEFLATE_COMPRESS_DYNAMIC -- the same units and segments, every one a block with
// its own code tables where that is smaller (the _dynamic entry points below).
constexpr size_t kCompressWhole = (size_t)1 << 20, kCompressSegment = (size_t)256 << 10;
static int deflate_compress_unit(int codec, const uint8_t* data, size_t len, HostUnit& u) {
    if (len > kCompressWhole) {
        const size_t nseg = (len + kCompressSegment - 1) / kCompressSegment;
        std::vector<HostUnit> segs(nseg);
        for (size_t k = 0; k < nseg; k++) {
            HostUnit& s = segs[k];
            const size_t lo = k * kCompressSegment, n = std::min(kCompressSegment, len - lo);
            s.in = data + lo; s.in_len = n;
            s.base = data; s.base_len = len;            // one staged copy of the buffer, every segment a sub-range of it
            s.cap_hint = n + n / 8 + 32;
            s.cap_exact = true;
            s.aux = k + 1 < nseg ? 1 : 0;
        }
        const int st = run_units(codec, segs);
        if (st != SWC_OK) return st;
        size_t total = 0;
        for (const HostUnit& s : segs) { if (s.status != SWC_OK) { u.status = s.status; return SWC_OK; } total += s.size(); }
        u.out.clear();
        u.out.reserve(total);
        for (const HostUnit& s : segs) u.out.insert(u.out.end(), s.data(), s.data() + s.size());
        u.out_size = u.out.size();
        u.in_consumed = len;
        u.status = SWC_OK;
        return SWC_OK;
    }
    u.in = data; u.in_len = len;
    u.cap_hint = len + len / 8 + 16;
    u.cap_exact = true;
    return run_one(codec, u);
}
static int deflate_compress_impl(int codec, const uint8_t* data, size_t len, uint8_t** out, size_t* out_len) try {
    if (!out || !out_len || (len && !data)) return SWC_E_INVALID_ARGUMENT;
    HostUnit u;
    int st = deflate_compress_unit(codec, data, len, u);
    if (st == SWC_OK) st = u.status;
    if (st) { give_empty(out, out_len); return st; }
    give(u.out, out, out_len);
    return SWC_OK;
} catch (...) {
    if (out && out_len) give_empty(out, out_len);
    return SWC_E_DEVICE;
}
int swc_deflate_compress(const uint8_t* data, size_t len, uint8_t** out, size_t* out_len) {
    return deflate_compress_impl(SWC_CODEC_DEFLATE_COMPRESS, data, len, out, out_len);
}
int swc_deflate_compress_dynamic(const uint8_t* data, size_t len, uint8_t** out, size_t* out_len) {
    return deflate_compress_impl(SWC_CODEC_DEFLATE_COMPRESS_DYNAMIC, data, len, out, out_len);
}
// GzipArchive.archive(data:comment:fileName:writeHeaderCRC:isTextFile:osType:modificationTime:extraFields:) (GzipArchive.swift:126-240)
static int gzip_archive_impl(int codec, const uint8_t* data, size_t len, const uint8_t* comment, size_t comment_len, const uint8_t* file_name,
                             size_t file_name_len, int write_header_crc, int is_text_file, int os_type, int has_mtime, int64_t mtime,
                             const swc_gzip_extra_field* extra, size_t n_extra, uint8_t** out, size_t* out_len) try {
    if (!out || !out_len || (len && !data) || (comment_len && !comment) || (file_name_len && !file_name) || (n_extra && !extra))
        return SWC_E_INVALID_ARGUMENT;
    uint8_t flags = 0;
    if (comment) flags |= 1 << 4;                                      // :131-132
    if (file_name) flags |= 1 << 3;                                    // :144-145
    if (n_extra) flags |= 1 << 2;                                      // :157-159
    if (write_header_crc) flags |= 1 << 1;                             // :161-163
    if (is_text_file) flags |= 1 << 0;                                 // :165-167
    std::vector<uint8_t> z = {0x1f, 0x8b, 8, flags};                   // :180-184
    for (int i = 0; i < 4; i++) z.push_back(has_mtime ? (uint8_t)((uint64_t)mtime >> (8 * i)) : 0);   // :171-178, :185-187
    z.push_back(2);                                                    // :188 XFL: the slowest algorithm
    z.push_back((uint8_t)os_type);                                     // :169, :189
    if (n_extra) {                                                     // :191-209
        size_t xlen = 0;
        for (size_t k = 0; k < n_extra; k++) {
            if (extra[k].len && !extra[k].bytes) { give_empty(out, out_len); return SWC_E_INVALID_ARGUMENT; }
            xlen += 4 + extra[k].len;
        }
        if (xlen > 65535) { give_empty(out, out_len); return SWC_E_GZIP_CANNOT_ENCODE_ISO_LATIN1; }
        z.push_back((uint8_t)(xlen & 0xFF));
        z.push_back((uint8_t)(xlen >> 8));
        for (size_t k = 0; k < n_extra; k++) {
            z.push_back(extra[k].si1);
            z.push_back(extra[k].si2);
            z.push_back((uint8_t)(extra[k].len & 0xFF));
            z.push_back((uint8_t)((extra[k].len >> 8) & 0xFF));
            z.insert(z.end(), extra[k].bytes, extra[k].bytes + extra[k].len);
        }
    }
    auto terminated = [&](const uint8_t* p, size_t n) {                // :134-136, :147-149: a zero behind it unless it ends in one
        z.insert(z.end(), p, p + n);
        if (n == 0 || p[n - 1] != 0) z.push_back(0);
    };
    if (file_name) terminated(file_name, file_name_len);               // :213
    if (comment) terminated(comment, comment_len);                     // :214
    if (write_header_crc) {                                            // :216-221
        const uint32_t h = swc_crc32(z.data(), z.size(), 0);
        z.push_back((uint8_t)h);
        z.push_back((uint8_t)(h >> 8));
    }
    HostUnit u;
    int st = deflate_compress_unit(codec, data, len, u);               // :223
    if (st == SWC_OK) st = u.status;
    if (st) { give_empty(out, out_len); return st; }
    z.insert(z.end(), u.out.begin(), u.out.end());
    const uint32_t c = swc_crc32(data, len, 0);                        // :225-230
    for (int i = 0; i < 4; i++) z.push_back((uint8_t)(c >> (8 * i)));
    const uint64_t isize = (uint64_t)len % ((uint64_t)1 << 32);       // :232-237
    for (int i = 0; i < 4; i++) z.push_back((uint8_t)(isize >> (8 * i)));
    give(z, out, out_len);
    return SWC_OK;
} catch (...) {
    if (out && out_len) give_empty(out, out_len);
    return SWC_E_DEVICE;
}
int swc_gzip_archive(const uint8_t* data, size_t len, const uint8_t* comment, size_t comment_len, const uint8_t* file_name,
                     size_t file_name_len, int write_header_crc, int is_text_file, int os_type, int has_mtime, int64_t mtime,
                     const swc_gzip_extra_field* extra, size_t n_extra, uint8_t** out, size_t* out_len) {
    return gzip_archive_impl(SWC_CODEC_DEFLATE_COMPRESS, data, len, comment, comment_len, file_name, file_name_len, write_header_crc,
                             is_text_file, os_type, has_mtime, mtime, extra, n_extra, out, out_len);
}
int swc_gzip_archive_dynamic(const uint8_t* data, size_t len, const uint8_t* comment, size_t comment_len, const uint8_t* file_name,
                             size_t file_name_len, int write_header_crc, int is_text_file, int os_type, int has_mtime, int64_t mtime,
                             const swc_gzip_extra_field* extra, size_t n_extra, uint8_t** out, size_t* out_len) {
    return gzip_archive_impl(SWC_CODEC_DEFLATE_COMPRESS_DYNAMIC, data, len, comment, comment_len, file_name, file_name_len, write_header_crc,
                             is_text_file, os_type, has_mtime, mtime, extra, n_extra, out, out_len);
}
// ZlibArchive.archive(data:) (ZlibArchive.swift:54-70)
static int zlib_archive_impl(int codec, const uint8_t* data, size_t len, uint8_t** out, size_t* out_len) try {
    if (!out || !out_len || (len && !data)) return SWC_E_INVALID_ARGUMENT;
    HostUnit u;
    int st = deflate_compress_unit(codec, data, len, u);
    if (st == SWC_OK) st = u.status;
    if (st) { give_empty(out, out_len); return st; }
    std::vector<uint8_t> z;
    z.reserve(u.out.size() + 6);
    z.push_back(120);                                                  // :56 CM = 8, CINFO = 7
    z.push_back(218);                                                  // :57 slowest algorithm, no preset dictionary
    z.insert(z.end(), u.out.begin(), u.out.end());
    const uint32_t a = swc_adler32(data, len);                         // :62-66 big endian
    for (int i = 3; i >= 0; i--) z.push_back((uint8_t)(a >> (8 * i)));
    give(z, out, out_len);
    return SWC_OK;
} catch (...) {
    if (out && out_len) give_empty(out, out_len);
    return SWC_E_DEVICE;
}
int swc_zlib_archive(const uint8_t* data, size_t len, uint8_t** out, size_t* out_len) {
    return zlib_archive_impl(SWC_CODEC_DEFLATE_COMPRESS, data, len, out, out_len);
}
int swc_zlib_archive_dynamic(const uint8_t* data, size_t len, uint8_t** out, size_t* out_len) {
    return zlib_archive_impl(SWC_CODEC_DEFLATE_COMPRESS_DYNAMIC, data, len, out, out_len);
}

// ---- BGZF writer (an extension: the reference has none; csrc/bgzf_pack.h) ----------------------------------------
}  // extern "C"
namespace swc {
static std::atomic<size_t> g_bgzf_round{16384};   // members per round of the host entry: 1 GiB of input at the default block size
void set_bgzf_round_members(int v) { g_bgzf_round = (size_t)v; }
static bool bgzf_block_size(uint64_t& bs) {
    if (bs == 0) bs = bgzf::kMaxBlock;
    return bs <= bgzf::kMaxBlock;
}
// The device work of one call on `stream`, and its outcome (the call waits for it: the status is what it returns).
static int bgzf_run(const uint8_t* src, uint64_t len, uint64_t bs, int dynamic, uint8_t* dst, uint64_t dst_cap, uint64_t* total,
                    uint64_t* sizes, void* workspace, size_t workspace_bytes, bool eof, hipStream_t stream, uint64_t* total_host) {
    const bgzf::Plan p = bgzf::plan(len, bs);
    uint8_t* ws = reinterpret_cast<uint8_t*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    if (!workspace || workspace_bytes < p.bytes + (size_t)(ws - static_cast<uint8_t*>(workspace))) return SWC_E_NEED_WORKSPACE;
    const hipError_t e = launch_bgzf_archive(src, len, (uint32_t)bs, dynamic != 0, dst, dst_cap, total, sizes, ws, eof, stream);
    if (e == hipErrorInvalidValue) return SWC_E_INVALID_ARGUMENT;
    if (e != hipSuccess) return SWC_E_DEVICE;
    bgzf::Result res;
    if (hipMemcpyAsync(&res, ws + p.res, sizeof res, hipMemcpyDeviceToHost, stream) != hipSuccess) return SWC_E_DEVICE;
    if (hipStreamSynchronize(stream) != hipSuccess) return SWC_E_DEVICE;
    if (total_host) *total_host = res.total;
    return res.status;
}
}  // namespace swc
extern "C" {

size_t swc_bgzf_bound(size_t len, size_t block_size) {
    uint64_t bs = block_size;
    if (!bgzf_block_size(bs)) return 0;
    return len + 31 * (size_t)((len + bs - 1) / bs) + 28;
}
size_t swc_bgzf_workspace_bytes(size_t len, size_t block_size) {
    uint64_t bs = block_size;
    if (!bgzf_block_size(bs)) return 0;
    return (size_t)bgzf::plan(len, bs).bytes + 16;   // (+ 16: the areas are cut from the first 16-byte boundary of the workspace)
}

int swc_batch_bgzf_archive(const uint8_t* src, uint64_t len, uint64_t block_size, int dynamic, uint8_t* dst, uint64_t dst_cap,
                           uint64_t* total, uint64_t* member_sizes, void* workspace, size_t workspace_bytes, const swc_batch_opts* opts) try {
    if (!bgzf_block_size(block_size) || (len && !src) || !dst || !total) return SWC_E_INVALID_ARGUMENT;
    if (!device_ready()) return SWC_E_DEVICE;
    if (opts && opts->device >= 0 && hipSetDevice(opts->device) != hipSuccess) return SWC_E_DEVICE;
    hipStream_t stream = opts ? static_cast<hipStream_t>(opts->stream) : nullptr;
    return bgzf_run(src, len, block_size, dynamic, dst, dst_cap, total, member_sizes, workspace, workspace_bytes, true, stream, nullptr);
} catch (...) {
    return SWC_E_DEVICE;
}

int swc_bgzf_archive(const uint8_t* data, size_t len, size_t block_size, int dynamic, uint8_t** out, size_t* out_len, size_t** sizes,
                     size_t* n_members) try {
    if (sizes) *sizes = nullptr;
    if (n_members) *n_members = 0;
    uint64_t bs = block_size;
    if (!out || !out_len) return SWC_E_INVALID_ARGUMENT;
    if ((len && !data) || !bgzf_block_size(bs)) { give_empty(out, out_len); return SWC_E_INVALID_ARGUMENT; }
    if (!device_ready()) { give_empty(out, out_len); return SWC_E_DEVICE; }
    hipStream_t stream = hipStreamPerThread;
    const size_t n = (size_t)((len + bs - 1) / bs), per = std::max<size_t>(1, g_bgzf_round.load());
    // the input once; per round: the packed bytes of up to `per` members, their sizes, the workspace
    const size_t round_len = (size_t)std::min<uint64_t>(len, (uint64_t)per * bs), round_n = std::min(n, per);
    const size_t dst_cap = swc_bgzf_bound(round_len, bs), ws_bytes = swc_bgzf_workspace_bytes(round_len, bs);
    DevBuf d_src(len + 16), d_dst(dst_cap + 16), d_meta((round_n + 2) * sizeof(uint64_t)), d_ws(ws_bytes);
    if (!d_src.ok() || !d_dst.ok() || !d_meta.ok() || !d_ws.ok()) { give_empty(out, out_len); return SWC_E_DEVICE; }
    if (len && hipMemcpyAsync(d_src.ptr(), data, len, hipMemcpyHostToDevice, stream) != hipSuccess) { give_empty(out, out_len); return SWC_E_DEVICE; }
    std::vector<size_t> msz;
    std::vector<uint64_t> round_sizes(round_n + 1);
    msz.reserve(n + 1);
    uint8_t* res = host_result(swc_bgzf_bound(len, bs));   // (nothing below throws: the vectors have their room)
    if (!res) throw std::bad_alloc();
    uint64_t* d_total = reinterpret_cast<uint64_t*>(d_meta.ptr());
    size_t pos = 0, done = 0;
    int st = SWC_OK;
    do {
        const size_t m = std::min(per, n - done), lo = done * (size_t)bs, rl = std::min(len - lo, m * (size_t)bs);
        const bool last = done + m == n;
        uint64_t total = 0;
        st = bgzf_run(d_src.u8() + lo, rl, bs, dynamic, d_dst.u8(), dst_cap, d_total, d_total + 1, d_ws.ptr(), ws_bytes, last, stream, &total);
        if (st != SWC_OK) break;
        // the round's bytes straight to their place in the result, its sizes behind the others'
        const size_t cnt = m + (last ? 1 : 0);
        if (hipMemcpyAsync(res + pos, d_dst.ptr(), total, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(round_sizes.data(), d_total + 1, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) { st = SWC_E_DEVICE; break; }
        for (size_t k = 0; k < cnt; k++) msz.push_back((size_t)round_sizes[k]);
        pos += (size_t)total;
        done += m;
        stat_add(kStatLaunches, 1);
        stat_add(kStatUnits, (long long)m);
    } while (done < n);
    if (st != SWC_OK) { host_result_free(res); give_empty(out, out_len); return st; }
    *out = res;
    *out_len = pos;
    if (sizes) *sizes = give_sizes(msz);
    if (n_members) *n_members = msz.size();
    return SWC_OK;
} catch (...) {
    if (out && out_len) give_empty(out, out_len);
    return SWC_E_DEVICE;
}

int swc_zlib_unarchive(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len) try {
    if (!out || !out_len || (in_len && !in)) return SWC_E_INVALID_ARGUMENT;
    size_t p = 0;
    int st = zlib_parse_header(in, in_len, p);
    if (st) { give_empty(out, out_len); return st; }
    HostUnit u;
    u.in = in + p; u.in_len = in_len - p;
    u.sum_kind = 2;                                                    // Adler-32 on the device, behind the decode
    st = run_one(SWC_CODEC_DEFLATE, u, kCut);
    if (st) { give_empty(out, out_len); return st; }
    if (u.status) { give_empty(out, out_len); return u.status; }
    size_t q = p + u.in_consumed;
    give(u.out, out, out_len);                                         // wrongAdler32 carries the data (:34,39)
    if (in_len - q < 4) return SWC_E_ZLIB_WRONG_ADLER32;
    uint32_t stored = (uint32_t)in[q] << 24 | (uint32_t)in[q + 1] << 16 | (uint32_t)in[q + 2] << 8 | in[q + 3];
    return (u.sum_valid ? (uint32_t)u.sum : swc_adler32(u.out.data(), u.out.size())) == stored ? SWC_OK : SWC_E_ZLIB_WRONG_ADLER32;
} catch (...) {   // std::bad_alloc / length_error from a size taken from the input: never through the C boundary
    if (out && out_len) give_empty(out, out_len);
    return SWC_E_DEVICE;
}

}  // extern "C"
