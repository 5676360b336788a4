// bgzf_pack.h -- the BGZF writer's own part of the device work: the job set-up, the offsets of the members and the pack.
//
// A BGZF file (SAM/BAM specification 4.1) is a sequence of gzip members of at most 64 KiB each, every one with the extra field
// 'BC' that holds BSIZE = member size - 1, closed by an empty member of 28 fixed bytes.  The input is cut into chunks of
// `block_size` bytes; the chunks are compressed by the Deflate encoder (deflate_comp.h, ONE launch of codec 8 or 9 over all of
// them, every stream into its own 4-byte aligned SLOT of the workspace) and their CRC-32 comes from the wave CRC (crc32_wave.h,
// over a second job list that describes the chunks).  What is left is here:
//   setup_jobs    fills the two job lists (a thread per member);
//   scan_members  one wavefront walks the members 64 at a time: the exclusive 64-bit prefix sum of the member sizes 26 + s, the
//                 sizes themselves, the total, the first error by member index, and the decision whether anything is written at
//                 all (Result::status: an error of a compress job, or SWC_E_CAPACITY when the total exceeds the room);
//   pack_wave     one wavefront per member lays it out at its offset: 18 header bytes, the s stream bytes from the slot, CRC-32
//                 and ISIZE; one more wavefront writes the end-of-file member.
//
// The pack and its borders.  A member starts wherever the one in front ended, so the 16-byte destination chunk at either end of
// a member is shared with a neighbour that ANOTHER wave writes at the same time: nothing may be stored there but the member's own
// bytes, and a read-modify-write of a full chunk would lose the neighbour's.  So a member is three parts:
//   head      the header and the stream bytes in front of the first 16-byte boundary of the destination (at most 33 bytes),
//   interior  the destination chunks that lie wholly inside the stream: an aligned 16-byte store each, assembled from a 16-byte
//             and a 4-byte load at the 4-byte aligned source address below the chunk's and four v_alignbyte_b32 (the idiom of
//             lz_copy.h; source and destination advance together, so the shift is one value per member),
//   tail      the stream bytes behind the last whole chunk and the trailer (at most 23 bytes),
// and head and tail go out as byte stores, a byte per lane, under the exec mask.  A member without an interior chunk (fewer than
// 31 stream bytes) is all head: at most 56 bytes.
// No LDS, no cross-lane step in the pack; the scan's are the wrappers of simt.h.
#ifndef SWC_BGZF_PACK_H
#define SWC_BGZF_PACK_H

#include "swc_common.h"
#include "simt.h"

namespace swc {
namespace bgzf {

constexpr uint32_t kHeader = 18, kTrailer = 8, kOverhead = kHeader + kTrailer, kEofBytes = 28;
constexpr uint32_t kMaxBlock = 65280;     // 0xFF00, what bgzip cuts: BSIZE then fits 16 bits whatever the chunk holds
constexpr uint64_t kHead0 = 0x0000000004088b1full;   // 1f 8b 08 04 | MTIME
constexpr uint64_t kHead1 = 0x000243420006ff00ull;   // XFL 00, OS ff, XLEN 6, 'B' 'C', SLEN 2
// the end-of-file member: the header with BSIZE 27, an empty static block (03 00), CRC-32 0, ISIZE 0
constexpr uint64_t kEof2 = 0x000000000003001bull, kEof3 = 0ull;

// What the scan leaves for the pack and for the host
struct Result {
    uint64_t total;     // bytes of the file (needed, when status is SWC_E_CAPACITY)
    int32_t status;     // SWC_OK: the pack writes; anything else: nothing is written
    uint32_t pad;
    uint64_t bad;       // member whose compress job reported `status`
};

// room of a member's slot (the job contract of codecs 8 and 9: out_cap >= n + n / 8 + 32, out 4-byte aligned)
SWC_HD uint64_t slot_cap(uint64_t chunk) { return (chunk + chunk / 8 + 32 + 3) & ~(uint64_t)3; }

// The workspace of one call, cut from a 16-byte aligned base: [compress jobs | chunk jobs | CRCs | offsets (n + 1) | Result | slots]
struct Plan {
    uint64_t n, stride, cjobs, kjobs, crcs, offs, res, slots, bytes;
};
SWC_HD Plan plan(uint64_t len, uint64_t bs) {
    Plan p;
    auto up = [](uint64_t v) { return (v + 15) & ~(uint64_t)15; };
    p.n = (len + bs - 1) / bs;
    p.stride = up(slot_cap(len < bs ? len : bs));
    p.cjobs = 0;
    p.kjobs = p.cjobs + up(p.n * sizeof(Job));
    p.crcs = p.kjobs + up(p.n * sizeof(Job));
    p.offs = p.crcs + up(p.n * sizeof(uint32_t));
    p.res = p.offs + up((p.n + 1) * sizeof(uint64_t));
    p.slots = p.res + up(sizeof(Result));
    p.bytes = p.slots + p.n * p.stride;
    return p;
}

// ---- job set-up: thread g * N + t fills member i of both lists ----------------------------------------------------------------
// cj: the compress job of the chunk (out = its slot); kj: the chunk itself as a job's OUTPUT, which is what launch_crc32 sums.
template <int N>
SWC_D void setup_jobs(uint32_t g, const uint8_t* src, uint64_t len, uint32_t bs, uint64_t n, Job* cj, Job* kj, uint8_t* slots, uint64_t stride) {
    SIMT_BEGIN(t, N)
        const uint64_t i = (uint64_t)g * N + (uint32_t)t;
        if (i < n) {
            const uint64_t lo = i * bs, c = len - lo < bs ? len - lo : (uint64_t)bs;
            Job j;
            j.in = src + lo; j.in_len = c;
            j.out = slots + i * stride; j.out_cap = slot_cap(c);
            j.out_len = 0; j.in_consumed = 0;
            j.status = SWC_E_DEVICE; j.aux = 0;   // aux 0: a final block, the stream of a member
            j.dict = nullptr; j.dict_len = 0;
            cj[i] = j;
            j.in = nullptr; j.in_len = 0;
            j.out = const_cast<uint8_t*>(src + lo); j.out_cap = c; j.out_len = c;
            j.status = SWC_OK;
            kj[i] = j;
        }
    SIMT_END
}

// ---- offsets: ONE wavefront, 64 members per step ---------------------------------------------------------------------------------
// offs[i] = sum of the sizes of the members in front of i (offs[n]: of all of them), sizes[i] = 26 + s_i (sizes may be null; with
// `eof`, sizes[n] = 28), *total and res->total = offs[n] (+ 28 with `eof`).  A step's sum stays below 2^32 (64 x 65,311); the running
// sum is 64 bits.
template <int N>
SWC_D void scan_members(const Job* cj, uint64_t n, uint64_t* offs, uint64_t* sizes, uint64_t* total, Result* res, uint64_t dst_cap, bool eof) {
    using namespace simt;
    static_assert(N == kWave, "one wavefront");
    uint64_t run = 0, bad = 0;
    int32_t status = SWC_OK;
    for (uint64_t base = 0; base < n; base += N) {
        PT<uint32_t, N> sz, incl, st;
        PT<bool, N> err;
        SIMT_BEGIN(t, N)
            const uint64_t i = base + (uint32_t)t;
            const int32_t s = i < n ? cj[i].status : (int32_t)SWC_OK;
            st[t] = (uint32_t)s;
            err[t] = s != SWC_OK;
            sz[t] = i < n && s == SWC_OK ? kOverhead + (uint32_t)cj[i].out_len : 0u;
            incl[t] = sz[t];
        SIMT_END
        wave_scan_incl(incl);
        SIMT_BEGIN(t, N)
            const uint64_t i = base + (uint32_t)t;
            if (i < n) {
                offs[i] = run + incl[t] - sz[t];
                if (sizes) sizes[i] = sz[t];
            }
        SIMT_END
        const uint64_t m = wave_ballot(err);
        if (status == SWC_OK && m != 0) {   // the first error by member index
            const int lane = ctz64(m);
            status = (int32_t)wave_read(st, lane);
            bad = base + (uint32_t)lane;
        }
        run += wave_read(incl, N - 1);
    }
    const uint64_t all = run + (eof ? kEofBytes : 0u);
    if (status == SWC_OK && all > dst_cap) status = SWC_E_CAPACITY;
    SIMT_BEGIN(t, N)
        if (t == 0) {
            offs[n] = run;
            if (sizes && eof) sizes[n] = kEofBytes;
            *total = all;
            res->total = all;
            res->status = status;
            res->pad = 0;
            res->bad = bad;
        }
    SIMT_END
}

// ---- pack -----------------------------------------------------------------------------------------------------------------------
struct __attribute__((packed, aligned(4), may_alias)) q128a4 { uint32_t x, y, z, w; };
struct __attribute__((aligned(16), may_alias)) q128a16 { uint32_t x, y, z, w; };

// byte q of a member whose stream of s bytes lies at `slot` (q < 26 + s); only the head and the tail are read this way
SWC_D uint32_t member_byte(uint32_t q, gcptr slot, uint32_t s, uint32_t bsize, uint64_t trailer) {
    if (q < 8u) return (uint32_t)(kHead0 >> (8u * q)) & 0xFFu;
    if (q < 16u) return (uint32_t)(kHead1 >> (8u * (q - 8u))) & 0xFFu;
    if (q < kHeader) return (bsize >> (8u * (q - 16u))) & 0xFFu;
    if (q < kHeader + s) return slot[q - kHeader];
    return (uint32_t)(trailer >> (8u * (q - kHeader - s))) & 0xFFu;
}

// One member by the 64 lanes of a wave: d = where it begins (any alignment), slot = its stream (4-byte aligned, s bytes, at least
// 4 readable bytes behind them: the slot's slack is 27 and more).  Writes d[0 .. 26 + s) and not a byte outside.
template <int N>
SWC_D void pack_member(gptr d, gcptr slot, uint32_t s, uint32_t crc, uint32_t isize) {
    static_assert(N >= 64, "head and tail are a byte per lane: up to 56 bytes");
    const uint32_t len = kOverhead + s, bsize = len - 1u;
    const uint64_t trailer = (uint64_t)crc | (uint64_t)isize << 32;
    const uint32_t fa = (uint32_t)(0u - ((uint32_t)(uintptr_t)d + kHeader)) & 15u;   // stream bytes in front of the first boundary
    const uint32_t chunks = s >= fa + 16u ? (s - fa) >> 4 : 0u;
    const uint32_t head = chunks ? kHeader + fa : len;
    const uint32_t tail0 = head + (chunks << 4), tail = len - tail0;
    const uint32_t r = fa & 3u;                 // the chunk's source against the aligned dword below it: one value per member
    gcptr a0 = slot + (fa - r);                 // 4-byte aligned
    gptr d0 = d + head;                         // 16-byte aligned when there is a chunk
    SIMT_BEGIN(t, N)
        const uint32_t u = (uint32_t)t;
        if (u < head) d[u] = (uint8_t)member_byte(u, slot, s, bsize, trailer);
        if (u < tail) d[tail0 + u] = (uint8_t)member_byte(tail0 + u, slot, s, bsize, trailer);
        auto lo4 = [a0](uint32_t k) { return *(const SWC_AS_GLOBAL q128a4*)(a0 + ((size_t)k << 4)); };
        auto hi1 = [a0](uint32_t k) { return *(const SWC_AS_GLOBAL uint32_t*)(a0 + ((size_t)k << 4) + 16); };
        auto put = [d0, r](uint32_t k, const q128a4& lo, uint32_t hi) {
            q128a16 v;
            v.x = alignbyte32(lo.y, lo.x, r);
            v.y = alignbyte32(lo.z, lo.y, r);
            v.z = alignbyte32(lo.w, lo.z, r);
            v.w = alignbyte32(hi, lo.w, r);
            *(SWC_AS_GLOBAL q128a16*)(d0 + ((size_t)k << 4)) = v;
        };
        uint32_t k = u;
        for (; k + (uint32_t)N < chunks; k += 2u * (uint32_t)N) {   // two chunks per lane in flight: the loads of both before either store
            const q128a4 la = lo4(k), lb = lo4(k + (uint32_t)N);
            const uint32_t ha = hi1(k), hb = hi1(k + (uint32_t)N);
            put(k, la, ha);
            put(k + (uint32_t)N, lb, hb);
        }
        if (k < chunks) put(k, lo4(k), hi1(k));
    SIMT_END
}

// Wave i of n (+ 1 with `eof`): member i, or -- i == n -- the end-of-file member.  Nothing is written unless the scan said so.
template <int N>
SWC_D void pack_wave(uint64_t i, uint64_t n, const Job* cj, const Job* kj, const uint32_t* crcs, const uint64_t* offs, const Result* res,
                     uint8_t* dst, bool eof) {
    if (res->status != SWC_OK) return;
    gptr d = (gptr)dst + offs[i < n ? i : n];
    if (i < n) {
        const uint32_t s = simt::uniform((uint32_t)cj[i].out_len);
        pack_member<N>(d, (gcptr)cj[i].out, s, simt::uniform(crcs[i]), simt::uniform((uint32_t)kj[i].out_len));
    } else if (i == n && eof) {
        SIMT_BEGIN(t, N)
            const uint32_t u = (uint32_t)t;
            if (u < kEofBytes) {
                const uint64_t w = u < 8u ? kHead0 : u < 16u ? kHead1 : u < 24u ? kEof2 : kEof3;
                d[u] = (uint8_t)(w >> (8u * (u & 7u)));
            }
        SIMT_END
    }
}

}  // namespace bgzf
}  // namespace swc
#endif
