// sha256_lane.h -- SHA-256 (FIPS 180-4) of one byte range by ONE lane: the block check of an .xz file written with
// --check=sha256 (reference Sources/Common/Sha256.swift:28-142, checked at Sources/XZ/XZArchive.swift:106-121).
//
// The 64 rounds of a block are one dependent chain and two blocks of a message cannot be combined, so a message is not cut:
// every lane of a wave hashes a message of its own, and the throughput of a launch is the number of its jobs.  No cross-lane step,
// no LDS.  The rounds are written out one by one with their constants as literals: the eight working variables rotate by their
// names, the sixteen message words are a ring of registers that every index addresses at compile time.
//
// ONE loop takes a message through all its blocks, padding included: an iteration either loads a whole 64-byte block (four 16-byte
// loads at the block's own address, whatever its alignment) or builds a block of the tail -- whole dwords, then single bytes, the
// 0x80 marker, zeros, the bit length in the last block -- and then runs the one copy of the rounds.  Lanes of a wave whose messages
// differ in length therefore share iterations: a short message's padding block runs beside a long message's data block, and the
// wave lasts as long as its longest message.  No byte outside p[0 .. len) is read; len == 0 reads nothing (p may be null).
#ifndef SWC_SHA256_LANE_H
#define SWC_SHA256_LANE_H

#include "swc_common.h"

namespace swc {
namespace sha {

SWC_HD uint32_t rotr(uint32_t x, uint32_t n) { return funnel32(x, x, n); }                    // v_alignbit_b32
SWC_HD uint32_t big0(uint32_t x) { return rotr(x, 2) ^ rotr(x, 13) ^ rotr(x, 22); }
SWC_HD uint32_t big1(uint32_t x) { return rotr(x, 6) ^ rotr(x, 11) ^ rotr(x, 25); }
SWC_HD uint32_t small0(uint32_t x) { return rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3); }
SWC_HD uint32_t small1(uint32_t x) { return rotr(x, 17) ^ rotr(x, 19) ^ (x >> 10); }
SWC_HD uint32_t ch(uint32_t e, uint32_t f, uint32_t g) { return bfi32(e, f, g); }             // (e & f) | (~e & g)
SWC_HD uint32_t maj(uint32_t a, uint32_t b, uint32_t c) { return bfi32(a ^ b, c, a); }        // where a and b differ c decides
SWC_HD uint32_t be32(uint32_t x) { return __builtin_bswap32(x); }                             // v_perm_b32

// round I with the variables in this order, constant K: words 16 and up are made in the ring just before they are used
#define SWC_SHA256_ROUND(I, a, b, c, d, e, f, g, h, K)                                                                     \
    {                                                                                                                      \
        if ((I) >= 16) w[(I) & 15] += small0(w[((I) + 1) & 15]) + w[((I) + 9) & 15] + small1(w[((I) + 14) & 15]);           \
        const uint32_t t1 = h + big1(e) + ch(e, f, g) + (K) + w[(I) & 15];                                                 \
        const uint32_t t2 = big0(a) + maj(a, b, c);                                                                        \
        d += t1;                                                                                                           \
        h = t1 + t2;                                                                                                       \
    }
// eight rounds bring every variable back to its name
#define SWC_SHA256_ROUNDS8(I, K0, K1, K2, K3, K4, K5, K6, K7)                                                              \
    SWC_SHA256_ROUND((I) + 0, a, b, c, d, e, f, g, h, K0)                                                                  \
    SWC_SHA256_ROUND((I) + 1, h, a, b, c, d, e, f, g, K1)                                                                  \
    SWC_SHA256_ROUND((I) + 2, g, h, a, b, c, d, e, f, K2)                                                                  \
    SWC_SHA256_ROUND((I) + 3, f, g, h, a, b, c, d, e, K3)                                                                  \
    SWC_SHA256_ROUND((I) + 4, e, f, g, h, a, b, c, d, K4)                                                                  \
    SWC_SHA256_ROUND((I) + 5, d, e, f, g, h, a, b, c, K5)                                                                  \
    SWC_SHA256_ROUND((I) + 6, c, d, e, f, g, h, a, b, K6)                                                                  \
    SWC_SHA256_ROUND((I) + 7, b, c, d, e, f, g, h, a, K7)

// one block: w = its sixteen big-endian words (used up), s = the state
SWC_D void sha256_block(uint32_t (&s)[8], uint32_t (&w)[16]) {
    uint32_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
    SWC_SHA256_ROUNDS8(0, 0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u)
    SWC_SHA256_ROUNDS8(8, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u)
    SWC_SHA256_ROUNDS8(16, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau)
    SWC_SHA256_ROUNDS8(24, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u)
    SWC_SHA256_ROUNDS8(32, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u)
    SWC_SHA256_ROUNDS8(40, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u)
    SWC_SHA256_ROUNDS8(48, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u)
    SWC_SHA256_ROUNDS8(56, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u)
    s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e; s[5] += f; s[6] += g; s[7] += h;
}
#undef SWC_SHA256_ROUNDS8
#undef SWC_SHA256_ROUND

// h = SHA-256 of p[0 .. len) as eight words (the digest is their big-endian bytes)
SWC_D void sha256_lane(gcptr p, uint64_t len, uint32_t (&h)[8]) {
    h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
    const uint64_t blocks = (len + 8) / 64 + 1;   // the marker and the eight length bytes make one block more where len % 64 >= 56
    for (uint64_t b = 0; b < blocks; b++) {
        const uint64_t off = b * 64;
        uint32_t w[16];
        if (off + 64 <= len) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const u128_any v = load_u128(p + off + 16 * q);
                w[4 * q] = be32(v.x); w[4 * q + 1] = be32(v.y); w[4 * q + 2] = be32(v.z); w[4 * q + 3] = be32(v.w);
            }
        } else {
            // the tail: the words that lie inside the message whole, the word that takes the marker (with up to three bytes of the
            // message in front of it), zeros; behind a marker that fell into the block before (off > len) nothing but zeros
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint64_t pos = off + 4 * (uint64_t)i;
                uint32_t v = 0;
                if (pos + 4 <= len) {
                    v = be32(load_u32(p + pos));
                } else if (pos <= len) {
                    const uint32_t r = (uint32_t)(len - pos);
                    if (r > 0) v |= (uint32_t)p[pos] << 24;
                    if (r > 1) v |= (uint32_t)p[pos + 1] << 16;
                    if (r > 2) v |= (uint32_t)p[pos + 2] << 8;
                    v |= 0x80000000u >> (8 * r);
                }
                w[i] = v;
            }
            if (b + 1 == blocks) { w[14] = (uint32_t)(len >> 29); w[15] = (uint32_t)(len << 3); }   // the length in bits
        }
        sha256_block(h, w);
    }
}

}  // namespace sha
}  // namespace swc
#endif
