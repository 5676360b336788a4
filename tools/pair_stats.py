#!/usr/bin/env python3
"""How many matches of the benchmark's text would be ONE table step: a length code, its extra bits and the distance code behind it
inside the 10 index bits of the direct lit/len table (csrc/inflate_sync.h, PAIR entries).  Pure Python, no GPU: six
corpus.p_text(65536, seed) members, seeds 2..7, zlib level 6, raw Deflate, parsed code by code.  A counting aid, not a decoder:
it keeps no output and checks nothing.

    python tools/pair_stats.py [--payload text|mix]
"""
import argparse
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swcompression_amd import corpus  # noqa: E402

LIT_BITS, PAIR_LEN_MAX = 10, 127
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_BITS = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BITS = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class Bits:
    def __init__(self, data):
        self.v, self.p = int.from_bytes(data, "little"), 0

    def take(self, n):
        x = (self.v >> self.p) & ((1 << n) - 1)
        self.p += n
        return x


def decoder(lengths):
    """{(length, code read MSB first): symbol}"""
    code, table = 0, {}
    for n in range(1, 16):
        for s, l in enumerate(lengths):
            if l == n:
                table[(n, code)] = s
                code += 1
        code <<= 1
    return table


def symbol(b, table):
    code = 0
    for n in range(1, 16):
        code = (code << 1) | b.take(1)
        if (n, code) in table:
            return table[(n, code)], n
    raise ValueError("no code")


def count(stream, c):
    b = Bits(stream)
    final = 0
    while not final:
        final, kind = b.take(1), b.take(2)
        if kind == 0:
            b.p = (b.p + 7) & ~7
            n = b.take(16)
            b.take(16)
            b.p += 8 * n
            continue
        if kind == 1:
            lit, dist = decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), decoder([5] * 32)
        else:
            hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
            cl = [0] * 19
            for k in range(hclen):
                cl[CL_ORDER[k]] = b.take(3)
            clt, lens = decoder(cl), []
            while len(lens) < hlit + hdist:
                s, _ = symbol(b, clt)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + b.take(2))
                else:
                    lens += [0] * (3 + b.take(3) if s == 17 else 11 + b.take(7))
            lit, dist = decoder(lens[:hlit]), decoder(lens[hlit:])
        while True:
            s, n = symbol(b, lit)
            if s == 256:
                break
            if s < 256:
                c["literals"] += 1
                continue
            e = LEN_BITS[s - 257]
            length = LEN_BASE[s - 257] + b.take(e)
            d, dn = symbol(b, dist)
            b.take(DIST_BITS[d])
            c["matches"] += 1
            if n + e + dn <= LIT_BITS:
                c["fit"] += 1
                c["fit, length <= %d (built)" % PAIR_LEN_MAX] += length <= PAIR_LEN_MAX
                c["fit, length 3..10"] += e == 0 and length <= 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--payload", default="text", choices=["text", "mix"])
    a = ap.parse_args()
    c = {"literals": 0, "matches": 0, "fit": 0, "fit, length <= %d (built)" % PAIR_LEN_MAX: 0, "fit, length 3..10": 0}
    for seed in range(2, 8):
        count(corpus.deflate_raw(corpus.PAYLOADS[a.payload](65536, seed), 6), c)
    turns = c["literals"] + 2 * c["matches"]
    for k, v in c.items():
        print("%-32s %7d%s" % (k, v, "  (%.1f %% of the matches)" % (100.0 * v / c["matches"]) if k.startswith("fit") else ""))
    print("%-32s %7d" % ("loop turns (literals + 2 x matches)", turns))
    for k in list(c)[2:]:
        print("%-32s %7d  (x %.3f)" % ("turns, " + k, turns - c[k], (turns - c[k]) / turns))


if __name__ == "__main__":
    main()
