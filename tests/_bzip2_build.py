"""BZip2 streams BUILT symbol by symbol (TEST INFRASTRUCTURE): what no encoder writes, and what the decoder is specified to answer.

Three layers, each usable on its own:
  bit layer     `Builder`: stream header of any level, every block header field given explicitly (randomised bit, origPtr, the group
                map and each group word, the table and selector counts, selectors as MTF indices, code lengths as a start value and
                per-symbol delta walks), symbols coded with the table their group's selector names, codes assigned as
                Code.huffmanCodes assigns them (never validated), CRCs computed or given, bits behind the end-of-stream magic;
  symbol layer  `mtf_encode` (L -> RUNA / RUNB / MTF symbols) and `symbols_decode`, its inverse as the reference's symbol loop does
                it: run_length / repeat_power wrap at 64 bits, the run is written only if the wrapped value is > 0, and a run that
                fails that test is NOT reset;
  block layer   `bwt_reverse` (BurrowsWheeler.reverse: a stable counting sort and n pointer steps from origPtr -- for ANY L, one cycle
                or many), `rle1_undo` (the positional rule of BZip2.swift:251-267) and `bwt_forward` (T -> L, origPtr), so that the
                RLE1-encoded text T can be chosen directly.
`model_stream` restates the reference's decoder over the bits (heap semantics of DecodingTree for sets that are incomplete or
over-subscribed): the expected outcome of the cases whose codes are not prefix-free and of every error case comes from it.
"""
import collections
import random
import re
import zlib

import numpy as np

BLOCK_MAGIC = 0x314159265359
END_MAGIC = 0x177245385090
M64 = (1 << 64) - 1
N_USED_BOUNDARIES = (1, 2, 62, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
LIST_POSITIONS = (1, 62, 63, 64, 65, 127, 128, 191, 192, 255)
RANDOM_N = (1, 9, 49, 50, 51, 300, 4000, 20000)
MAX_OUTPUT = 1 << 24          # the oracle's cap in these tests (refcpu_set_max_output): a run beyond it is 901 on both sides

Case = collections.namedtuple("Case", "name stream plain status consumed block_bits l_len libbz2_ok block_crc block_plain block_status block_cycles")
TAIL = bytes((37 * j + 11) & 255 for j in range(256))     # behind a small stream: the decoder's look-ahead has its input (see `one`)

_REV8 = bytes(int("{:08b}".format(i)[::-1], 2) for i in range(256))


_RLE1 = re.compile(rb"(.)\1\1\1(.)", re.S)


def bz_crc(data):
    """CheckSums.bzip2crc32: the MSB-first CRC-32 -- zlib's with every byte and the result bit-reversed."""
    return int("{:032b}".format(zlib.crc32(bytes(data).translate(_REV8)))[::-1], 2)


# ------------------------------------------------------------------------------------------------------------------ block layer
def _pointers(L):
    return np.argsort(np.frombuffer(bytes(L), np.uint8), kind="stable")


def bwt_reverse(L, orig):
    """BurrowsWheeler.reverse(bytes:_:): None where the reference traps (origPtr outside a non-empty L)."""
    n = len(L)
    if n == 0:
        return b""
    if orig >= n:
        return None
    P = _pointers(L)
    if n > 2000:        # the n positions P(orig), P^2(orig), ... by doubling: seq[m:2m] = P^m[seq[:m]]
        seq, power = P[orig:orig + 1], P
        while len(seq) < n:
            seq = np.concatenate((seq, power[seq]))
            if len(seq) < n:
                power = power[power]
        return np.frombuffer(L, np.uint8)[seq[:n]].tobytes()
    P = P.tolist()
    out, e = bytearray(n), orig
    for i in range(n):
        e = P[e]
        out[i] = L[e]
    return bytes(out)


def cycles(L):
    """Number of cycles of the permutation the walk follows (1: what every encoder's L has)."""
    P = _pointers(L).tolist()
    seen, c = bytearray(len(P)), 0
    for i in range(len(P)):
        if not seen[i]:
            c += 1
            while not seen[i]:
                seen[i] = 1
                i = P[i]
    return c


def rle1_undo(T):
    """BZip2.swift:251-267: four equal bytes AND i < n - 4, then a count byte; anything else is a literal."""
    return _RLE1.sub(lambda m: m.group(1) * (m.group(2)[0] + 4), bytes(T))    # (leftmost, not overlapping: the reference's scan)


def rle1_roles(T):
    """Per byte of T what the undo takes it for: "l" a literal outside a run of four, "r" one of the four, "c" a count."""
    roles, i, n = [], 0, len(T)
    while i < n:
        if i < n - 4 and T[i] == T[i + 1] == T[i + 2] == T[i + 3]:
            roles += "rrrrc"
            i += 5
        else:
            roles.append("l")
            i += 1
    return roles


def bwt_forward(T):
    """(L, origPtr) of the text T: sorted rotations below 4 Ki, prefix doubling over numpy above."""
    T = bytes(T)
    n = len(T)
    assert 0 < n <= 70000
    if n < 4096:
        rot = sorted(range(n), key=lambda i: T[i:] + T[:i])
    else:
        idx = np.arange(n)
        rank = np.frombuffer(T, np.uint8).astype(np.int64)
        k = 1
        while True:
            second = rank[(idx + k) % n]
            order = np.lexsort((second, rank))
            a, b = rank[order], second[order]
            step = np.concatenate(([0], ((a[1:] != a[:-1]) | (b[1:] != b[:-1])).astype(np.int64)))
            new = np.empty(n, np.int64)
            new[order] = np.cumsum(step)
            rank = new
            if int(rank.max()) == n - 1 or k >= n:
                break
            k *= 2
        rot = np.lexsort((idx, rank)).tolist()
    L = bytes(T[i - 1] for i in rot)
    orig = rot.index(0)
    assert bwt_reverse(L, orig) == T
    return L, orig


# ----------------------------------------------------------------------------------------------------------------- symbol layer
def run_digits(run):
    """A run of `run` >= 1 in bijective base 2: RUNA (symbol 0) = 1, RUNB (symbol 1) = 2, lowest digit first."""
    d = []
    while run > 0:
        d.append(0 if run & 1 else 1)
        run = (run - 1) >> 1
    return d


def mtf_encode(L, used):
    """L -> symbols (without the end-of-block symbol): position 0 of the list counts into a run, position m > 0 is symbol m + 1."""
    lst, syms, run = list(used), [], 0
    for b in L:
        i = lst.index(b)
        if i == 0:
            run += 1
            continue
        syms += run_digits(run)
        run = 0
        syms.append(i + 1)
        lst.insert(0, lst.pop(i))
    return syms + run_digits(run)


def symbols_decode(syms, used, limit=MAX_OUTPUT):
    """The reference's symbol loop (BZip2.swift:212-246) over symbols: (status, L).  `syms` ends with the end-of-block symbol
    len(used) + 1.  900: usedSymbols[0] of an empty list; 901: a run beyond `limit`."""
    lst, out, rl, rp, eob = list(used), bytearray(), 0, 1, len(used) + 1
    for s in syms:
        if s < 2:
            rl = (rl + ((rp << s) & M64)) & M64
            rp = (rp << 1) & M64
            continue
        if 0 < rl < 1 << 63:
            if not lst:
                return 900, None
            if len(out) + rl > limit:
                return 901, None
            out += bytes([lst[0]]) * rl
            rl, rp = 0, 1
        if s == eob:
            return 0, bytes(out)
        lst.insert(0, lst.pop(s - 1))
        out.append(lst[0])
    raise AssertionError("no end-of-block symbol")


# ------------------------------------------------------------------------------------------------------------------ code tables
def ref_codes(lengths):
    """Code.huffmanCodes (Code.swift:15-39): (code, length) per symbol in (length, symbol) order, lengths <= 0 skipped, not validated."""
    codes, loop_bits, sym = {}, -1, -1
    for ln, s in sorted((ln, s) for s, ln in enumerate(lengths) if ln > 0):
        sym += 1
        if ln != loop_bits:
            sym <<= ln - loop_bits
            loop_bits = ln
        codes[s] = (sym & ((1 << ln) - 1), ln)
    return codes


def kraft(lengths):
    return sum(2.0 ** -l for l in lengths if l > 0)


def prefix_free(lengths):
    return all(1 <= l <= 20 for l in lengths) and kraft(lengths) == 1.0


def flat_lengths(count, depth=0):
    """A complete code of `count` >= 1 symbols below a node at `depth`: the first 2^d - count symbols one bit shorter."""
    if count == 1:
        return [depth]
    d = (count - 1).bit_length()
    short = (1 << d) - count
    return [depth + d - 1] * short + [depth + d] * (count - short)


def skew_lengths(count, k, perm=None):
    """A complete code: 1, 2, .. k bits for the first k symbols of `perm`, the rest flat below them."""
    k = max(0, min(k, count - 2))
    ls = list(range(1, k + 1)) + flat_lengths(count - k, k)
    assert max(ls) <= 20 and kraft(ls) == 1.0
    out = [0] * count
    for s, l in zip(perm if perm is not None else range(count), ls):
        out[s] = l
    return out


def default_tables(count, n_tables, seed=0):
    """`n_tables` complete codes over `count` symbols, all different wherever the alphabet has room for that."""
    rnd = random.Random(1000 * count + n_tables + seed)
    tables = []
    for t in range(n_tables):
        perm = list(range(count))
        rnd.shuffle(perm)
        tables.append(skew_lengths(count, t if count > 3 else 0, perm))
    return tables


# -------------------------------------------------------------------------------------------------------------------- bit layer
class Builder:
    """The bit layer.  Methods write exactly what they are given; `block` is the one convenience on top (a whole block from L)."""

    def __init__(self, level=9, counters=None):
        self.buf, self.acc, self.nacc = bytearray(), 0, 0
        self.n = collections.Counter() if counters is None else counters
        self.level = level
        self.blocks = []            # dicts: bit, l_len, crc, plain, status
        self.combined = 0
        self.libbz2_ok = 1 <= level <= 9
        self.put(0x425A68, 24)
        self.put(0x30 + level, 8)

    # -- raw bits
    def put(self, value, nbits):
        self.acc = (self.acc << nbits) | (value & ((1 << nbits) - 1))
        self.nacc += nbits
        if self.nacc >= 256:
            keep = self.nacc & 7
            self.buf += (self.acc >> keep).to_bytes((self.nacc - keep) // 8, "big")
            self.acc &= (1 << keep) - 1
            self.nacc = keep

    def bit_length(self):
        return len(self.buf) * 8 + self.nacc

    def data(self):
        pad = -self.nacc % 8
        return bytes(self.buf) + ((self.acc << pad).to_bytes((self.nacc + pad) // 8, "big") if self.nacc else b"")

    # -- block header fields
    def block_header(self, crc, orig, randomised=0, group_map=0, group_words=()):
        self.put(BLOCK_MAGIC, 48)
        self.put(crc, 32)
        body = self.bit_length()
        self.put(randomised, 1)
        self.put(orig, 24)
        self.put(group_map, 16)
        for w in group_words:
            self.put(w, 16)
        return body

    def counts(self, n_tables, n_selectors):
        self.put(n_tables, 3)
        self.put(n_selectors, 15)

    def selectors(self, mtf_indices):
        for c in mtf_indices:
            self.put(((1 << c) - 1) << 1, c + 1)

    def table(self, start, walks):
        """`walks`: per symbol the list of +1 / -1 steps taken before the symbol's closing 0 bit."""
        self.put(start, 5)
        for w in walks:
            for d in w:
                self.put(0b10 if d > 0 else 0b11, 2)
            self.put(0, 1)

    def table_lengths(self, lengths, start=None):
        """A table with these final lengths: the shortest walks from `start` (default: the first length, clamped to 0 .. 20)."""
        cur = max(0, min(20, lengths[0])) if start is None else start
        first, walks = cur, []
        for ln in lengths:
            walks.append([1 if ln > cur else -1] * abs(ln - cur))
            cur = ln
        self.table(first, walks)

    def symbols(self, syms, tables, sel):
        """Each symbol with the code its group's table gives it; a symbol without a code (length <= 0) leaves no bits."""
        codes = [ref_codes(t) for t in tables]
        for g in range(0, len(syms), 50):
            c = codes[sel[g // 50] if g // 50 < len(sel) else 0]
            for s in syms[g:g + 50]:
                if s in c:
                    self.put(*c[s])

    def end_of_stream(self, crc=None):
        self.put(END_MAGIC, 48)
        self.put(self.combined if crc is None else crc, 32)
        if crc is not None and crc != self.combined:
            self.libbz2_ok = False

    # -- a whole block
    def block(self, L, orig, used=None, tables=None, sel=None, n_selectors=None, sel_mtf=None, crc=None, syms=None, randomised=0,
              empty_groups=(), n_tables=None, starts=None, plain=None, status=0, odd=False, l_len=None):
        """One block whose BWT column is L.  `used`: the symbol map (sorted byte values); `tables`: code lengths per table over the
        len(used) + 2 symbols; `sel`: the table of every group of 50 symbols (default: round robin over the tables), `n_selectors`
        / `sel_mtf` / `n_tables`: what is written where that shall differ; `syms`: the symbols instead of mtf_encode(L) + end of
        block; `empty_groups`: groups whose bit is set with an empty word; `plain` / `status`: the block's outcome where it is not
        what (L, origPtr) give; `odd`: the codes are not prefix-free and complete -- the restated reference says what they decode to;
        `l_len`: the length of the column where L is not given (a block built for an error)."""
        L = bytes(L)
        used = sorted(set(L)) if used is None else list(used)
        count = len(used) + 2
        if syms is None:
            syms = mtf_encode(L, used) + [count - 1]
        tables = default_tables(count, 2) if tables is None else tables
        groups = (len(syms) + 49) // 50
        sel = [g % len(tables) for g in range(groups)] if sel is None else list(sel)
        if sel_mtf is None:
            lst, sel_mtf = list(range(len(tables))), []
            for t in sel:
                i = lst.index(t)
                sel_mtf.append(i)
                lst.insert(0, lst.pop(i))
        n_selectors = len(sel_mtf) if n_selectors is None else n_selectors
        n_tables = len(tables) if n_tables is None else n_tables
        l_len = len(L) if l_len is None else l_len
        if odd and plain is None and status == 0:
            # what the restated reference makes of these codes decides (a trial copy of the block with a CRC of 0)
            trial = Builder(self.level)
            trial.block(L, orig, used=used, tables=tables, sel=sel, n_selectors=n_selectors, sel_mtf=sel_mtf, crc=0, syms=syms,
                        empty_groups=empty_groups, n_tables=n_tables, starts=starts, plain=b"")
            trial.end_of_stream()
            r = _Bits(trial.data())
            r.p = trial.blocks[0]["bit"]
            status, plain, l_len = model_block(r)
        if plain is None and status == 0:
            T = bwt_reverse(L, orig)
            plain = rle1_undo(T)
            if len(T) >= 4 and T[-4:] == T[-1:] * 4 and (len(T) > 100000 or rle1_roles(T)[-4:] == list("llll")):
                self.libbz2_ok = False      # four equal bytes at the very end, no count: literals by the positional rule, an error in libbz2
        if crc is None:
            crc = bz_crc(plain) if plain is not None else 0
        elif status == 0 and crc != bz_crc(plain):
            status = 210
        words = [0] * 16
        for b in used:
            words[b >> 4] |= 0x8000 >> (b & 15)
        gmap = sum(0x8000 >> g for g in range(16) if words[g] or g in empty_groups)
        body = self.block_header(crc, orig, randomised, gmap, [words[g] for g in range(16) if words[g] or g in empty_groups])
        self.counts(n_tables, n_selectors)
        self.selectors(sel_mtf)
        for t, lengths in enumerate(tables):
            self.table_lengths(lengths, None if starts is None else starts[t])
        self.symbols(syms, tables, sel)
        if status == 0:
            self.combined = (((self.combined << 1) | (self.combined >> 31)) & 0xFFFFFFFF) ^ crc
        self.blocks.append(dict(bit=body, l_len=l_len, crc=crc, plain=plain, status=status, cycles=cycles(L) if 0 < len(L) <= 70000 and not odd else None))
        # what libbz2 reads: it walks n steps from origPtr like the reference, one cycle or many, and ignores surplus selectors up to
        # 18,002; it refuses an empty block, a block over the level, codes that are not complete and prefix-free
        if (odd or len(L) == 0 or orig >= max(len(L), 1) or len(L) > self.level * 100000 or n_selectors > 18002 or n_selectors < groups
                or not 2 <= n_tables <= 6 or empty_groups or randomised or status or not all(prefix_free(t) for t in tables)):
            self.libbz2_ok = False
        self._count(used, syms, tables, sel_mtf[:n_selectors], n_tables)
        return body

    def _count(self, used, syms, tables, sel_mtf, n_tables):
        """What the block reaches in the decoder's symbol loop, as the loop itself would see it: the list position of every byte
        symbol, the digits of every run, and for every run that a byte symbol ends the place i of that symbol in its group of 50
        and the bytes k staged in front of it (a run enters the staging register if run - 1 < 13 + i - k, else everything staged is
        flushed first).  This is the builder's own account of i and k, nothing the decoder reports, and it says nothing about whether
        the group runs in the decoder's fast form at all: that needs 184 bytes of input in front of the group (the tail of `one`), a
        table that is not over-subscribed and, symbol by symbol, a table index below 64."""
        n = self.n
        n["n_used", len(used)] += 1
        n["tables", n_tables] += 1
        for c in sel_mtf:
            n["selector", n_tables, c] += 1
        k = digits = 0
        rl, rp = 0, 1
        for at, s in enumerate(syms):
            i = at % 50 + 1
            if i == 1:
                k = 0
            if s < 2:
                rl, rp, digits = (rl + ((rp << s) & M64)) & M64, (rp << 1) & M64, digits + 1
                continue
            if digits:
                n["digits", digits] += 1
                if digits > 20:       # (libbz2 refuses a run of 2 Mi and more)
                    self.libbz2_ok = False
                if 0 < rl < 1 << 63:
                    admitted = rl - 1 < 13 + i - k
                    n["stage", i, k, admitted, rl - (13 + i - k)] += 1
                    k = k + rl if admitted else 0
                    rl, rp, digits = 0, 1, 0
                else:                 # not positive: skipped and NOT reset -- the next digits go on from here
                    n["wrapped", digits] += 1
                    digits = 0
            if s - 1 < len(used):
                n["position", s - 1] += 1
                k += 1

    def case(self, name, tail=b"", end=True, status=None, plain=None, consumed=None, libbz2_ok=None):
        if end:
            self.end_of_stream()
        consumed_bits = self.bit_length()
        stream = self.data() + tail
        bad = [b for b in self.blocks if b["status"]]
        if status is None:
            status = bad[0]["status"] if bad else 0
        if plain is None and status == 0:
            plain = b"".join(b["plain"] for b in self.blocks)
        ok = self.libbz2_ok and status == 0 and bool(self.blocks) if libbz2_ok is None else libbz2_ok
        return Case(name, stream, plain, status, (consumed_bits + 7) // 8 if consumed is None else consumed, [b["bit"] for b in self.blocks],
                    [b["l_len"] for b in self.blocks], ok, [b["crc"] for b in self.blocks], [b["plain"] for b in self.blocks],
                    [b["status"] for b in self.blocks], [b.get("cycles") for b in self.blocks])


# ------------------------------------------------------------------------------------------------------- the reference, restated
class _Bits:
    def __init__(self, data):
        self.s = bin(int.from_bytes(b"\x01" + bytes(data), "big"))[3:]
        self.p = 0

    def left(self):
        return len(self.s) - self.p

    def get(self, n):
        assert self.p + n <= len(self.s)
        v = int(self.s[self.p:self.p + n], 2) if n else 0
        self.p += n
        return v


def _tree(lengths):
    mx = max(max(lengths), 0)
    if mx > 26:
        return None
    return mx, {(l, c): s for s, (c, l) in sorted(ref_codes(lengths).items(), key=lambda kv: (kv[1][1], kv[0]))}


def _next(tree, r):
    mx, leaves = tree
    code = depth = 0
    while r.left() > 0:
        code, depth = code * 2 + r.get(1), depth + 1
        if depth > mx:
            return -1
        if (depth, code) in leaves:
            return leaves[depth, code]
    return -1


def model_block(r):
    """BZip2.decode(_:_:) over the bits: (status, output bytes of the block, length of L)."""
    if r.left() < 41:
        return 201, None, 0
    if r.get(1):
        return 205, None, 0
    orig, gmap = r.get(24), r.get(16)
    if r.left() < 16 * bin(gmap).count("1") + 18:
        return 201, None, 0
    used = []
    for g in range(16):
        if gmap & (0x8000 >> g):
            w = r.get(16)
            used += [16 * g + s for s in range(16) if w & (0x8000 >> s)]
    count = len(used) + 2
    n_tables = r.get(3)
    if not 2 <= n_tables <= 6:
        return 206, None, 0
    n_sel = r.get(15)
    lst, sel = list(range(n_tables)), []
    for _ in range(n_sel):
        c = 0
        while r.left() > 0 and r.get(1):
            c += 1
        if c >= n_tables:
            return 207, None, 0
        lst.insert(0, lst.pop(c))
        sel.append(lst[0])
    trees = []
    for _ in range(n_tables):
        if r.left() < 5:
            return 208, None, 0
        length, lengths = r.get(5), []
        for _ in range(count):
            if not 0 <= length <= 20:
                return 208, None, 0
            while r.left() > 0 and r.get(1):
                if r.left() <= 0:
                    return 208, None, 0
                length -= r.get(1) * 2 - 1
            lengths.append(length)
        t = _tree(lengths)
        if t is None:
            return 900, None, 0
        trees.append(t)
    if n_sel == 0:
        return 900, None, 0
    L, decoded, tree, si, rl, rp = bytearray(), 0, trees[sel[0]], 1, 0, 1
    while True:
        if decoded >= 50:
            if si >= n_sel:
                return 207, None, 0
            tree, si, decoded = trees[sel[si]], si + 1, 0
        s = _next(tree, r)
        if s == -1:
            return 209, None, 0
        decoded += 1
        if s < 2:
            rl, rp = (rl + ((rp << s) & M64)) & M64, (rp << 1) & M64
            continue
        if 0 < rl < 1 << 63:
            if not used:
                return 900, None, 0
            if len(L) + rl > MAX_OUTPUT:
                return 901, None, 0
            L += bytes([used[0]]) * rl
            rl, rp = 0, 1
        if s == count - 1:
            break
        used.insert(0, used.pop(s - 1))
        L.append(used[0])
    T = bwt_reverse(L, orig)
    if T is None:
        return 900, None, len(L)
    return 0, rle1_undo(T), len(L)


def model_stream(data):
    """BZip2.decompress(data:) over the bits: (status, bytes -- of status 0 and of 210 --, consumed, [length of L per block],
    [status per block, 210 where its own CRC does not match])."""
    r, out, total, ls, bs = _Bits(data), bytearray(), 0, [], []
    if r.left() < 32 or r.get(16) != 0x425A:
        return 201, b"", 0, ls, bs
    if r.get(8) != 104:
        return 202, b"", 0, ls, bs
    if not 0x31 <= r.get(8) <= 0x39:
        return 203, b"", 0, ls, bs
    while True:
        if r.left() < 80:
            return 201, b"", 0, ls, bs
        magic, crc = r.get(48), r.get(32)
        if magic == BLOCK_MAGIC:
            st, plain, n = model_block(r)
            ls.append(n)
            bs.append(st)
            if st:
                return st, b"", 0, ls, bs
            out += plain
            if bz_crc(plain) != crc:
                bs[-1] = 210
                return 210, bytes(out), 0, ls, bs
            total = (((total << 1) | (total >> 31)) & 0xFFFFFFFF) ^ crc
        elif magic == END_MAGIC:
            if total != crc:
                return 210, bytes(out), 0, ls, bs
            return 0, bytes(out), (r.p + 7) // 8, ls, bs
        else:
            return 204, b"", 0, ls, bs


def modelled(b, name, **kw):
    """The case of a builder whose outcome the restated reference decides over the finished stream (error cases: what follows the
    block can matter)."""
    kw.setdefault("tail", TAIL)
    c = b.case(name, **kw)
    st, plain, cons, ls, bs = model_stream(c.stream)
    return c._replace(plain=plain if st in (0, 210) else None, status=st, consumed=cons if st == 0 else c.consumed, libbz2_ok=False,
                      block_status=bs + c.block_status[len(bs):], l_len=ls + c.l_len[len(ls):])


# -------------------------------------------------------------------------------------------------------------------- directed
def text_over(used, n, seed, runs=False):
    """n bytes over the byte values `used`, every one of them present (n >= len(used)), no byte four times in a row unless `runs`."""
    rnd = random.Random(seed)
    used = list(used)
    t = used[:]
    rnd.shuffle(t)
    while len(t) < n:
        b = rnd.choice(used[:max(1, len(used) // 3)]) if rnd.random() < 0.5 else rnd.choice(used)
        if not runs and len(used) > 1 and len(t) >= 3 and t[-1] == t[-2] == t[-3] == b:
            continue
        t.append(b)
    return bytes(t[:max(n, len(used))])


def spread(n_used):
    """n_used byte values spread over the 16 groups of the symbol map."""
    return sorted(random.Random(n_used).sample(range(256), n_used))


def one(name, L, orig, counters, level=9, tail=TAIL, **kw):
    """A single-block stream.  The symbol loop takes its fast form -- on the device the assembly loop -- only for a group that has
    184 bytes of input in front of it (bzip2_block.h: br.next + 184 > br.n): a block of a few dozen bytes would never reach it, so
    256 bytes follow the end-of-stream magic unless the case says otherwise.  They are not part of the stream (`consumed`)."""
    b = Builder(level, counters)
    b.block(L, orig, **kw)
    return b.case(name, tail=tail)


def of_text(name, T, counters, level=9, tail=TAIL, **kw):
    L, orig = bwt_forward(T)
    return one(name, L, orig, counters, level, tail, **kw)


def from_symbols(name, syms, used, counters, orig=0, level=9, **kw):
    """A block given by its symbols (the end-of-block symbol appended here): L is what the reference's loop makes of them."""
    syms = list(syms) + [len(used) + 1]
    st, L = symbols_decode(syms, used)
    assert st == 0, (name, st)
    return one(name, L, orig if orig < max(len(L), 1) else 0, counters, level, used=used, syms=syms, **kw)


def staging_pairs():
    """(prefix of flushed runs, bytes staged, run, admitted) around run - 1 < 13 + i - k: for as many (i, k) as a group has, one run on
    each side of the rule with the same number of digits."""
    out = []
    for pre in (0, 1, 2, 4):
        for kb in (0, 1, 2, 3, 5, 8, 12, 17, 25, 33, 40):
            at = 7 * pre + kb          # a flushed run of 100 bytes: six digits and the byte symbol that ends it (staged: k = 1)
            k = kb + (1 if pre else 0)
            for r in range(1, 70):
                i = at + len(run_digits(r)) + 1
                if i <= 50 and r == 13 + i - k and len(run_digits(r + 1)) == len(run_digits(r)):
                    out.append((pre, kb, r, True))
                    out.append((pre, kb, r + 1, False))
    return out


def rle1_cut_text(n, situation):
    """T of n bytes whose cut points n * part / 64 (bzip2_block.h: rle1_undo_to_output) all fall `situation`: "inside" a run of four,
    on the "count" byte behind it, directly "behind" the count."""
    t = bytearray((37 + 11 * i) % 200 + 1 if i % 2 else (91 + 7 * i) % 199 + 2 for i in range(n))
    for i in range(3, n):            # (no accidental run, no two equal neighbours: every byte outside the runs placed below is a safe start)
        while t[i] == t[i - 1] or t[i] == t[i - 2]:
            t[i] = t[i] % 250 + 1
    for part in range(1, 64):
        cut = n * part // 64
        at = {"inside": cut - 2, "count": cut - 4, "behind": cut - 5}[situation]
        t[at:at + 4] = bytes([251]) * 4
        t[at + 4] = 252 if situation != "count" else 3
    return bytes(t)


def _build_directed(n):
    cases = []
    add = cases.append
    rnd = random.Random(0xB21)

    def fin(b, name, **kw):
        kw.setdefault("tail", TAIL)
        return b.case(name, **kw)

    # ---- symbol map and alphabet
    for n_used in N_USED_BOUNDARIES:
        used = spread(n_used)
        add(of_text("n_used-%d" % n_used, text_over(used, max(300, 3 * n_used), n_used), n, tables=default_tables(n_used + 2, 3, 5)))
    add(of_text("group-bit-set-with-an-empty-word", text_over([0x21, 0x22, 0x70], 120, 1), n, empty_groups=(0, 5, 15)))
    for what, syms in (("eob-position-symbols-only", [1, 1, 1]), ("a-run", [0, 1, 0])):
        b = Builder(9, n)
        b.block(b"", 0, used=[], syms=syms, tables=[[1, 1], [1, 1]], status=1)
        add(modelled(b, "n_used-0-with-" + what))
        b = Builder(9, n)
        b.block(b"", 0, used=[], syms=syms, tables=[[1, 1], [1, 1]], sel=[0] * 100, status=1)
        add(modelled(b, "n_used-0-with-%s-to-the-end-of-the-input" % what))

    # ---- tables and selectors
    abc = spread(40)
    for nt in (2, 3, 4, 5, 6):
        T = text_over(abc, 50 * nt * 3 + 17, nt)
        add(of_text("%d-tables-all-different-all-used" % nt, T, n, tables=default_tables(42, nt, 9)))
        L, orig = bwt_forward(T)
        groups = (len(mtf_encode(L, sorted(set(L)))) + 50) // 50
        sel, lst = [], list(range(nt))
        for g in range(groups):      # every selector MTF index 0 .. nt - 1, again and again
            c = g % nt
            lst.insert(0, lst.pop(c))
            sel.append(lst[0])
        add(one("%d-tables-every-selector-index" % nt, L, orig, n, tables=default_tables(42, nt, 3), sel=sel))
        b = Builder(9, n)
        b.block(L, orig, tables=default_tables(42, nt, 3), sel=sel, sel_mtf=[0, nt] + [0] * (groups - 2), status=207)
        add(fin(b, "%d-tables-selector-index-%d" % (nt, nt)))
    for nt in (0, 1, 7):
        b = Builder(9, n)
        b.block(b"abcab", 1, tables=default_tables(5, 2), n_tables=nt, status=206)
        add(fin(b, "n_tables-%d" % nt))
    T = text_over(abc, 330, 77)
    L, orig = bwt_forward(T)
    nsym = len(mtf_encode(L, abc)) + 1
    needed = (nsym + 49) // 50
    for extra, name in ((1, "needed-plus-1"), (18002 - needed, "18002"), (32767 - needed, "32767")):
        add(one("n_selectors-" + name, L, orig, n, sel=[g % 2 for g in range(needed)] + [rnd.randrange(2) for _ in range(extra)]))
    b = Builder(9, n)
    b.block(L, orig, sel=[g % 2 for g in range(needed - 1)], status=207)
    add(fin(b, "n_selectors-needed-minus-1"))
    b = Builder(9, n)
    b.block(L, orig, n_selectors=0, sel_mtf=[], status=900)
    add(fin(b, "n_selectors-0"))
    for nth in (50, 51):             # the end-of-block symbol as the 50th symbol of the last group / as the first of one more
        syms = [2 + (j % 7) for j in range(100 + nth - 1)]
        add(from_symbols("eob-as-symbol-%d-of-the-last-group" % nth, syms, abc, n, sel=[0, 1, 0] if nth == 50 else [0, 1, 0, 1]))
    b = Builder(9, n)
    syms = [2 + (j % 7) for j in range(150)] + [41]
    b.block(symbols_decode(syms, abc)[1], 0, used=abc, syms=syms, sel=[0, 1, 0], status=207)
    add(fin(b, "eob-as-symbol-51-without-its-selector"))

    # ---- code lengths
    small = [0x41, 0x42, 0x43, 0x44, 0x45, 0x46]                        # 8 symbols
    T8 = text_over(small, 140, 8)
    good = [3, 3, 3, 3, 3, 3, 3, 3]
    for start in (0, 1, 20, 21, 31):
        b = Builder(9, n)
        b.block(*bwt_forward(T8), tables=[good, skew_lengths(8, 4)], starts=[start, None], status=0 if start <= 20 else 208)
        add(fin(b, "code-length-start-%d" % start, libbz2_ok=False if start == 0 else None))
    b = Builder(9, n)                # the bit layer alone
    L, orig = bwt_forward(T8)
    syms = mtf_encode(L, small) + [7]
    body = b.block_header(bz_crc(T8), orig, 0, 0x0800, [sum(0x8000 >> (x & 15) for x in small)])
    b.counts(2, (len(syms) + 49) // 50)
    b.selectors([0, 1, 1][:(len(syms) + 49) // 50])
    for _ in range(2):               # 3 bits for every symbol, each reached by a walk up to 20 and back
        b.table(1, [[1] * 19 + [-1] * 17] + [[1] * 17 + [-1] * 17] * 7)
    b.symbols(syms, [good, good], [0, 1, 0])
    b.blocks.append(dict(bit=body, l_len=len(L), crc=bz_crc(T8), plain=T8, status=0))
    b.combined = bz_crc(T8)
    add(fin(b, "delta-walks-from-1-to-20-and-back"))
    for k in (0, 1):
        for bad, st in ((-1, 208), (21, 208), (0, 0)):
            tb = [skew_lengths(8, 3), skew_lengths(8, 2)]
            b = Builder(9, n)
            if bad == 0:             # length 0 is in 0 ... 20: a symbol without a code -- which the text then must not use
                tb[k] = [2, 2, 2, 0, 3, 3, 3, 3]
                syms = [s for s in mtf_encode(L, small) if s != 3] + [7]
                b.block(symbols_decode(syms, small)[1], 0, used=small, syms=syms, tables=tb, odd=True)
            else:
                tb[k] = [3, 3, 3, bad, 3, 3, 3, 3]
                b.block(L, orig, tables=tb, status=st)
            add(modelled(b, "non-final-symbol-driven-to-%d-in-table-%d" % (bad, k)))
        for last in (0, -2, 21, 22, 23, 24, 25, 26):
            tb = [skew_lengths(8, 3), skew_lengths(8, 2), good]
            tb[k] = [1, 2, 3, 4, 5, 6, 7, last]
            b = Builder(9, n)
            b.block(L, orig, tables=tb, odd=True)
            add(modelled(b, "final-symbol-at-%d-in-table-%d" % (last, k)))
    used256 = list(range(256))
    add(of_text("all-258-symbols-at-20-bits", text_over(used256, 700, 20), n, tables=[[20] * 258, [20] * 258], odd=True))
    # 64 symbols the text never uses at 7 bits, everything else at 8 and 9: every symbol of the text has a table index >= 64
    Lf, of_ = bwt_forward(text_over([3, 77, 78, 200, 201, 255], 400, 5))
    occurring = set(mtf_encode(Lf, used256)) | {257}
    short = [s for s in range(258) if s not in occurring][:64]
    deep = dict(zip([s for s in range(258) if s not in short], flat_lengths(194, 1)))
    lengths = [7 if s in short else deep[s] for s in range(258)]
    assert prefix_free(lengths)
    add(one("used-symbols-hold-the-longest-codes", Lf, of_, n, used=used256, tables=[lengths, lengths]))
    hole = [2, 2, 3, 3, 4, 4, 4, 5]   # 00 01 100 101 1100 1101 1110 11110: 11111 is no code
    b = Builder(9, n)
    b.block(L, orig, tables=[hole, hole], syms=mtf_encode(L, small)[:70], status=209)
    b.put(0b11111, 5)
    add(modelled(b, "incomplete-code-whose-missing-word-occurs"))
    b = Builder(9, n)
    b.block(L, orig, tables=[hole, skew_lengths(8, 2)], odd=True)
    add(modelled(b, "incomplete-code-whose-missing-word-never-occurs"))
    # over-subscribed, and read as written: a complete code over the symbols the text uses, and one symbol more -- list position 6,
    # the byte that never occurs -- a bit longer than all of them: Code.huffmanCodes wraps its code to 0000.., below the first leaf
    small7 = small + [0x47]
    beyond = skew_lengths(8, 3) [:7] + [max(skew_lengths(8, 3)) + 1] + skew_lengths(8, 3)[7:]
    assert kraft(beyond) > 1
    for nt, name in ((2, "alternating-with-a-prefix-free-one"), (3, "between-two-prefix-free-ones")):
        L2, o2 = bwt_forward(text_over(small, 450, nt))
        b = Builder(9, n)
        b.block(L2, o2, used=small7, tables=[skew_lengths(9, 3), beyond, skew_lengths(9, 0)][:nt], odd=True)
        add(modelled(b, "over-subscribed-table-" + name))
        assert cases[-1].status == 0 and cases[-1].plain == rle1_undo(bwt_reverse(L2, o2))
    over = [2, 2, 2, 2, 2, 3, 3, 3]   # five 2-bit codes: the fifth takes the first's leaf, the 3-bit ones are shadowed -- NOT read as written
    for nt in (2, 3):
        L2, o2 = bwt_forward(text_over(small, 450, nt))
        b = Builder(9, n)
        b.block(L2, o2, tables=[skew_lengths(8, 3), over, good][:nt], odd=True)
        add(modelled(b, "over-subscribed-table-with-stolen-leaves-%d-tables" % nt))
    b = Builder(9, n)
    b.block(b"\x41" * 30, 0, used=small, tables=[over, over], odd=True)
    add(modelled(b, "over-subscribed-tables-only"))

    # ---- symbol loop
    for pos in LIST_POSITIONS:
        syms = [pos + 1, 2, pos + 1, 0, 3, pos + 1]
        add(from_symbols("byte-from-list-position-%d" % pos, syms, used256, n, tables=default_tables(258, 2, pos)))
    # (runs of the byte 0: four zeros and a count of 0 in T -- the RLE1 undo shrinks them; of a letter it would make 17 times as much)
    zed = [0, 0x42, 0x43, 0x44, 0x45, 0x46]
    # 23 digits, at the block start and directly before the end-of-block symbol at once: "one-run-of-2^23" below, a block with only
    # that run -- the one block of that size
    for d in range(1, 23):
        run = sum((2 if j % 3 else 1) << j for j in range(d)) if d <= 16 else (1 << d) - 1 + d
        assert len(run_digits(run)) == d
        add(from_symbols("run-of-%d-digits-at-the-block-start" % d, run_digits(run) + [2, 3, 2], zed, n, orig=run // 2))
        add(from_symbols("run-of-%d-digits-before-eob" % d, [2, 2] + run_digits(run), zed, n, orig=1))      # (2, 2: the byte 0 is in front again)
    # split across a group boundary with a table switch: 2 .. 18 digits, the first, the middle and the last place to split.  (19 .. 23
    # digits are left out here: three more columns of 0.5 .. 12 MB each, and the split itself is no different for them)
    for d in range(2, 19):
        for split in range(1, d):
            if split in (1, d - 1, d // 2):
                run = sum((1 + (j + split) % 2) << j for j in range(d)) if d < 18 else (1 << 18) + 1000 + split      # (18: the shortest ones)
                assert len(run_digits(run)) == d
                syms = [2 + j % 5 for j in range(50 - split)] + run_digits(run) + [3, 2]
                add(from_symbols("run-of-%d-digits-split-%d-before-a-table-switch" % (d, split), syms, zed, n,
                                 tables=[skew_lengths(8, 5), skew_lengths(8, 1, [7, 6, 5, 4, 3, 2, 1, 0])]))
    for pre, kb, r, admitted in staging_pairs():
        # byte symbols behind the run up to the 50th of the group: with the longest run the rule admits, k + run + (51 - i) is exactly
        # 64 -- the staging register is full to its last lane when the group ends, and one byte more would be lost
        syms = (run_digits(100) + [3]) * pre + [2 + j % 4 for j in range(kb)] + run_digits(r) + [3]
        syms += [2 + j % 4 for j in range(50 - len(syms))]
        # (such a column has many cycles and the walk follows one: origPtr is the place of the group's last byte, so that this byte --
        # the one a register filled beyond its last lane would lose -- is among the bytes compared)
        last = len(symbols_decode(syms + [7], small)[1]) - 1
        add(from_symbols("run-%d-behind-%d-flushed-runs-and-%d-bytes-%s" % (r, pre, kb, "admitted" if admitted else "flushed"), syms + [3, 2, 2],
                         small, n, orig=last, tables=default_tables(8, 2, r)))
    for d in (63, 64, 65, 66, 130):
        # (63 RUNB: -2 with a repeat power of 2^63 -- one more digit would make it huge; 64 and more: -2 for good, the repeat power is 0)
        syms = [2, 3] + [1] * d + ([2, 4, 0, 1, 3] if d >= 64 else []) + [3, 2]
        add(from_symbols("run-of-%d-digits-wrapped-not-positive" % d, syms, small, n))
    add(from_symbols("run-of-64-digits-wrapped-to-5", [2, 3] + run_digits((1 << 64) + 5) + [3, 0, 2], small, n))
    add(from_symbols("block-with-only-a-run", run_digits(37), [0x61], n))
    add(from_symbols("block-with-only-a-run-of-one", [0], [0x61, 0x62], n))
    add(from_symbols("block-of-eob-only", [], small, n))
    b = Builder(9, n)
    b.block(*bwt_forward(T8))
    b.block(b"", 0, used=small, tables=default_tables(8, 2))
    b.block(*bwt_forward(T8[::-1]), tables=default_tables(8, 3))
    add(fin(b, "block-of-eob-only-between-two-blocks"))

    # ---- end of input: the same block, 0 .. 200 bytes behind the end-of-stream magic
    T = text_over(abc, 900, 31)
    for extra in (0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 120, 144, 160, 170, 176, 180, 183, 184, 185, 192, 200):
        add(of_text("%d-bytes-behind-the-end-of-stream-magic" % extra, T, n, tail=bytes((7 * j + extra) & 255 for j in range(extra)),
                    tables=default_tables(42, 4, 2)))

    # ---- workspace
    for ln in (100001, 100065, 400100):
        rr = random.Random(ln)
        L = bytes(rr.choice(b"abcdefgh") for _ in range(ln))
        add(one("BZh1-with-L-of-%d" % ln, L, ln // 3, n, level=1, used=list(b"abcdefgh")))
    for p in (12, 16, 20, 23):
        # (2^23: nothing but the run -- 23 digits at the block start and directly before the end-of-block symbol)
        add(from_symbols("one-run-of-2^%d" % p, [2] + run_digits(1 << p) + [3] if p < 23 else run_digits(1 << p), [0, 1, 2], n, level=1, orig=1, tail=b""))
    b = Builder(1, n)
    syms = [2] + run_digits(1 << 25) + [3, 4]
    b.block(b"", 0, used=[0, 1, 2], syms=syms, status=901, l_len=(1 << 25) + 3)
    add(fin(b, "one-run-of-2^25"))

    # ---- BWT
    Ln = bytes(rnd.choice(b"xyz") for _ in range(40))
    add(one("origPtr-0", Ln, 0, n))
    add(one("origPtr-n-minus-1", Ln, 39, n))
    for orig in (40, (1 << 24) - 1):
        b = Builder(9, n)
        b.block(Ln, orig, status=900)
        add(fin(b, "origPtr-%d-of-40" % orig))
    for k in range(1, 9):
        b = Builder(9, n)
        for orig in range(k):
            b.block(b"q" * k, orig, used=[0x71, 0x72])
        add(fin(b, "L-of-%d-equal-bytes-every-origPtr" % k))
    two = next(x for x in (bytes(rnd.choice(b"abc") for _ in range(24)) for _ in range(10000)) if cycles(x) == 2)
    add(one("two-cycles", two, 5, n))
    Lm = bytes(sorted(text_over(small, 3000, 4)))
    add(one("many-cycles-sorted-L", Lm, 1234, n))
    Lr = text_over(abc, 5000, 12)
    assert cycles(Lr) > 2
    add(one("many-cycles-arbitrary-L", Lr, 4999, n))
    for ln in (1, 2, 3, 31, 32, 33, 64, 65, 511, 512, 513, 1024, 1025):
        add(of_text("single-cycle-n-%d" % ln, text_over(abc[:min(ln, 40)], ln, ln) if ln >= 3 else b"ab"[:ln], n))
        if ln > 3:
            add(one("arbitrary-L-n-%d" % ln, text_over(abc[:min(ln, 40)], ln, ln + 1), ln - 2, n))
    T = text_over(abc, 2048, 2)
    # rotating T changes origPtr alone.  The marks of 2,048 bytes: multiples of 4 in the block's own wavefront (512 segments), of 32 in
    # the team walk
    for want, name in ((lambda o: o % 32 == 0 and o > 0, "on"), (lambda o: o % 4 == 1, "off")):
        L2, o2 = next(x for x in (bwt_forward(T[sh:] + T[:sh]) for sh in range(2048)) if want(x[1]))
        add(one("origPtr-%s-a-mark" % name, L2, o2, n))

    # ---- RLE1 (T chosen)
    for k in range(1, 13):
        add(of_text("rle1-a-times-%d" % k, b"a" * k, n, used=[0x61, 0x62]))
    add(of_text("rle1-ends-in-four-equal-no-count", b"xyzzy-aaaa", n))
    add(of_text("rle1-four-equal-count-0", b"xy-aaaa\x00-z", n))
    add(of_text("rle1-four-equal-count-255", b"xy-aaaa\xff-z", n))
    add(of_text("rle1-count-equal-to-the-byte-then-the-byte", b"aaaaa" * 9 + b"b", n))
    add(of_text("rle1-count-followed-by-three-bytes-equal-to-it", b"zaaaa\x07\x07\x07\x07\x02q" + b"bbbb\x62bbb!", n))
    for ln in list(range(64, 71)) + [5, 17, 40, 63]:
        add(of_text("rle1-parts-n-%d" % ln, bytes(b"pqqqq\x03r"[j % 7] for j in range(ln)), n))
    add(of_text("rle1-no-safe-start-at-all", b"aabbaabbccaa" * 40 + b"aa", n))
    for situation in ("inside", "count", "behind"):
        T = rle1_cut_text(4096 + 640, situation)
        roles = rle1_roles(T)
        for part in range(1, 64):    # the layout came from the formula; what the undo takes the bytes at the cut for is counted
            cut = len(T) * part // 64
            n["rle1-cut", {"r": "inside", "c": "count"}.get(roles[cut], "behind" if roles[cut - 1] == "c" else "literal")] += 1
        add(of_text("rle1-cut-points-%s" % situation, T, n))
    add(of_text("rle1-50000-of-aaaa-ff", b"aaaa\xff" * 10000, n))

    # ---- streams
    for nb in (1, 2, 3, 5):
        for shift in range(8):
            if nb in (2, 3) or shift in (0, 5):
                b = Builder(9, n)
                for j in range(nb):
                    T = text_over(abc[:12 + j], 150 + 60 * j, 100 * nb + j)
                    L, orig = bwt_forward(T)
                    g = (len(mtf_encode(L, sorted(set(L)))) + 50) // 50
                    b.block(L, orig, sel=[x % 2 for x in range(g)] + [(g - 1) % 2] * (shift + j))     # surplus selectors of one bit each
                add(b.case("%d-blocks-shifted-by-%d" % (nb, shift)))
    nib = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 9]
    used14 = list(range(0x30, 0x3E))
    flat16 = [[4] * 16, [4] * 16]
    for magic, digits in (("block", nib), ("end-of-stream", [1, 7, 7, 2, 4, 5, 3, 8, 5, 0, 9, 0])):
        for lead in range(9):
            # sixteen symbols of four bits, symbol == code: the nibbles of the magic as symbols behind `lead` byte symbols (a nibble of
            # 0 or 1 is a run digit, 15 would end the block: the magics hold no 15).  A leading symbol moves the magic by four bits,
            # a surplus selector by one: 5 * lead mod 8 takes every value.
            syms = [2 + j % 3 for j in range(lead)] + digits + [2, 3]
            add(from_symbols("%s-magic-in-the-data-behind-%d-symbols" % (magic, lead), syms, used14, n, tables=flat16, sel=[0] * (1 + lead % 8)))
    three = [text_over(abc[:9], 200, 400 + j) for j in range(3)]
    b = Builder(9, n)
    for j, T in enumerate(three):
        L, orig = bwt_forward(T)
        b.block(L, orig, crc=bz_crc(T) ^ (0x10 if j == 1 else 0))
    add(fin(b, "wrong-crc-on-block-2-of-3", status=210, plain=three[0] + three[1], libbz2_ok=False))
    b = Builder(9, n)
    for T in three:
        b.block(*bwt_forward(T))
    b.end_of_stream(b.combined ^ 1)
    add(fin(b, "wrong-combined-crc", end=False, status=210, plain=b"".join(three), libbz2_ok=False))
    return cases


_cache = {}


def _directed():
    if not _cache:
        n = collections.Counter()
        _cache["cases"] = _build_directed(n)
        _cache["counters"] = n
    return _cache


def directed_cases():
    return _directed()["cases"]


def directed_counters():
    return _directed()["counters"]


def multi_cases():
    """(name, data): built streams back to back, for multi_decompress."""
    by = {c.name: c for c in directed_cases()}
    a, b, c = by["3-blocks-shifted-by-3"], by["2-blocks-shifted-by-6"], by["5-blocks-shifted-by-5"]
    return [("two-built-streams", a.stream + b.stream), ("three-built-streams", b.stream + c.stream + a.stream)]


# ---------------------------------------------------------------------------------------------------------------------- random
STYLES = ("many tables", "long codes", "runs", "deep MTF", "RLE1-heavy T", "arbitrary L")


def random_lengths(rnd, count, long_codes):
    perm = list(range(count))
    rnd.shuffle(perm)
    k = rnd.randrange(0, 17 if long_codes else 5)
    return skew_lengths(count, min(k, 20 - max(1, (count - 1).bit_length())), perm)


def random_block(rnd, b, strict=True, constructs=None, n=None, style=None):
    """One more status-0 block on the builder `b`.  strict: only what libbz2 reads (prefix-free complete codes of 1 .. 20 bits, at most
    18,002 selectors, origPtr < n, n within the level, L from a forward BWT); otherwise also what it refuses -- each such construct is
    added to the set `constructs`."""
    style = rnd.choice(STYLES) if style is None else style
    n = rnd.choice(RANDOM_N) if n is None else n
    n_used = rnd.choice(N_USED_BOUNDARIES)
    used = sorted(rnd.sample(range(256), n_used))
    if strict and style == "arbitrary L":
        style = "deep MTF"
    if style == "runs":
        t, cur = bytearray(), used[0]
        while len(t) < n:
            cur = rnd.choice(used[:4])
            t += bytes([cur]) * rnd.choice([1, 2, 3, 5, 13, 14, 15, 40, 64, 300])
        text = bytes(t[:n])
    elif style == "RLE1-heavy T":
        t = bytearray()
        while len(t) < n:
            c = rnd.choice(used[:3])
            t += bytes([c]) * rnd.choice([1, 3, 4, 4, 4, 5, 8]) + bytes([rnd.choice([0, 1, c, 255, rnd.randrange(256)])]) * rnd.randrange(2)
        text = bytes(t[:n])
        used = sorted(set(used) | set(text))
    elif style == "deep MTF":
        text = bytes(rnd.choice(used) for _ in range(n))
    else:
        text = bytes(rnd.choice(used[:max(1, len(used) // 4)]) if rnd.random() < 0.7 else rnd.choice(used) for _ in range(n))
    if strict and len(text) >= 4 and text[-4:] == text[-1:] * 4:      # (libbz2 refuses four equal bytes at the end without a count)
        text = text[:-1] + bytes([text[-1] ^ 1])
        used = sorted(set(used) | set(text))
    if style in ("arbitrary L", "runs") and not strict:
        L, orig = text, rnd.randrange(n)
        if style == "runs":
            L = bytes(sorted(L)) if rnd.randrange(2) else L
        if constructs is not None and cycles(L) > 1:
            constructs.add("multi-cycle L")
    else:
        L, orig = bwt_forward(text)
    count = len(used) + 2
    nt = rnd.randrange(2, 7) if style != "many tables" else rnd.choice([5, 6])
    tables = [random_lengths(rnd, count, style == "long codes") for _ in range(nt)]
    syms = mtf_encode(L, used) + [count - 1]
    kw = {}
    if not strict and rnd.randrange(3) == 0 and len(L) > 20 and syms[-2] >= 2:
        # a wrapped run in front of the end-of-block symbol: 64 RUNB digits leave -2 and a repeat power of 0 -- nothing is written
        syms = syms[:-1] + [1] * 64 + [count - 1]
        kw["odd"] = True
        if constructs is not None:
            constructs.add("wrapped run")
    groups = (len(syms) + 49) // 50
    sel = [rnd.randrange(nt) for _ in range(groups)]
    if not strict and rnd.randrange(3) == 0:
        sel += [rnd.randrange(nt) for _ in range(rnd.choice([1, 7, 18100 - groups if groups < 100 else 3]))]
        if constructs is not None:
            constructs.add("surplus selectors")
    idle = [s for s in range(2, count - 1) if s not in set(syms)]
    if not strict and rnd.randrange(3) == 0 and idle and count >= 4:
        # over-subscribed and still read as written: a complete code over all symbols but one that the block never uses, and that one
        # a bit longer than the longest -- Code.huffmanCodes wraps its code to 00 .. 0, below the leaf of the first code
        u, t = rnd.choice(idle), rnd.randrange(nt)
        rest = random_lengths(rnd, count - 1, False)
        tables[t] = rest[:u] + [max(rest) + 1] + rest[u:]
        kw["odd"] = True
        if constructs is not None:
            constructs.add("over-subscribed table")
    if constructs is not None and len(L) > b.level * 100000:
        constructs.add("block size over the level")
    b.block(L, orig, used=used, tables=tables, sel=sel, syms=syms, **kw)


def random_stream(rnd, strict=True, constructs=None, name="random", big=None):
    """1 .. 4 random blocks; `big` (default: one stream in eight that is not strict): a BZh1 whose first block is larger than the
    level allows."""
    big = not strict and (rnd.randrange(8) == 0 if big is None else big)
    b = Builder(1 if big else rnd.randrange(1, 10))
    for j in range(rnd.randrange(1, 5)):
        if big and j == 0:
            L = bytes(rnd.choice(b"\x00\x01\x02\xfe\xff") for _ in range(100000 + rnd.choice([1, 64, 65, 3000])))
            b.block(L, rnd.randrange(len(L)))
            if constructs is not None:
                constructs.add("block size over the level")
                constructs.add("multi-cycle L")
        else:
            random_block(rnd, b, strict, constructs)
    return b.case(name)
