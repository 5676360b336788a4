"""Runs of Deflate units -- SWC_DEFLATE_JOINED / SWC_DEFLATE_OPEN jobs (include/swc_hip.h) -- and what is expected of them, shared
by the CPU tier (test_deflate_units_emulation.py) and the GPU tier (test_gpu_deflate_units.py).  TEST INFRASTRUCTURE.

What a unit must report follows from how it was BUILT (_deflate_build) and from what the ORACLE says about the same bytes as a
whole stream (_oracle.deflate):
  - a unit built to end open -- on a byte, where a block header would start: its plain text, in_consumed = its length, the bit
    still set (and the oracle decodes the unit ++ an empty final stored block to that text);
  - any other unit: what a plain job reports for its bytes -- the oracle's status, bytes and in_consumed -- the bit cleared.
"""
import random

import _deflate_build as DB
import _oracle as O

JOINED, OPEN = 1, 2
OK, REF_TRAP, CAPACITY, INVALID_ARGUMENT = 0, 900, 901, 903
FINAL_EMPTY = b"\x01\x00\x00\xff\xff"


def U(data, cap, aux, open_plain=None):
    """open_plain: the unit was built to end open -- on a byte, where a block header would start -- and this is its plain text."""
    return {"data": bytes(data), "cap": int(cap), "aux": int(aux), "open_plain": open_plain}


def text(rnd, n):
    words = [b"alpha", b"beta", b"gamma", b"delta", b"flush", b"point", b"unit", b"wave", b"\xc3\xa9t\xc3\xa9", b"\xf0\x9f\x8c\x8a"]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + rnd.choice([b" ", b", ", b"\n"])
    return bytes(out[:n])


def repetitive(rnd, n):
    """Text with real matches: a few phrases repeated."""
    phrases = [text(rnd, rnd.randint(5, 40)) for _ in range(6)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(phrases)
    return bytes(out[:n])


def greedy_tokens(plain):
    """Literals and matches (the longest match within the unit that starts at one of the last occurrences of the next three bytes)."""
    toks, i, last = [], 0, {}
    n = len(plain)
    while i < n:
        key = plain[i:i + 3]
        j = last.get(key)
        if len(key) == 3 and j is not None and i - j <= 32768:
            length = 3
            while length < 258 and i + length < n and plain[j + length] == plain[i + length]:
                length += 1
            toks.append((length, i - j))
            for k in range(i, i + length):
                last[plain[k:k + 3]] = k
            i += length
        else:
            last[key] = i
            toks.append(plain[i])
            i += 1
    return toks


def unit_open_stored(plain):
    """A fixed block and an empty stored block behind it: what Z_FULL_FLUSH leaves."""
    w = DB.BitWriter()
    DB.fixed_block(w, greedy_tokens(plain), False)
    DB.stored_block(w, b"", False)
    d = w.data()
    assert d.endswith(b"\x00\x00\xff\xff")
    return d


def unit_open_fixed_on_byte(plain):
    """A non-final fixed block that ends exactly on a byte: nine-bit literals (144 and above) appended until it does.  Returns
    (unit, plain text)."""
    plain = bytearray(plain)
    for _ in range(9):
        w = DB.BitWriter()
        DB.fixed_block(w, list(plain), False)
        if w.bit_length() % 8 == 0:
            return w.data(), bytes(plain)
        plain.append(200)
    raise AssertionError("no alignment found")


def unit_one_code_longer(plain):
    """unit_open_fixed_on_byte and one nine-bit code more: the end-of-block code ends one bit into a byte."""
    _, p = unit_open_fixed_on_byte(plain)
    w = DB.BitWriter()
    DB.fixed_block(w, list(p) + [201], False)
    assert w.bit_length() % 8 == 1
    return w.data()


def unit_final(plain, tail=b""):
    w = DB.BitWriter()
    DB.fixed_block(w, greedy_tokens(plain), True)
    return w.data() + tail


def unit_reaches_back(plain):
    """The first token is a match one byte in front of the unit."""
    w = DB.BitWriter()
    DB.fixed_block(w, [(5, 1)] + list(plain), False)
    DB.stored_block(w, b"", False)
    return w.data()


def expect(u):
    """(status, out_len, in_consumed, aux, bytes) of one unit, whatever its place in a run (no history is shared); None for what the
    test does not pin (the figures of a failed unit).  bytes: what lies at the job's `out`, min(out_len, out_cap) of them."""
    data, cap, aux = u["data"], u["cap"], u["aux"]
    if u.get("open_plain") is not None:   # built to end where a block header would start, on a byte: the unit ++ an empty final block is a stream
        plain = u["open_plain"]
        assert aux & OPEN and O.deflate(data + FINAL_EMPTY) == (OK, plain, len(data) + len(FINAL_EMPTY))
        res = (OK, len(plain), len(data), aux, plain)
    else:                                 # what a plain job reports for these bytes
        st, out, cons = O.deflate(data)
        res = (st, len(out), cons, aux & ~OPEN, out) if st == OK else (st, None, None, aux & ~OPEN, None)
    if res[0] == OK and res[1] > cap:
        return (CAPACITY, res[1], res[2], res[3], res[4][:cap])
    return res


def directed_runs():
    """name -> list of units (the first a head).  Capacities: the unit's own output, rounded up a little, so that a neighbour's first
    byte follows at an odd address."""
    rnd = random.Random(20261018)
    a, b, c, d = (repetitive(rnd, n) for n in (700, 333, 1501, 64))
    on_byte, on_byte_plain = unit_open_fixed_on_byte(text(rnd, 90))
    runs = {}
    runs["stored-markers"] = [U(unit_open_stored(a), len(a), OPEN, a), U(unit_open_stored(b), len(b), JOINED | OPEN, b), U(unit_final(c), len(c), JOINED)]
    runs["fixed-on-a-byte"] = [U(on_byte, len(on_byte_plain), OPEN, on_byte_plain), U(unit_final(d), len(d), JOINED)]
    runs["one-code-longer"] = [U(unit_one_code_longer(text(rnd, 90)), 200, OPEN), U(unit_final(d), len(d), JOINED)]
    runs["final-and-trailing"] = [U(unit_final(b, b"trailing bytes"), len(b), OPEN), U(unit_final(a), len(a), JOINED)]
    runs["reaches-back"] = [U(unit_open_stored(b), len(b), OPEN, b), U(unit_reaches_back(text(rnd, 50)), 100, JOINED | OPEN), U(unit_final(d), len(d), JOINED)]
    runs["over-capacity"] = [U(unit_open_stored(a), len(a), OPEN, a), U(unit_open_stored(c), 1000, JOINED | OPEN, c), U(unit_final(b), len(b), JOINED)]
    runs["empty-units"] = [U(unit_open_stored(b""), 1, OPEN, b""), U(unit_open_stored(b"x"), 1, JOINED | OPEN, b"x"), U(unit_final(b""), 1, JOINED | OPEN),
                           U(unit_final(a), len(a), JOINED)]
    return runs


def residue_pairs():
    """Copy: two adjacent units for each of the sixteen residues of the second unit's first byte (the first unit's length mod 16),
    both with matches, neither a multiple of the 16-byte line."""
    rnd = random.Random(7)
    runs = []
    for r in range(16):
        a = repetitive(rnd, 160 + r)
        b = repetitive(rnd, 99 + 3 * r)
        runs.append([U(unit_open_stored(a), len(a), OPEN, a), U(unit_final(b), len(b), JOINED)])
    return runs


def long_run():
    """Placing across tiles: 37 whole streams, then ONE run of 150 units that starts in the middle of tile 0 (job 37), fills tile 1
    without a head in it and ends in tile 2 -- the look-back goes two tiles deep -- then a short run behind it.  The units' sizes
    differ from their capacities (every capacity leaves 0..6 bytes unused), among them a unit of 0 bytes, one of 1 byte and one over
    capacity, so that no joined unit lands where a layout by capacities would put it.  Returns the job list."""
    rnd = random.Random(150)
    jobs = [U(unit_final(repetitive(rnd, 40 + 3 * i)), 40 + 3 * i + i % 5, 0) for i in range(37)]
    n = 150
    for k in range(n):
        size = {20: 0, 70: 1}.get(k, 30 + (k * 37) % 211)
        p = repetitive(rnd, size)
        cap = max(1, size - 50 if k == 100 else size + k % 7)
        aux = (JOINED if k else 0) | (OPEN if k + 1 < n else 0)
        jobs.append(U(unit_open_stored(p), cap, aux, p) if k + 1 < n else U(unit_final(p), cap, aux))
    a, b = repetitive(rnd, 77), repetitive(rnd, 130)
    jobs += [U(unit_open_stored(a), 80, OPEN, a), U(unit_final(b), 130, JOINED)]
    return jobs
