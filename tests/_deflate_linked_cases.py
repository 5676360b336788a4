"""Runs of Deflate units that share history -- SWC_DEFLATE_LINKED jobs (include/swc_hip.h) -- and what is expected of them, shared by
the CPU tier (test_deflate_linked_emulation.py) and the GPU tier (test_gpu_deflate_linked.py).  TEST INFRASTRUCTURE.

The units of a run are consecutive pieces of ONE stream, built token by token (_deflate_build) or cut from zlib's output.  What
job k must leave is the ORACLE's decode (_oracle.deflate) of the units of its chain up to and including k, concatenated -- closed
with an empty final block where unit k ends open -- minus what the units in front of it produced; where the oracle reports an
error, job k reports that status.  A chain begins at every job without the LINKED bit (and behind a job that has the bit without
JOINED, which reports SWC_E_INVALID_ARGUMENT and leaves nothing).

What the oracle cannot say, because no stream looks like it, follows from the contract:
  - a unit whose reach lies in front of its history is SWC_E_REF_TRAP with the sizes the parse found -- the oracle's for the unit
    behind 32,768 bytes of history -- and not one of its bytes written;
  - behind a unit that failed, trapped or lacked room the bytes in front are not the stream's any more: of the units behind it the
    status and the sizes are pinned -- every job keeps its own -- and the bytes are not.
"""
import random
import zlib

import _deflate_build as DB
import _deflate_units_cases as K
import _oracle as O

JOINED, OPEN, LINKED = 1, 2, 4
JL = JOINED | LINKED
OK, REF_TRAP, CAPACITY, INVALID_ARGUMENT = K.OK, K.REF_TRAP, K.CAPACITY, K.INVALID_ARGUMENT
FINAL_EMPTY = K.FINAL_EMPTY
FILL = 0xA5   # what the drivers fill the output buffers with: the bytes of a trapped unit keep it


def U(data, cap, aux, ends_open):
    return {"data": bytes(data), "cap": int(cap), "aux": int(aux), "ends_open": bool(ends_open)}


def _history_block():
    w = DB.BitWriter()
    DB.stored_block(w, bytes(32768), False)
    return w.data()


_HIST = _history_block()


def parse_view(u):
    """What phase 1 reports for the unit on its own: (status, out_len, in_consumed, aux); a linked unit behind a full history."""
    tail = FINAL_EMPTY if u["ends_open"] else b""
    if u["aux"] & LINKED:
        st, out, cons = O.deflate(_HIST + u["data"] + tail)
        n, cons = len(out) - 32768, cons - len(_HIST)
    else:
        st, out, cons = O.deflate(u["data"] + tail)
        n = len(out)
    if st != OK:
        return (st, None, None, u["aux"] & ~OPEN)
    if u["ends_open"]:
        assert cons == len(u["data"]) + len(FINAL_EMPTY)
        return (OK, n, len(u["data"]), u["aux"])
    return (OK, n, cons, u["aux"] & ~OPEN)


def expect(units):
    """Per job (status, out_len, in_consumed, aux, bytes); None for what is not pinned: the figures of a unit that failed on its own,
    the bytes of a unit behind one that did not come out whole."""
    res = []
    orphan = True          # job 0 and what is joined to it have no head
    prefix, made, clean = b"", 0, True
    for i, u in enumerate(units):
        aux = u["aux"]
        if not aux & JOINED:
            orphan = False
        pv = parse_view(u)
        if aux & LINKED and not aux & JOINED:          # reported by phase 1, which does not parse it: the chain behind it starts with nothing
            res.append((INVALID_ARGUMENT, 0, 0, aux & ~OPEN, b""))
            prefix, made, clean = b"", 0, True
            continue
        if orphan:
            res.append((INVALID_ARGUMENT, 0, 0, pv[3], b""))
            continue
        if not aux & LINKED:
            prefix, made, clean = b"", 0, True
        if pv[0] != OK:                                 # broken on its own: the status, and what lies behind it is anybody's
            if clean:
                assert O.deflate(prefix + u["data"])[0] == pv[0]
            res.append((pv[0], None, None, pv[3], None))
            clean = False
            continue
        st, n, cons, aux_out = pv
        kept = min(n, u["cap"])
        if clean:
            ost, out, _ = O.deflate(prefix + u["data"] + (FINAL_EMPTY if u["ends_open"] else b""))
            if ost == OK:
                assert len(out) == made + n
                res.append((CAPACITY if n > u["cap"] else OK, n, cons, aux_out, out[made:made + kept]))
                clean = n <= u["cap"]
            else:
                assert ost == REF_TRAP and aux & LINKED, "the stream fails where the unit alone does not: only a reach can do that"
                res.append((REF_TRAP, n, cons, aux_out, bytes([FILL]) * kept))
                clean = False
        else:
            res.append((CAPACITY if n > u["cap"] else OK, n, cons, aux_out, None))
        prefix += u["data"]
        made += kept
    return res


# ---------------------------------------------------------------------------------------------------------------- builders
def sync_unit(tokens, final=False):
    """A fixed block and, unless it is the stream's last, the empty stored block of a sync flush behind it."""
    w = DB.BitWriter()
    DB.fixed_block(w, tokens, final)
    if not final:
        DB.stored_block(w, b"", False)
    return w.data()


def run_of(specs):
    """specs: (tokens, aux) or (tokens, aux, cap) per unit, the last unit final unless its aux says OPEN.  Capacity: what the tokens
    produce, unless given."""
    units = []
    for k, spec in enumerate(specs):
        tokens, aux = spec[0], spec[1]
        n = sum(1 if isinstance(t, int) else t[0] for t in tokens)
        units.append(U(sync_unit(tokens, final=not aux & OPEN), spec[2] if len(spec) > 2 else max(n, 1), aux, aux & OPEN))
    return units


def lits(rnd, n):
    return list(K.text(rnd, n))


def rep_tokens(rnd, n):
    return K.greedy_tokens(K.repetitive(rnd, n))


def directed_runs():
    """name -> list of units."""
    rnd = random.Random(20261019)
    runs = {}
    a100 = lits(rnd, 100)
    runs["seam-5-1"] = run_of([(a100, OPEN), ([(5, 1)] + lits(rnd, 40), JL)])
    runs["seam-every-byte"] = run_of([(a100, OPEN), ([(10, 100)] + lits(rnd, 33), JL)])
    runs["seam-one-more"] = run_of([(a100, OPEN), ([(10, 101)] + lits(rnd, 33), JL | OPEN), (lits(rnd, 20), JL)])
    runs["overlap-across-the-seam"] = run_of([(a100, OPEN), ([(258, 3)] + lits(rnd, 7) + [(258, 1), (100, 260)], JL)])
    # saturation: the third unit reaches 32,768 back at its first byte -- legal with 40,000 bytes in front, a trap with 32,767
    big_a, big_b = rep_tokens(rnd, 20000), rep_tokens(rnd, 20000)
    third = [(100, 32768)] + rep_tokens(rnd, 19000) + [(258, 32768), (3, 32767)]
    runs["saturation-legal"] = run_of([(big_a, OPEN), (big_b, JL | OPEN), (third, JL)])
    runs["saturation-trap"] = run_of([(rep_tokens(rnd, 12767), OPEN), (big_b, JL | OPEN), ([(10, 32768)] + lits(rnd, 50), JL)])
    # a source in the history and far in front of the 6 KiB window of the copier
    body = rep_tokens(rnd, 7000)
    runs["outside-the-window"] = run_of([(rep_tokens(rnd, 3000), OPEN), (body + [(200, 7100)] + rep_tokens(rnd, 1000) + [(30, 8300)], JL)])
    # a chain that restarts: head, linked, joined only, linked, linked -- the fourth job's history ends at the third's `out`
    t3 = lits(rnd, 77)
    for name, d in (("restart-legal", 77), ("restart-trap", 78)):
        runs[name] = run_of([(lits(rnd, 120), OPEN), ([(7, 120)] + lits(rnd, 30), JL | OPEN), (t3, JOINED | OPEN),
                             ([(20, d)] + lits(rnd, 11), JL | OPEN), ([(50, 77 + 31)] + lits(rnd, 9), JL)])
    # capacity and failure: every unit's sizes stay exact, every unit keeps its own status
    runs["predecessor-over-capacity"] = run_of([(a100, OPEN), ([(30, 90)] + rep_tokens(rnd, 1500), JL | OPEN, 1000), ([(9, 40)] + lits(rnd, 60), JL | OPEN),
                                                (lits(rnd, 5) + [(40, 20)], JL)])
    broken = lits(rnd, 300) + [(8, 350), ("code", "lit", 286)]
    runs["failed-in-mid-chain"] = [run_of([(a100, OPEN)])[0], U(sync_unit(broken), 400, JL | OPEN, False),
                                   run_of([([(6, 10)] + lits(rnd, 25), JL | OPEN)])[0], run_of([(lits(rnd, 3) + [(12, 9)], JL)])[0]]
    # units of 0 and 1 bytes; the bit without JOINED; a linked job 0
    runs["zero-and-one"] = run_of([(a100, OPEN), ([], JL | OPEN), ([66], JL | OPEN), ([(5, 1), (30, 101)] + lits(rnd, 10), JL)])
    runs["linked-not-joined"] = run_of([(a100, OPEN), ([(5, 1)] + lits(rnd, 20), LINKED | OPEN), ([(5, 1)] + lits(rnd, 20), JL | OPEN), (lits(rnd, 30), JL)])
    return runs


def linked_job_0():
    """A job list that opens with linked jobs nobody heads, a whole run behind them."""
    rnd = random.Random(5)
    return run_of([([(5, 1)] + lits(rnd, 20), JL | OPEN), (lits(rnd, 20), JL | OPEN), (lits(rnd, 64), OPEN), ([(9, 64)] + lits(rnd, 3), JL)])


def residue_runs():
    """Sixteen residues: the first unit has 160 + r bytes, the second opens with a match into it and ends off a 16-byte line."""
    rnd = random.Random(16)
    runs = []
    for r in range(16):
        n2 = 99 + 3 * r
        while n2 % 16 == 0 or (160 + r + n2) % 16 == 0:
            n2 += 1
        second = [(20, 50 + r)] + rep_tokens(rnd, n2 - 20 - 4) + [(4, 150 + r)]
        runs.append(run_of([(rep_tokens(rnd, 160 + r), OPEN), (second, JL)]))
    return runs


def tiles_run():
    """A chain across three place tiles: 60 whole streams, then seventy tiny linked units (jobs 60 .. 129)."""
    rnd = random.Random(70)
    jobs = [U(K.unit_final(K.repetitive(rnd, 20 + i)), 20 + i + i % 3, 0, False) for i in range(60)]
    specs = [(lits(rnd, 9), OPEN)]
    have = 9
    for k in range(1, 70):
        toks = [(3 + k % 5, 1 + (k * 7) % have)] + lits(rnd, k % 3)
        have += 3 + k % 5 + k % 3
        specs.append((toks, JL | (OPEN if k < 69 else 0), 3 + k % 5 + k % 3 + k % 2))
    return jobs + run_of(specs)


def sync_flush_stream(total=300000, every=40000, seed=300, wbits=-15):
    """(stream, plain): zlib's own output, text flushed with Z_SYNC_FLUSH every `every` bytes -- every piece sees the 32 KiB in front."""
    from swcompression_amd import corpus
    plain = corpus.p_text(total, seed)
    c = zlib.compressobj(6, zlib.DEFLATED, wbits)
    out = b""
    for o in range(0, total, every):
        out += c.compress(plain[o:o + every])
        if o + every < total:
            out += c.flush(zlib.Z_SYNC_FLUSH)
    return out + c.flush(), plain


def units_of_refs(stream, refs, cap):
    """The job list of swc_index_blocks kind 3: (offset, length, uncompressed length, aux) per unit."""
    return [U(stream[off:off + n], cap, aux, aux & OPEN) for off, n, _, aux in refs]
