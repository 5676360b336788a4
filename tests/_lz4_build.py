"""LZ4 blocks built sequence by sequence (LZ4 block format; the reference's reader: Sources/LZ4/LZ4.swift:332-413), so that a
test can write what liblz4 never emits: a first sequence that reaches in front of the block, an offset one byte too far, a
block of a handful of bytes.  TEST INFRASTRUCTURE ONLY.  The builder does not check anything: what it writes may be invalid
on purpose, and what a block decodes to is the oracle's to say."""


def _length(n):
    """The extension bytes of a length whose token nibble is 15 (n = length - 15)."""
    out = bytearray()
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)
    return bytes(out)


def sequence(literals, offset=None, match_len=None):
    """One sequence: the literals, then a match of match_len bytes (>= 4) `offset` back; offset None = the block's last sequence."""
    literals = bytes(literals)
    ll = len(literals)
    ml = 0 if offset is None else match_len - 4
    assert ml >= 0
    out = bytearray([(min(ll, 15) << 4) | min(ml, 15)])
    if ll >= 15:
        out += _length(ll - 15)
    out += literals
    if offset is not None:
        out += bytes([offset & 0xFF, (offset >> 8) & 0xFF])
        if ml >= 15:
            out += _length(ml - 15)
    return bytes(out)


def block(sequences, last_literals=b""):
    """sequences: list of (literals, offset, match_len); last_literals: the literals of the closing sequence (None: no closing
    sequence -- the block ends behind a match, which the format forbids)."""
    out = b"".join(sequence(*s) for s in sequences)
    if last_literals is not None:
        out += sequence(last_literals)
    return out
