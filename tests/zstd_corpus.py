"""Deterministic blob corpus for the zstd level-3 tests (test data, generated; no reference
content).  Each kind exercises a different part of the compressor: Huffman literals of skewed
text, dense short matches (thousands of sequences per block, FSE tables with low-probability
symbols), long-distance repeats across a window larger than 2 MiB, long runs (match lengths over
64 KiB, RLE blocks), random bytes (raw blocks) and tiny blobs."""
import random

import numpy as np

KINDS = ("text", "tokens", "repeats", "runs", "random", "mixed")


def blob(kind, n, seed):
    r = random.Random(seed * 1000003 + KINDS.index(kind))
    g = np.random.default_rng(seed * 7 + KINDS.index(kind))
    if kind == "text":
        p = g.dirichlet(np.ones(48) * 0.35)
        words = [bytes((g.choice(48, size=int(g.integers(1, 9)), p=p) + 40).astype(np.uint8))
                 for _ in range(int(g.integers(8, 600)))]
        b = bytearray()
        while len(b) < n:
            b += words[int(g.integers(len(words)))] + b" "
        return bytes(b[:n])
    if kind == "tokens":
        toks = [r.randbytes(r.randrange(4, 7)) for _ in range(r.randrange(2, 64))]
        parts, size = [], 0
        while size < n:
            t = toks[r.randrange(len(toks))]
            if r.random() < 0.3:
                t += bytes([r.randrange(256)])
            parts.append(t)
            size += len(t)
        return b"".join(parts)[:n]
    if kind == "repeats":
        base = r.randbytes(r.randrange(1000, 300000))
        b = bytearray()
        while len(b) < n:
            s = r.randrange(len(base))
            b += base[s:s + r.randrange(100, 200000)]
            if r.random() < 0.3:
                b += r.randbytes(r.randrange(1, 50))
        return bytes(b[:n])
    if kind == "runs":
        b = bytearray()
        while len(b) < n:
            b += bytes([r.randrange(3)]) * r.randrange(1, 400000)
            b += r.randbytes(r.randrange(0, 100))
        return bytes(b[:n])
    if kind == "random":
        return r.randbytes(n)
    b = bytearray()
    while len(b) < n:
        k = r.randrange(3)
        if k == 0:
            b += r.randbytes(r.randrange(1, 3000))
        elif k == 1 and b:
            s = r.randrange(len(b))
            b += b[s:s + r.randrange(4, 5000)]
        else:
            b += bytes([r.randrange(256)]) * r.randrange(1, 2000)
    return bytes(b[:n])


def corpus(sizes, seed=0):
    """[(kind, n, bytes)] for every kind at every size."""
    return [(k, n, blob(k, n, seed + i)) for i, n in enumerate(sizes) for k in KINDS]


# ------------------------------------------------------------------ edge kinds
# Blobs built to reach the frame modes the kinds above never do (tests/test_zstd.py, the census,
# names every mode and which of these reach it).  A separate tuple: the seeds of the kinds above
# depend on KINDS.index, and the tests parametrised over KINDS keep their cases.
#   skew_narrow / skew_mid / skew_wide   i.i.d. bytes, sums of four uniform draws (15, 32 and 256 values):
#       almost no matches, so a block is one Huffman literal section of about n bytes -- literal
#       counts at the 1-stream and header-width thresholds, the 5-byte header, blocks with no
#       sequences; the narrow alphabet's Huffman weights are written direct.
#   rle_lits    a random block, then matches into it separated by one repeated byte: RLE literals.
#   one_code    a random block, then sequences that share one LL, OF or ML code: RLE table modes.
#   mispredict  a compressible block, one or two blocks that stay uncompressed although they parse
#       into sequences (random with two short repeats: raw; one byte: RLE), then a block whose first
#       match is the repeat offset from before the gap, and whose literals reuse the Huffman table.
#   seqflood    a random block, then four-byte matches alternating between two offsets with no
#       literals: over 0x7F00 sequences in one block (the 3-byte sequence count).
#   far         60,000 bytes repeated more than 1 MiB on, after 70,000 literals of the last block: offset
#       code 20 and literal-length code 35.
#   longmatch   one period repeated to the end: a single match of over 65,538 bytes (match-length code 52).
#   fse_follow  a block with FSE-coded tables, then a short block of the same statistics (where an
#       encoder that kept FSE tables across blocks would write repeat mode; level 3 does not).
EDGE_KINDS = ("skew_narrow", "skew_mid", "skew_wide", "rle_lits", "one_code", "mispredict", "seqflood", "fse_follow", "far",
              "longmatch")
BLOCK = 128 * 1024


def _skew(r, n, kind):
    a = np.frombuffer(r.randbytes(4 * n), np.uint8).reshape(n, 4).astype(np.uint16)
    if kind == "skew_narrow":
        return ((a & 7).sum(1) >> 1).astype(np.uint8).tobytes()
    if kind == "skew_mid":
        return ((a & 31).sum(1) >> 2).astype(np.uint8).tobytes()
    return (a.sum(1) >> 2).astype(np.uint8).tobytes()


def _periodic(r, n, p):
    """n bytes of period p (skewed bytes) with a changed byte every few hundred."""
    b = bytearray((_skew(r, p, "skew_wide") * (n // p + 1))[:n])
    i = p + r.randrange(50, 400)
    while i < n - 50:
        b[i] = _skew(r, 1, "skew_wide")[0]
        i += r.randrange(200, 900)
    return b


def edge_blob(kind, n, seed):
    """One edge blob; n is its length, or for rle_lits and one_code the length it grows past."""
    r = random.Random(seed * 1000003 + 100 + EDGE_KINDS.index(kind))
    if kind.startswith("skew_"):
        return _skew(r, n, kind)
    if kind == "fse_follow":
        return blob("tokens", n, seed)
    if kind == "longmatch":
        p = r.randrange(40, 300)
        return (_skew(r, p, "skew_wide") * (n // p + 1))[:n]
    if kind == "far":
        # 60,000 bytes again after more than 1 MiB, 70,000 literals into the last block
        b = _skew(r, n - 60000, "skew_wide")
        return b + b[:60000]
    if kind == "mispredict":
        small = seed % 8 >= 4  # under 256 literals in the last block: one Huffman stream
        p = r.randrange(40, 120 if small else 300)
        b = bytearray(_skew(r, 16000, "skew_wide")) + _periodic(r, BLOCK - 16000, p)
        for middle in ((("raw",), ("rle",), ("raw", "rle"), ("rle", "raw"))[seed % 4]):
            if middle == "raw":  # two 12-byte repeats: sequences, new repeat offsets, and no gain
                m = bytearray(r.randbytes(BLOCK))
                m[100:112] = m[20:32]
                m[300:312] = m[150:162]
                b += m
            else:
                b += bytes([r.randrange(256)]) * BLOCK
        b += _skew(r, 70 if small else 250, "skew_wide")
        return bytes(b + _periodic(r, n - len(b), p))
    # the rest: a random block, then about n - BLOCK bytes that copy pieces of its first 16 KiB (where the
    # match finder's skip is still short, so a piece of 140 bytes or more is found), no piece twice
    R = r.randbytes(BLOCK)
    b = bytearray(R)
    if kind == "rle_lits":
        z, s = r.randrange(256), 1
        while len(b) < n and s < 16000:
            ln = r.randrange(140, 200)
            b += R[s:s + ln] + (bytes([z]) * r.randrange(1, 4) if len(b) + ln < n else b"")
            s += ln + r.randrange(1, 9)
        return bytes(b)
    if kind == "one_code":
        fixed = ("ll", "of", "ml") if seed % 4 == 0 else (("ll", "of", "ml")[seed % 4 - 1],)
        lo, hi = 1, 16000
        while len(b) < n and lo + 600 < hi:
            b += r.randbytes(r.randrange(70, 120) if "ll" in fixed else r.randrange(1, 200))
            ln = r.randrange(140, 250) if "ml" in fixed else r.randrange(140, 600)
            if "of" in fixed or r.random() < 0.5:  # distances of 128 KiB and more
                b += R[lo:lo + ln]
                lo += ln + 1
            else:                                  # and under 128 KiB
                hi -= ln + 1
                b += R[hi:hi + ln]
        return bytes(b)
    if kind == "seqflood":
        # every four bytes continue the copy at one of two offsets and break the other's (one byte more
        # where the two sources agree)
        b += R[10:18] + R[100:108]
        off = (BLOCK - 10, BLOCK + 8 - 100)
        use = 0
        while len(b) < n - 8:
            for _ in range(4):
                b.append(b[len(b) - off[use]])
            while len(b) < n and b[len(b) - off[use]] == b[len(b) - off[1 - use]]:
                b.append(b[len(b) - off[use]])
            use = 1 - use
        while len(b) < n:
            b.append(b[len(b) - off[use]])
        return bytes(b[:n])
    raise ValueError(kind)


# (kind, n, seed): found by search with the oracle and tests/zstd_frames.py; the census test fails
# if an edit here (or to the generators) loses a class.
EDGE_CASES = (
    # Huffman literal counts at 255 / 256 (one stream below 256), 1,023 / 1,024 and 16,383 / 16,384 (header
    # widths); direct Huffman weights (narrow, mid); blocks with no sequences and the 5-byte header (wide)
    ("skew_narrow", 288, 0), ("skew_narrow", 263, 1), ("skew_narrow", 289, 0), ("skew_narrow", 264, 1),
    ("skew_mid", 1032, 0), ("skew_mid", 1035, 1), ("skew_mid", 1033, 0), ("skew_mid", 1036, 1),
    ("skew_mid", 16387, 2), ("skew_mid", 16404, 4), ("skew_mid", 16388, 2), ("skew_mid", 16405, 4),
    ("skew_wide", 16383, 0), ("skew_wide", 16383, 1), ("skew_wide", 16384, 0), ("skew_wide", 16384, 1),
    ("skew_wide", BLOCK, 0), ("skew_wide", 200000, 1),
    ("rle_lits", BLOCK + 12000, 0), ("rle_lits", BLOCK + 12000, 1),
) + tuple(("one_code", BLOCK + 6000, s) for s in range(8)) + tuple(
    ("mispredict", BLOCK * (2 + (s % 4 > 1)) + 3000, s) for s in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 14)) + (
    ("seqflood", 2 * BLOCK, 0), ("seqflood", 2 * BLOCK, 1),
    ("fse_follow", BLOCK + 20000, 0), ("fse_follow", BLOCK + 20000, 1),
    ("far", 9 * BLOCK + 130000, 0), ("far", 9 * BLOCK + 130000, 1),
    ("longmatch", 100000, 0), ("longmatch", BLOCK + 70000, 1),
)


def edge_corpus():
    """[(kind, n, seed, bytes)] for every edge case."""
    return [(k, n, s, edge_blob(k, n, s)) for k, n, s in EDGE_CASES]
