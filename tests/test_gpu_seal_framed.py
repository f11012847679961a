"""Store-framed sealing (k_seal_ctr<false, true> in bw_seal.hip, reached through Context.pack_build
with its default flags) at the raw lengths where a 16-byte AES block meets the frame's structure.

The plaintext of a framed item is never in memory: k_seal_ctr builds the zstd store frame (2 bytes
of frame header, then raw blocks of at most 128 KiB behind 3-byte block headers) from the raw bytes
while it encrypts.  A block that lies inside one raw block's data is one unaligned 16-byte load;
every other block (the first, one that straddles a block header, the ragged last) is assembled byte
by byte.  With the 5 bytes of frame and first block header, the lengths below put the item's end
before, on and after a 16-byte boundary (11 raw bytes are one full block), and before, on and after
the second and third block headers; 3 MiB is the largest blob (24 raw blocks, 25 pieces).  One
length, whose second block header straddles two AES blocks, runs at every source byte alignment.

The reference is oracle/pack_oracle.py (zstd_store, seal_blob_payload, write_packfiles), byte for
byte over the whole output.
"""
import numpy as np
import pytest

from backuwup_amd.synth import splitmix_bytes

pytestmark = pytest.mark.gpu

PRK = bytes.fromhex("3d" * 32)
KIB = 1024
RAW_LENS = [0, 1, 11, 12, 13, 14, 15, 128 * KIB - 1, 128 * KIB, 128 * KIB + 1, 128 * KIB + 13, 256 * KIB + 3,
            3 * KIB * KIB]
ALIGN_LEN = 128 * KIB + 13


@pytest.fixture(scope="module")
def po(oracle):
    from oracle import pack_oracle
    return pack_oracle


def _check(ctx, po, seed, lens, aligns):
    """lens[i] raw bytes at a source offset with off & 15 == aligns[i], packed with store frames,
    against the oracle's packfiles."""
    rng = np.random.default_rng(seed)
    n = len(lens)
    datas = [splitmix_bytes(seed * 100 + i, int(m)).tobytes() for i, m in enumerate(lens)]
    hashes = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    kinds = rng.integers(0, 2, n).astype(np.uint8)
    nonces = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    offs, pos = [], 0
    for m, a in zip(lens, aligns):
        pos += (a - pos) % 16
        offs.append(pos)
        pos += m
    assert [o & 15 for o in offs] == list(aligns)
    src = np.full(max(pos, 1), 0xEE, dtype=np.uint8)
    for o, d in zip(offs, datas):
        src[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    plan, total = ctx.pack_plan(np.asarray(lens, dtype=np.uint64))
    ids = rng.integers(0, 256, (len(plan), 12), dtype=np.uint8)
    got = ctx.pack_build(PRK, src, offs, lens, hashes, kinds, nonces, plan, total, ids)
    blobs = [(bytes(hashes[i]), int(kinds[i]), bytes(nonces[i]),
              po.seal_blob_payload(PRK, hashes[i], nonces[i], po.zstd_store(d))) for i, d in enumerate(datas)]
    assert [len(b[3]) for b in blobs] == [po.zstd_store_size(m) + 16 for m in lens]
    want = po.write_packfiles(PRK, blobs, [bytes(x) for x in ids])
    assert len(want) == len(plan) and sum(len(b) for _, b in want) == total
    for k, (p, (_, buf)) in enumerate(zip(plan, want)):
        have = got[int(p["offset"]):int(p["offset"] + p["size"])].tobytes()
        if have != buf:
            a, b = np.frombuffer(have, dtype=np.uint8), np.frombuffer(buf, dtype=np.uint8)
            bad = np.flatnonzero(a != b) if a.size == b.size else []
            raise AssertionError("packfile %d (blobs %d..%d): %d of %d bytes differ, first at %s"
                                 % (k, p["first_blob"], p["first_blob"] + p["n_blobs"] - 1, len(bad), len(buf),
                                    bad[:4].tolist() if len(bad) else "(sizes %d, %d)" % (a.size, b.size)))


def test_framed_lengths(ctx, po):
    # frame bytes = 2 + 3 per raw block + raw bytes: the ends fall on 5, 6, 16, 17, ... and the
    # second block header starts at frame byte 131077 = 16 * 8192 + 5
    assert [po.zstd_store_size(m) % 16 for m in RAW_LENS[:7]] == [5, 6, 0, 1, 2, 3, 4]
    assert [po.zstd_store_size(m) for m in RAW_LENS[7:10]] == [131076, 131077, 131081]
    _check(ctx, po, 11, RAW_LENS, [(3 * i + 1) % 16 for i in range(len(RAW_LENS))])


def test_framed_every_source_alignment(ctx, po):
    _check(ctx, po, 12, [ALIGN_LEN] * 16, list(range(16)))
