"""AES-256-GCM sealing and opening (bw_seal.hip through the C ABI) against OpenSSL at the points
where the launch geometry, the item tables and the tag check can go wrong unnoticed by
tests/test_seal.py:

  1. more than 16,384 pieces in one call: k_seal_ctr's grid is capped at 1024 blocks of 16 waves,
     so a wave loops on to a piece of another item and rebuilds its LDS tables (the H^64 table that
     multi-block pieces use) in place; one item's pieces straddle the pass boundary;
  2. zero-length items anywhere in the table (they own no piece and share piece0 with their
     successor), and a batch of nothing but empty items;
  3. info_len 0..54 and several PRKs through k_seal_prep's one-block HMAC;
  4. every (src_off & 15, dst_off & 15) pair of the 16-byte vector loads and stores, with canaries
     after every output range, in the device and the host forms;
  5. tag verification under a tamper matrix (every tag byte, nonce, info, PRK, transplanted and
     truncated / extended items), with failures at ok indices on both sides of a 256-thread block;
  6. two asynchronous bw_seal_device calls in a row, the second regrowing the context's buffers.

The reference everywhere is the system OpenSSL (tests/openssl_ref.py) under the key
T(1) = HMAC-SHA-256(prk, info || 0x01) computed with Python's hmac: nothing of the project's own.
"""
import hashlib
import hmac

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PRK = bytes.fromhex("a5" * 32)
PIECE_BLOCKS = 8192          # bw_internal.h: 16-byte blocks per k_seal_ctr wave task
PIECE = PIECE_BLOCKS * 16
PASS_PIECES = 1024 * 16      # launch_seal: at most 1024 blocks of SEAL_THREADS / 64 = 16 waves
SRC_PAD, CANARY = 0x5A, 0xA5


def _ssl():
    try:
        import openssl_ref
        openssl_ref.lib()
        return openssl_ref
    except OSError:
        pytest.skip("OpenSSL libcrypto not available")


def _key(prk, info):
    """HKDF-Expand (RFC 5869) to 32 bytes: the one block T(1)."""
    return hmac.new(bytes(prk), bytes(info) + b"\x01", hashlib.sha256).digest()


def _blocks(n):
    return (int(n) + 15) // 16


def _pieces(n):
    return (_blocks(n) + PIECE_BLOCKS - 1) // PIECE_BLOCKS


class Layout:
    """Byte ranges of sizes[i] at off[i] in one buffer, each followed by at least `gap` bytes that
    belong to no range.  align[i] (optional) is off[i] & 15."""

    def __init__(self, sizes, align=None, gap=16):
        self.sizes = np.asarray(sizes, dtype=np.uint64)
        self.off = np.zeros(len(self.sizes), dtype=np.uint64)
        pos = 0
        for i, n in enumerate(self.sizes):
            if align is not None:
                pos += (int(align[i]) - pos) % 16
            self.off[i] = pos
            pos += int(n) + gap
        self.total = max(pos, 1)

    def fill(self, pad, chunks=None):
        buf = np.full(self.total, pad, dtype=np.uint8)
        if chunks is not None:
            for o, n, c in zip(self.off, self.sizes, chunks):
                assert len(c) == int(n)
                buf[int(o):int(o) + int(n)] = np.frombuffer(bytes(c), dtype=np.uint8)
        return buf

    def ranges(self, buf, pad):
        """The ranges' bytes, after asserting that every byte outside them still holds `pad`."""
        assert buf.size == self.total
        edge = np.zeros(self.total + 1, dtype=np.int8)
        off, end = self.off.astype(np.int64), (self.off + self.sizes).astype(np.int64)
        np.add.at(edge, off, 1)
        np.add.at(edge, end, -1)
        outside = np.cumsum(edge[:-1], dtype=np.int8) == 0
        hit = np.flatnonzero(outside & (buf != pad))
        if hit.size:
            owner = int(np.searchsorted(end, hit[0], side="right")) - 1
            raise AssertionError("%d gap bytes overwritten, first at %d (%d past the end of range %d, off & 15 = %d)"
                                 % (hit.size, hit[0], hit[0] - end[owner] if owner >= 0 else -1, owner,
                                    off[owner] & 15 if owner >= 0 else -1))
        return [buf[o:e].tobytes() for o, e in zip(off, end)]


def _run(ctx, form, prk, src, lsrc, infos, nonces, ldst, open_=False):
    """One seal / open call over the laid-out items into a canary-filled destination, through the
    device form (bw_seal_device / bw_open_device) or the host form (bw_seal / bw_open).  Returns the
    output buffer, the per-item output bytes (gaps checked) and the ok flags."""
    dst = ldst.fill(CANARY)
    if form == "host":
        r = ctx.seal(prk, src, lsrc.off, lsrc.sizes, infos, nonces, ldst.off, ldst.total, open_=open_, out=dst)
        out, ok = dst, (r[1] if open_ else None)
    else:
        import torch
        d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
        torch.cuda.synchronize()
        ok = ctx.seal_device(prk, d_src.data_ptr(), lsrc.off, lsrc.sizes, infos, nonces, d_dst.data_ptr(), ldst.off,
                             open_=open_)
        torch.cuda.synchronize()
        out = d_dst.cpu().numpy()
        assert np.array_equal(d_src.cpu().numpy(), src), "the source buffer was written"
    return out, ldst.ranges(out, CANARY), ok


def _mismatches(got, want):
    assert len(got) == len(want)
    return [i for i, (g, w) in enumerate(zip(got, want)) if g != w]


def _random_items(seed, lens, info_len=32):
    rng = np.random.default_rng(seed)
    pts = [rng.bytes(int(n)) for n in lens]
    infos = rng.integers(0, 256, (len(lens), info_len), dtype=np.uint8)
    nonces = rng.integers(0, 256, (len(lens), 12), dtype=np.uint8)
    return pts, infos, nonces


def _ssl_seal(ssl, prk, pts, infos, nonces):
    return [ssl.gcm_seal(_key(prk, infos[i]), bytes(nonces[i]), pts[i]) for i in range(len(pts))]


def _seal_and_open(ctx, ssl, form, prk, pts, infos, nonces, src_align=None, dst_align=None):
    """Seal against OpenSSL, then open the sealed buffer as it came out (canaries and all) back
    into the plaintext layout.  Returns (source layout, sealed layout, sealed buffer, sealed items)."""
    lens = [len(p) for p in pts]
    lp, ls = Layout(lens, src_align), Layout([n + 16 for n in lens], dst_align)
    want = _ssl_seal(ssl, prk, pts, infos, nonces)
    sealed_buf, got, _ = _run(ctx, form, prk, lp.fill(SRC_PAD, pts), lp, infos, nonces, ls)
    bad = _mismatches(got, want)
    assert not bad, ("seal", form, len(bad), [(i, lens[i]) for i in bad[:8]])
    _, plain, ok = _run(ctx, form, prk, sealed_buf, ls, infos, nonces, lp, open_=True)
    assert ok.tolist() == [1] * len(pts), ("open ok", form, np.flatnonzero(ok != 1)[:8].tolist())
    bad = _mismatches(plain, pts)
    assert not bad, ("open", form, len(bad), [(i, lens[i]) for i in bad[:8]])
    return lp, ls, sealed_buf, want


# ------------------------------------------------------------------ 1. more than one grid-stride pass

N_MANY, BIG_AT, CROSS_AT = 17200, 16300, 16376
RAGGED4 = 3 * PIECE + 16 * 100 + 5  # four pieces, the first of 101 blocks


def _many_piece_lens():
    lens = np.random.default_rng(101).integers(17, 4097, N_MANY)
    lens[BIG_AT:BIG_AT + 3] = [RAGGED4, 2 * PIECE, PIECE + 1]  # 4 + 2 + 2 pieces: 16,300 .. 16,307
    # 73 one-piece items follow (pieces 16,308 .. 16,380), so this one takes 16,381 .. 16,384
    lens[CROSS_AT] = RAGGED4
    return lens


def test_many_pieces_second_pass(ctx):
    ssl = _ssl()
    lens = _many_piece_lens()
    npc = np.array([_pieces(n) for n in lens])
    piece0 = np.concatenate(([0], np.cumsum(npc)[:-1]))
    assert int(npc.sum()) > PASS_PIECES
    assert piece0[BIG_AT] == BIG_AT and piece0[BIG_AT + 2] + npc[BIG_AT + 2] - 1 < PASS_PIECES  # all in the first pass
    straddle = [i for i in range(N_MANY) if piece0[i] < PASS_PIECES <= piece0[i] + npc[i] - 1]
    assert straddle == [CROSS_AT] and piece0[CROSS_AT] == 16381 and npc[CROSS_AT] == 4
    later_multi = [i for i in range(N_MANY) if piece0[i] >= PASS_PIECES and _blocks(lens[i]) >= 65]
    assert len(later_multi) >= 100  # second-pass waves whose rebuilt H^64 table is used (S >= 2)

    pts, infos, nonces = _random_items(102, lens)
    _, _, _, want = _seal_and_open(ctx, ssl, "device", PRK, pts, infos, nonces)
    # a small batch after the large one, on the same context
    k = 40
    ls = Layout([len(p) + 16 for p in pts[:k]])
    lp = Layout(lens[:k])
    _, got, _ = _run(ctx, "device", PRK, lp.fill(SRC_PAD, pts[:k]), lp, infos[:k], nonces[:k], ls)
    assert not _mismatches(got, want[:k])


# ------------------------------------------------------------------ 2. empty items

EMPTY_MIX = [0, 0, 5, 0, PIECE + 1, 0, 2 * PIECE, 0, 0, 16, 0]


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("lens,victim", [(EMPTY_MIX, 5), ([0] * 300, 277)], ids=["mixed", "all_empty"])
def test_empty_items(ctx, form, lens, victim):
    ssl = _ssl()
    assert lens[victim] == 0 and 0 < victim < len(lens) - 1
    pts, infos, nonces = _random_items(201 + len(lens), lens)
    lp, ls, sealed_buf, want = _seal_and_open(ctx, ssl, form, PRK, pts, infos, nonces)
    assert all(len(w) == 16 for w, n in zip(want, lens) if n == 0)  # an empty item's output is its tag
    # one flipped tag bit in one empty item: exactly that item fails
    bad = sealed_buf.copy()
    bad[int(ls.off[victim]) + 9] ^= 0x04
    tampered = bytes(bad[int(ls.off[victim]):int(ls.off[victim]) + 16])
    assert ssl.gcm_open(_key(PRK, infos[victim]), bytes(nonces[victim]), tampered) is None
    _, plain, ok = _run(ctx, form, PRK, bad, ls, infos, nonces, lp, open_=True)
    assert ok.tolist() == [int(i != victim) for i in range(len(lens))]
    assert not _mismatches(plain, pts)  # CTR output does not depend on the tag


# ------------------------------------------------------------------ 3. info_len and PRK

INFO_LENS = [0, 1, 2, 3, 4, 5, 6, 7, 31, 32, 33, 52, 53, 54]
_prk_rng = np.random.default_rng(301)
PRKS = [_prk_rng.bytes(32) for _ in range(3)] + [bytes([b]) * 32 for b in (0x00, 0xff, 0x36, 0x5c)]


@pytest.mark.parametrize("prk", PRKS, ids=["rand0", "rand1", "rand2", "00", "ff", "36", "5c"])
def test_info_len_and_prk(ctx, prk):
    ssl = _ssl()
    failed = []
    for il in INFO_LENS:
        pts, infos, nonces = _random_items(310 + il, [40] * 8, info_len=il)
        lp, ls = Layout([40] * 8), Layout([56] * 8)
        _, got, _ = _run(ctx, "host", prk, lp.fill(SRC_PAD, pts), lp, infos, nonces, ls)
        if _mismatches(got, _ssl_seal(ssl, prk, pts, infos, nonces)):
            failed.append(il)
    assert not failed, ("info_len", failed)


# ------------------------------------------------------------------ 4. alignment and canaries

ALIGN_LENS = [15, 16, 17, 47, 1030]  # 1030 bytes = 65 blocks: S = 2, ragged second half


@pytest.mark.parametrize("form", ["device", "host"])
def test_alignment_pairs_and_canaries(ctx, form):
    ssl = _ssl()
    combos = [(a, b, n) for a in range(16) for b in range(16) for n in ALIGN_LENS]
    pts, infos, nonces = _random_items(401, [n for _, _, n in combos])
    lp, ls, _, _ = _seal_and_open(ctx, ssl, form, PRK, pts, infos, nonces, src_align=[a for a, _, _ in combos],
                                  dst_align=[b for _, b, _ in combos])
    pairs = {(int(s) & 15, int(d) & 15) for s, d in zip(lp.off, ls.off)}
    assert len(pairs) == 256 and len(combos) == 1280


# ------------------------------------------------------------------ 5. tamper matrix

TAMPER_LENS = [0, 1, 16, 17, 1040, PIECE + 1, 2 * PIECE + 48]
OTHER_PRK = bytes.fromhex("c3" * 32)


def _flip(b, at, mask):
    b = bytearray(b)
    b[at] ^= mask
    return bytes(b)


def _tamper_batch(ssl):
    """-> (blobs, infos, nonces, plaintexts): the presented items; plaintexts[i] is None for a
    tampered item.  Tampered items sit at indices 0, 255, 256, 257 and the last."""
    rng = np.random.default_rng(505)
    bad, good = [], []
    for n in TAMPER_LENS:
        pt, info, nonce, info2, nonce2 = rng.bytes(n), rng.bytes(32), rng.bytes(12), rng.bytes(32), rng.bytes(12)
        blob = ssl.gcm_seal(_key(PRK, info), nonce, pt)
        by_info2 = ssl.gcm_seal(_key(PRK, info2), nonce, pt)
        by_nonce2 = ssl.gcm_seal(_key(PRK, info), nonce2, pt)
        good.append((blob, info, nonce, pt))

        def add(b, i=info, nc=nonce):
            bad.append((b, i, nc, None))

        for t in range(16):                       # every tag byte, one bit each
            add(_flip(blob, n + t, 1 << (t % 8)))
        for bit in range(8):                      # every bit of the first and the last tag byte
            add(_flip(blob, n, 1 << bit))
            add(_flip(blob, n + 15, 1 << bit))
        assert blob[n:] != bytes(16)
        add(blob[:n] + bytes(16))                 # tag zeroed
        add(blob[:n] + by_info2[n:])              # another item's valid tag
        add(by_info2)                             # valid under another info / another nonce
        add(by_nonce2)
        for k in range(12):
            add(blob, nc=_flip(nonce, k, 1 << (k % 8)))
        add(blob, i=_flip(info, 13, 0x10))
        if n:
            add(_flip(blob, 0, 0x01))
            add(_flip(blob, n - 1, 0x80))
            first = _blocks(n) - (_pieces(n) - 1) * PIECE_BLOCKS  # pieces are cut from the end
            for k in range(_pieces(n) - 1):       # both sides of every piece boundary
                at = 16 * (first + k * PIECE_BLOCKS)
                assert 0 < at < n
                add(_flip(blob, at - 1, 0x20))
                add(_flip(blob, at, 0x02))
            add(blob[:-1])                        # the last 16 bytes taken as the tag
            add(blob + b"\x77")                   # a stray byte: one more ciphertext byte, tag shifted
    assert sum(max(_pieces(n) - 1, 0) for n in TAMPER_LENS) == 3  # piece boundaries covered above
    while len(bad) + len(good) < 600:             # untouched small items
        pt, info, nonce = rng.bytes(int(rng.integers(0, 200))), rng.bytes(32), rng.bytes(12)
        good.append((ssl.gcm_seal(_key(PRK, info), nonce, pt), info, nonce, pt))
    total = len(bad) + len(good)
    forced = [0, 255, 256, 257, total - 1]
    rest = [i for i in range(total) if i not in forced]
    rng.shuffle(rest)
    rng.shuffle(bad)
    items = [None] * total
    for slot, it in zip(forced + rest, bad + good):
        items[slot] = it
    assert all(items[i][3] is None for i in forced)
    return tuple(list(col) for col in zip(*items))


def test_tamper_matrix(ctx):
    ssl = _ssl()
    blobs, infos, nonces, pts = _tamper_batch(ssl)
    n = len(blobs)
    assert n >= 600
    # the reference rejects every tampered item by itself, and accepts every untouched one
    for i in range(n):
        ref = ssl.gcm_open(_key(PRK, infos[i]), nonces[i], blobs[i])
        assert ref == pts[i], ("OpenSSL", i, len(blobs[i]))
    infos_a = np.frombuffer(b"".join(infos), dtype=np.uint8).reshape(n, 32)
    nonces_a = np.frombuffer(b"".join(nonces), dtype=np.uint8).reshape(n, 12)
    ls, lp = Layout([len(b) for b in blobs]), Layout([len(b) - 16 for b in blobs])
    src = ls.fill(SRC_PAD, blobs)
    _, plain, ok = _run(ctx, "device", PRK, src, ls, infos_a, nonces_a, lp, open_=True)
    want_ok = [int(p is not None) for p in pts]
    diff = [i for i in range(n) if ok[i] != want_ok[i]]
    assert ok.tolist() == want_ok, ("ok", len(diff), diff[:16])
    wrong = [i for i in range(n) if pts[i] is not None and plain[i] != pts[i]]
    assert not wrong, ("plaintext", wrong)
    # the whole batch under another PRK: nothing verifies
    for i in range(n):
        assert ssl.gcm_open(_key(OTHER_PRK, infos[i]), nonces[i], blobs[i]) is None
    _, _, ok = _run(ctx, "device", OTHER_PRK, src, ls, infos_a, nonces_a, lp, open_=True)
    assert ok.tolist() == [0] * n, ("other PRK", np.flatnonzero(ok).tolist())


# ------------------------------------------------------------------ 6. back-to-back asynchronous calls

def test_back_to_back_async_seal_device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ssl = _ssl()
    from backuwup_amd import Context
    batches = []
    for seed, lens in ((601, [100, 0, 17, 4096, 33, 1, 16, 2000, 64, 999]),
                       (602, np.random.default_rng(603).integers(17, 4097, 3000))):
        pts, infos, nonces = _random_items(seed, lens)
        lp, ls = Layout([len(p) for p in pts]), Layout([len(p) + 16 for p in pts])
        d_src = torch.from_numpy(lp.fill(SRC_PAD, pts)).cuda()
        d_dst = torch.from_numpy(ls.fill(CANARY)).cuda()
        batches.append((pts, infos, nonces, lp, ls, d_src, d_dst))
    torch.cuda.synchronize()
    with Context(0) as c:
        for pts, infos, nonces, lp, ls, d_src, d_dst in batches:  # no synchronisation in between
            c.seal_device(PRK, d_src.data_ptr(), lp.off, lp.sizes, infos, nonces, d_dst.data_ptr(), ls.off)
        torch.cuda.synchronize()
        for pts, infos, nonces, lp, ls, d_src, d_dst in batches:
            got = ls.ranges(d_dst.cpu().numpy(), CANARY)
            bad = _mismatches(got, _ssl_seal(ssl, PRK, pts, infos, nonces))
            assert not bad, (len(pts), len(bad), bad[:8])
