"""bw_reseal_device / bw_reseal (k_reseal_ctr, k_reseal_tag: one pass from the ciphertext under one PRK
to the ciphertext under another, no plaintext stored) against tests/rekey_ref.py, byte for byte: the
outputs, ok, canaries around every output range, and the source, which must come back untouched.
Every case runs through the device and the host form."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

A, B = bytes.fromhex("5c" * 32), bytes.fromhex("3e" * 32)
PIECE_BLOCKS = 8192          # bw_internal.h: 16-byte blocks per k_reseal_ctr wave task
PIECE = PIECE_BLOCKS * 16
PASS_PIECES = 16384          # launch_reseal: a grid pass covers 16,384 pieces
CANARY = 0xC3


@pytest.fixture(scope="module")
def rk():
    try:
        import openssl_ref
        openssl_ref.lib()
    except OSError:
        pytest.skip("OpenSSL libcrypto not available")
    import rekey_ref

    class NS:
        pass
    ns = NS()
    ns.ref, ns.ssl = rekey_ref, openssl_ref
    return ns


def _items(rk, seed, lens, info_len=32, prk=A):
    """Sealed by OpenSSL under prk: (sealed [bytes], infos n x info_len, nonces n x 12, new nonces n x 12)."""
    rng = np.random.default_rng(seed)
    n = len(lens)
    infos = rng.integers(0, 256, (n, info_len), dtype=np.uint8)
    nonces = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    new_nonces = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    sealed = [rk.ssl.gcm_seal(rk.ref.key(prk, infos[i]), bytes(nonces[i]), rng.bytes(int(m))) for i, m in enumerate(lens)]
    return sealed, infos, nonces, new_nonces


def _layout(sizes, align=None, gap=24):
    """Offsets of ranges of the given sizes in one buffer, range i at off & 15 == align[i], gaps between."""
    off, pos = [], gap
    for i, m in enumerate(sizes):
        if align is not None:
            pos += (int(align[i]) - pos) % 16
        off.append(pos)
        pos += int(m) + gap
    return np.array(off, dtype=np.uint64), pos


def _fill(sealed, off, total):
    buf = np.full(total, CANARY, dtype=np.uint8)
    for o, s in zip(off, sealed):
        buf[int(o):int(o) + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return buf


def _reseal(ctx, rk, buf, off, slen, infos, nonces, new_nonces=None, dst_align=None, old=A, new=B, want=None):
    """Both forms over the same tables against rekey_ref: returns (ok, outputs [bytes]).  want: the
    reference's (outputs, ok) when the caller has them already."""
    import torch
    from backuwup_amd import rekey
    slen = np.asarray(slen, dtype=np.uint64)
    n = len(slen)
    if want is None:
        ref = [rk.ref.reseal_item(old, new, infos[i], bytes(nonces[i]), buf[int(off[i]):int(off[i]) + int(slen[i])].tobytes(),
                                  None if new_nonces is None else bytes(new_nonces[i])) for i in range(n)]
        want = [r[0] for r in ref], [r[1] for r in ref]
    dst_off, total = _layout(slen, align=dst_align, gap=19)
    expect = _fill(want[0], dst_off, total)
    before = buf.copy()
    out = np.full(total, CANARY, dtype=np.uint8)
    got, ok_h = rekey.reseal(ctx, old, new, buf, off, slen, infos, nonces, dst_off, total, new_nonces=new_nonces, out=out)
    assert np.array_equal(buf, before), "bw_reseal wrote the host source"
    d_src = torch.from_numpy(buf).cuda()
    d_dst = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    ok_d = rekey.reseal_device(ctx, old, new, d_src.data_ptr(), off, slen, infos, nonces, d_dst.data_ptr(), dst_off,
                               new_nonces=new_nonces)
    torch.cuda.synchronize()
    assert np.array_equal(d_src.cpu().numpy(), before), "bw_reseal_device wrote the source buffer"
    for name, o, ok in (("bw_reseal", got, ok_h), ("bw_reseal_device", d_dst.cpu().numpy(), ok_d)):
        assert ok.tolist() == want[1], (name, [i for i in range(n) if ok[i] != want[1][i]][:8])
        bad = np.flatnonzero(o != expect)
        assert not bad.size, (name, "first differing byte", int(bad[0]), "item",
                              int(np.searchsorted(dst_off, bad[0], side="right")) - 1, "of", n)
    return want[1], want[0]


LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 64 * 16 - 1, 64 * 16 + 1, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 17,
           3 * 1024 * 1024]


@pytest.mark.parametrize("new_nonces", [False, True])
def test_lengths_around_every_boundary(ctx, rk, new_nonces):
    sealed, infos, nonces, nn = _items(rk, 301, LENGTHS)
    assert [len(s) for s in sealed] == [16 + m for m in LENGTHS] and len(sealed[-1]) == 3 * 1024 * 1024 + 16
    off, total = _layout([len(s) for s in sealed], align=[(5 * i + 3) % 16 for i in range(len(sealed))])
    ok, outs = _reseal(ctx, rk, _fill(sealed, off, total), off, [len(s) for s in sealed], infos, nonces,
                       new_nonces=nn if new_nonces else None, dst_align=[(7 * i + 1) % 16 for i in range(len(sealed))])
    assert ok == [1] * len(LENGTHS)
    for i, o in enumerate(outs):  # the reference's output is what OpenSSL opens under the new key
        assert rk.ssl.gcm_open(rk.ref.key(B, infos[i]), bytes((nn if new_nonces else nonces)[i]), o) is not None


def test_every_pair_of_source_and_destination_alignment(ctx, rk):
    lens = [16 + 1000 + 17] * 256  # ragged: 63 full blocks and 9 bytes
    sealed, infos, nonces, nn = _items(rk, 302, [m - 16 for m in lens])
    off, total = _layout(lens, align=[i & 15 for i in range(256)], gap=5)
    ok, _ = _reseal(ctx, rk, _fill(sealed, off, total), off, lens, infos, nonces, new_nonces=nn,
                    dst_align=[i >> 4 for i in range(256)])
    assert ok == [1] * 256


def test_more_pieces_than_one_grid_pass(ctx, rk):
    """16,380 items of one piece, then one of six pieces that straddles the pass border, then more small ones."""
    lens = np.random.default_rng(303).integers(16, 40, 16500)
    lens[16380] = 5 * PIECE + 333
    assert int(lens[:16380].astype(bool).sum()) == 16380 < PASS_PIECES < 16380 + 6
    sealed, infos, nonces, nn = _items(rk, 303, lens)
    slen = [len(s) for s in sealed]
    off, total = _layout(slen, gap=3)
    buf = _fill(sealed, off, total)
    want = [1] * len(lens)
    for i in (0, 255, 256, 8191, 16379, 16380, 16381, 16499):
        buf[int(off[i]) + 5] ^= 2
        want[i] = 0
    ok, _ = _reseal(ctx, rk, buf, off, slen, infos, nonces, new_nonces=nn)
    assert ok == want


@pytest.mark.parametrize("lens", [[0], [0, 0, 0], [0, 40, 70000], [40, 70000, 0], [33, 0, 0, 200, 0, PIECE + 5, 0]])
def test_empty_items_anywhere(ctx, rk, lens):
    sealed, infos, nonces, nn = _items(rk, 304, lens)
    slen = [len(s) for s in sealed]
    off, total = _layout(slen)
    assert _reseal(ctx, rk, _fill(sealed, off, total), off, slen, infos, nonces, new_nonces=nn)[0] == [1] * len(lens)


def test_no_items(ctx, rk):
    from backuwup_amd import rekey
    out, ok = rekey.reseal(ctx, A, B, np.zeros(8, np.uint8), [], [], [], [], [], 0)
    assert ok.size == 0 and out.size == 0
    assert rekey.reseal_device(ctx, A, B, 0, [], [], [], [], 0, []).size == 0


@pytest.mark.parametrize("info_len", [5, 6, 32, 54])
def test_info_lengths(ctx, rk, info_len):
    lens = [0, 31, 500, PIECE + 40]
    sealed, infos, nonces, nn = _items(rk, 305 + info_len, lens, info_len=info_len)
    slen = [len(s) for s in sealed]
    off, total = _layout(slen)
    assert _reseal(ctx, rk, _fill(sealed, off, total), off, slen, infos, nonces, new_nonces=nn)[0] == [1] * 4
    assert _reseal(ctx, rk, _fill(sealed, off, total), off, slen, infos, nonces)[0] == [1] * 4


def test_same_prk_and_kept_nonces_return_the_input(ctx, rk):
    lens = [0, 7, 16, 4000, PIECE + 1]
    sealed, infos, nonces, _ = _items(rk, 306, lens)
    slen = [len(s) for s in sealed]
    off, total = _layout(slen)
    ok, outs = _reseal(ctx, rk, _fill(sealed, off, total), off, slen, infos, nonces, new=A, want=(sealed, [1] * 5))
    assert ok == [1] * 5 and outs == sealed


def test_tamper_matrix(ctx, rk):
    """One case per kind of damage, spread over 300 items so that neighbours lie across a 256-item border:
    ok is 0, OpenSSL rejects the output under the new key, and it opens every neighbour."""
    two = PIECE + 100                      # two pieces: the first holds 7 blocks
    boundary = 16 * ((two + 15) // 16 - PIECE_BLOCKS)
    n = 300
    lens = [100] * n
    at = {"ct first": 3, "ct last": 9, "piece boundary": 14, "nonce": 20, "info": 27, "truncated": 33, "extended": 40,
          "near border": 255, "past border": 257}
    tags = {("tag", b): 50 + 3 * b for b in range(16)}
    for i in (at["ct first"], at["ct last"], at["piece boundary"]):
        lens[i] = two
    sealed, infos, nonces, nn = _items(rk, 307, lens)
    slen = np.array([len(s) for s in sealed], dtype=np.uint64)
    off, total = _layout(slen)
    buf = _fill(sealed, off, total)
    infos, nonces = infos.copy(), nonces.copy()
    for (_, b), i in tags.items():
        buf[int(off[i]) + 100 + b] ^= 1 << (b % 8)
    buf[int(off[at["ct first"]])] ^= 1
    buf[int(off[at["ct last"]]) + two - 1] ^= 0x80
    buf[int(off[at["piece boundary"]]) + boundary] ^= 8
    nonces[at["nonce"], 11] ^= 1
    infos[at["info"], 0] ^= 1
    slen[at["truncated"]] -= 1
    slen[at["extended"]] += 1            # a canary byte joins the item
    buf[int(off[at["near border"]]) + 50] ^= 4
    buf[int(off[at["past border"]]) + 50] ^= 4
    damaged = set(at.values()) | set(tags.values())
    ok, outs = _reseal(ctx, rk, buf, off, slen, infos, nonces, new_nonces=nn)
    assert ok == [int(i not in damaged) for i in range(n)]
    for i in range(n):
        opened = rk.ssl.gcm_open(rk.ref.key(B, infos[i]), bytes(nn[i]), outs[i])
        assert (opened is None) == (i in damaged), i
    # a wrong old PRK: nothing is authentic, and nothing comes out authentic
    clean, ci, cn, cnn = _items(rk, 308, [0, 50, two])
    clen = [len(s) for s in clean]
    coff, ctot = _layout(clen)
    wrong = bytes.fromhex("5d" + "5c" * 31)
    ok, outs = _reseal(ctx, rk, _fill(clean, coff, ctot), coff, clen, ci, cn, new_nonces=cnn, old=wrong)
    assert ok == [0, 0, 0]
    assert all(rk.ssl.gcm_open(rk.ref.key(B, ci[i]), bytes(cnn[i]), outs[i]) is None for i in range(3))


def test_refusals(ctx, rk):
    from backuwup_amd import _lib, rekey
    import torch
    buf = np.zeros(256, dtype=np.uint8)
    z32, z12 = np.zeros((2, 32), np.uint8), np.zeros((2, 12), np.uint8)
    d = torch.zeros(512, dtype=torch.uint8, device="cuda")
    cases = [([0, 20], [16, 15], [0, 64]),        # shorter than a tag
             ([0, 64], [40, 40], [0, 39]),        # outputs overlap by one byte
             ([0, 64], [40, 40], [100, 100])]     # the same output twice
    for so, sl, do in cases:
        with pytest.raises(_lib.BwError) as x:
            rekey.reseal(ctx, A, B, buf, so, sl, z32, z12, do, 256)
        assert x.value.rc == _lib.BW_EINVAL
        with pytest.raises(_lib.BwError) as x:
            rekey.reseal_device(ctx, A, B, d.data_ptr(), so, sl, z32, z12, d.data_ptr() + 256, do)
        assert x.value.rc == _lib.BW_EINVAL
    with pytest.raises(_lib.BwError) as x:            # an output over a source range
        rekey.reseal_device(ctx, A, B, d.data_ptr(), [0, 64], [40, 40], z32, z12, d.data_ptr(), [200, 100])
    assert x.value.rc == _lib.BW_EINVAL
    torch.cuda.synchronize()
    assert not d.cpu().numpy().any(), "a refused call wrote device memory"
