"""bw_auth_device / bw_auth (k_seal_auth: AES-GCM tags recomputed from the ciphertext, nothing decrypted)
against the system OpenSSL's accept / reject (tests/openssl_ref.py, key = HKDF-Expand by Python's hmac)
and, beside it, against bw_open_device's ok on the same tables.  Every case runs through the device
and the host form; the source buffer, canaries around every item included, must come back untouched."""
import hashlib
import hmac
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

PRK = bytes.fromhex("5c" * 32)
PIECE_BLOCKS = 8192          # bw_internal.h: 16-byte blocks per k_seal_auth wave task
PIECE = PIECE_BLOCKS * 16
PASS_PIECES = 16384          # launch_seal: a grid pass of k_seal_auth covers 16,384 pieces, whatever its workgroup size
CANARY = 0xC3


def _ssl():
    try:
        import openssl_ref
        openssl_ref.lib()
        return openssl_ref
    except OSError:
        pytest.skip("OpenSSL libcrypto not available")


def _key(prk, info):
    return hmac.new(bytes(prk), bytes(info) + b"\x01", hashlib.sha256).digest()  # HKDF-Expand (RFC 5869), one block


def _items(ssl, seed, lens, prk=PRK):
    """Sealed by OpenSSL: (sealed [bytes], infos n x 32, nonces n x 12)."""
    rng = np.random.default_rng(seed)
    infos = rng.integers(0, 256, (len(lens), 32), dtype=np.uint8)
    nonces = rng.integers(0, 256, (len(lens), 12), dtype=np.uint8)
    sealed = [ssl.gcm_seal(_key(prk, infos[i]), bytes(nonces[i]), rng.bytes(int(n))) for i, n in enumerate(lens)]
    return sealed, infos, nonces


def _layout(sealed, align=None, gap=24):
    """The items in one canary-filled buffer, item i at an offset with off & 15 == align[i], gaps between."""
    off, pos = [], gap
    for i, s in enumerate(sealed):
        if align is not None:
            pos += (int(align[i]) - pos) % 16
        off.append(pos)
        pos += len(s) + gap
    buf = np.full(pos, CANARY, dtype=np.uint8)
    for o, s in zip(off, sealed):
        buf[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return buf, np.array(off, dtype=np.uint64)


def _verdicts(ctx, ssl, buf, off, lens, infos, nonces, prk=PRK):
    """ok by bw_auth (host), bw_auth_device, bw_open_device and OpenSSL over the same tables; the three
    library answers must each equal OpenSSL's, and the source must come back byte for byte."""
    import torch
    from backuwup_amd import check
    lens = np.asarray(lens, dtype=np.uint64)
    want = np.array([ssl.gcm_open(_key(prk, infos[i]), bytes(nonces[i]), buf[int(o):int(o) + int(n)].tobytes()) is not None
                     for i, (o, n) in enumerate(zip(off, lens))], dtype=np.uint8)
    before = buf.copy()
    host = check.auth(ctx, prk, buf, off, lens, infos, nonces)
    assert np.array_equal(buf, before), "bw_auth wrote the host source"
    d = torch.from_numpy(buf).cuda()
    dev = check.auth_device(ctx, prk, d.data_ptr(), off, lens, infos, nonces)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), before), "bw_auth_device wrote the source buffer or a canary"
    dst_off = np.concatenate(([0], np.cumsum((lens - 16 + 31) // 16 * 16)[:-1])).astype(np.uint64)
    d_dst = torch.empty(int(dst_off[-1] + lens[-1] + 64) if len(lens) else 64, dtype=torch.uint8, device="cuda")
    opened = ctx.seal_device(prk, d.data_ptr(), off, lens, infos, nonces, d_dst.data_ptr(), dst_off, open_=True)
    for name, got in (("bw_auth", host), ("bw_auth_device", dev), ("bw_open_device", opened)):
        bad = np.flatnonzero(got != want)
        assert not bad.size, (name, bad[:8].tolist(), [int(lens[i]) for i in bad[:8]])
    return want


LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 64 * 16 - 1, 64 * 16 + 1, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 17,
           3 * 1024 * 1024 + 16]


def test_lengths_around_every_boundary(ctx):
    ssl = _ssl()
    sealed, infos, nonces = _items(ssl, 201, LENGTHS)
    buf, off = _layout(sealed, align=[(5 * i + 3) % 16 for i in range(len(sealed))])
    ok = _verdicts(ctx, ssl, buf, off, [len(s) for s in sealed], infos, nonces)
    assert ok.tolist() == [1] * len(LENGTHS)
    # one flipped bit per item, in its last byte: every one fails, whatever its length
    bad = buf.copy()
    for o, s in zip(off, sealed):
        bad[int(o) + len(s) - 1] ^= 0x20
    assert _verdicts(ctx, ssl, bad, off, [len(s) for s in sealed], infos, nonces).tolist() == [0] * len(LENGTHS)


def test_every_source_alignment(ctx):
    ssl = _ssl()
    lens = [n for a in range(16) for n in (17 + a, 1025, PIECE + 16 + a)]
    sealed, infos, nonces = _items(ssl, 202, lens)
    align = [a for a in range(16) for _ in range(3)]
    buf, off = _layout(sealed, align=align)
    assert sorted(set(int(o) & 15 for o in off)) == list(range(16))
    assert _verdicts(ctx, ssl, buf, off, [len(s) for s in sealed], infos, nonces).all()
    # a ciphertext bit flipped in every second item
    for i in range(0, len(sealed), 2):
        buf[int(off[i]) + len(sealed[i]) // 2] ^= 1
    ok = _verdicts(ctx, ssl, buf, off, [len(s) for s in sealed], infos, nonces)
    assert ok.tolist() == [i % 2 for i in range(len(sealed))]


def test_more_pieces_than_one_grid_pass(ctx):
    ssl = _ssl()
    lens = np.random.default_rng(203).integers(16, 49, 16500)
    assert len(lens) > PASS_PIECES  # one piece each: the waves of the first pass go on to a second piece
    sealed, infos, nonces = _items(ssl, 203, lens)
    buf, off = _layout(sealed, gap=3)
    want = np.ones(len(lens), dtype=np.uint8)
    for i in (0, 255, 256, 8191, 16383, 16384, 16499):  # both sides of the pass border and of a 256-lane block
        buf[int(off[i]) + 5] ^= 2
        want[i] = 0
    assert np.array_equal(_verdicts(ctx, ssl, buf, off, [len(s) for s in sealed], infos, nonces), want)


@pytest.mark.parametrize("lens", [[0], [0, 0, 0], [0, 40, 70000], [40, 70000, 0], [33, 0, 0, 200, 0, PIECE + 5, 0]])
def test_empty_items_anywhere(ctx, lens):
    ssl = _ssl()
    sealed, infos, nonces = _items(ssl, 204, lens)
    buf, off = _layout(sealed)
    assert _verdicts(ctx, ssl, buf, off, [len(s) for s in sealed], infos, nonces).all()
    for i, n in enumerate(lens):  # an empty item is its tag alone: a flipped tag bit fails it and nothing else
        if n == 0:
            bad = buf.copy()
            bad[int(off[i]) + 7] ^= 1
            ok = _verdicts(ctx, ssl, bad, off, [len(s) for s in sealed], infos, nonces)
            assert ok.tolist() == [int(k != i) for k in range(len(lens))]


def test_tamper_matrix(ctx):
    ssl = _ssl()
    two = PIECE + 100                      # two pieces: the first holds 7 blocks
    boundary = 16 * ((two + 15) // 16 - PIECE_BLOCKS)
    lens = [100] * 16 + [two, two, two] + [300, 300, 300, 300] + [90, 90] + [64]
    sealed, infos, nonces = _items(ssl, 205, lens)
    buf, off = _layout(sealed)
    slen = np.array([len(s) for s in sealed], dtype=np.uint64)
    infos, nonces = infos.copy(), nonces.copy()
    want = [0] * len(lens)
    for b in range(16):                                           # 0..15: every tag byte
        buf[int(off[b]) + 100 + b] ^= 1 << (b % 8)
    buf[int(off[16])] ^= 1                                        # 16: the first ciphertext byte
    buf[int(off[17]) + two - 1] ^= 0x80                           # 17: the last
    buf[int(off[18]) + boundary] ^= 8                             # 18: the first byte behind the piece boundary
    nonces[19, 11] ^= 1                                           # 19: nonce
    infos[20, 0] ^= 1                                             # 20: info
    slen[21] -= 1                                                 # 21: truncated by one byte
    slen[22] += 1                                                 # 22: extended by one byte (a canary)
    t23 = buf[int(off[23]) + 90:int(off[23]) + 106].copy()        # 23, 24: tags swapped
    buf[int(off[23]) + 90:int(off[23]) + 106] = buf[int(off[24]) + 90:int(off[24]) + 106]
    buf[int(off[24]) + 90:int(off[24]) + 106] = t23
    want[25] = 1                                                  # 25: untouched
    ok = _verdicts(ctx, ssl, buf, off, slen, infos, nonces)       # asserts OpenSSL's verdict per item
    assert ok.tolist() == want
    # another PRK: nothing verifies; the right one over the untouched items: everything does
    clean, ci, cn = _items(ssl, 206, [0, 50, two])
    cbuf, coff = _layout(clean)
    clen = [len(s) for s in clean]
    assert _verdicts(ctx, ssl, cbuf, coff, clen, ci, cn).tolist() == [1, 1, 1]
    assert _verdicts(ctx, ssl, cbuf, coff, clen, ci, cn, prk=bytes.fromhex("5d" + "5c" * 31)).tolist() == [0, 0, 0]


def test_a_length_below_the_tag_is_refused(ctx):
    from backuwup_amd import _lib, check
    buf = np.zeros(64, dtype=np.uint8)
    with pytest.raises(_lib.BwError) as x:
        check.auth(ctx, PRK, buf, [0, 20], [16, 15], np.zeros((2, 32), np.uint8), np.zeros((2, 12), np.uint8))
    assert x.value.rc == _lib.BW_EINVAL
    assert check.auth(ctx, PRK, buf, [], [], [], []).size == 0
