"""Rekey without a GPU: tests/rekey_ref.py, the yardstick of tests/test_gpu_reseal.py and
tests/test_gpu_rekey.py, pinned to cases checked by hand, and the library's new exports."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

A, B = bytes.fromhex("5c" * 32), bytes.fromhex("a7" * 32)


@pytest.fixture(scope="module")
def ref():
    try:
        import openssl_ref
        openssl_ref.lib()
    except OSError:
        pytest.skip("OpenSSL libcrypto not available")
    import rekey_ref
    return rekey_ref, openssl_ref


def test_same_prk_and_nonce_is_the_identity(ref):
    rk, ssl = ref
    for n in (0, 1, 16, 17, 1000):
        info, nonce = bytes(range(32)), bytes(range(12))
        sealed = ssl.gcm_seal(rk.key(A, info), nonce, bytes(k % 251 for k in range(n)))
        assert rk.reseal_item(A, A, info, nonce, sealed) == (sealed, 1)
        assert rk.reseal_item(A, A, info, nonce, sealed, new_nonce=nonce) == (sealed, 1)


def test_a_resealed_item_opens_under_the_new_prk_only(ref):
    rk, ssl = ref
    info, nonce, nn, pt = b"header", b"\x01" * 12, b"\x02" * 12, b"some header bytes"
    sealed = ssl.gcm_seal(rk.key(A, info), nonce, pt)
    out, ok = rk.reseal_item(A, B, info, nonce, sealed, new_nonce=nn)
    assert ok == 1 and len(out) == len(sealed)
    assert ssl.gcm_open(rk.key(B, info), nn, out) == pt
    assert ssl.gcm_open(rk.key(A, info), nonce, out) is None and ssl.gcm_open(rk.key(B, info), nonce, out) is None
    assert out == ssl.gcm_seal(rk.key(B, info), nn, pt)


def test_a_tampered_item_gets_the_complement_of_the_valid_tag(ref):
    rk, ssl = ref
    info, nonce, pt = bytes(32), bytes(12), bytes(range(40))
    sealed = bytearray(ssl.gcm_seal(rk.key(A, info), nonce, pt))
    sealed[3] ^= 0x10  # one ciphertext bit: the same bit of the plaintext, and of the new ciphertext
    out, ok = rk.reseal_item(A, B, info, nonce, bytes(sealed))
    good = bytearray(ssl.gcm_seal(rk.key(B, info), nonce, pt))
    good[3] ^= 0x10
    assert ok == 0 and out[:40] == bytes(good[:40])
    assert ssl.gcm_open(rk.key(B, info), nonce, out) is None
    fixed = out[:40] + bytes(b ^ 0xff for b in out[40:])
    damaged = bytearray(pt)
    damaged[3] ^= 0x10
    assert ssl.gcm_open(rk.key(B, info), nonce, fixed) == bytes(damaged)  # the complement is of the tag that would verify


def test_gcm_spec_vector_resealed(ref):
    """The GCM specification's test case 14 (key 0^32, IV 0^12, P = 0^16) resealed under test case 15's
    key and IV: the plaintext is zero, so the new ciphertext is the keystream, P15 ^ C15 of the spec."""
    rk, ssl = ref
    k14, iv14 = bytes(32), bytes(12)
    c14 = bytes.fromhex("cea7403d4d606b6e074ec5d3baf39d18" "d0d1c8a799996bf0265b98b5d48ab919")
    k15 = bytes.fromhex("feffe9928665731c6d6a8f9467308308" * 2)
    iv15 = bytes.fromhex("cafebabefacedbaddecaf888")
    p15, c15 = bytes.fromhex("d9313225f88406e5a55909c5aff5269a"), bytes.fromhex("522dc1f099567d07f47f37a32a84427d")
    out, ok = rk.reseal_keys(k14, k15, iv14, c14, new_nonce=iv15)
    assert ok == 1 and out[:16] == bytes(a ^ b for a, b in zip(p15, c15))
    assert ssl.gcm_open(k15, iv15, out) == bytes(16)
    # and back: test case 14's ciphertext and tag, bit for bit
    assert rk.reseal_keys(k15, k14, iv15, out, new_nonce=iv14) == (c14, 1)


def test_store_form_follows_the_packfile_layout(ref, oracle):
    rk, ssl = ref
    import numpy as np
    import prune_ref
    import restore_store
    rng = np.random.default_rng(7)
    b = restore_store.Builder(seed=7)
    for k in range(5):
        b.add(rng.integers(0, 256, 30 + 11 * k, dtype=np.uint8).tobytes())
    packs, _ = b.finish(target=3)
    prk = restore_store.PRK
    hd = prune_ref.headers_of(prk, packs)
    ents = [h[3] for h in hd]
    same, est, pst = rk.rekey_store(prk, prk, packs, ents)
    assert same == [bytes(p[1]) for p in packs] and est == [0] * 5 and pst == [0] * len(packs)
    new, est, pst = rk.rekey_store(prk, B, packs, ents)
    assert est == [0] * 5 and pst == [0] * len(packs)
    new_packs = [(pid, nb) for (pid, _), nb in zip(packs, new)]
    assert [h[3] for h in prune_ref.headers_of(B, new_packs)] == ents
    for (pid, old), nb, (_, _, hl, es) in zip(packs, new, hd):
        assert len(nb) == len(old) and nb[:8] == old[:8]
        for h, _, _, length, offset in es:
            at = 8 + hl + offset
            assert nb[at:at + 12] == old[at:at + 12]
            assert ssl.gcm_open(rk.key(B, h), nb[at:at + 12], nb[at + 12:at + 12 + length]) == \
                ssl.gcm_open(rk.key(prk, h), old[at:at + 12], old[at + 12:at + 12 + length]) != None  # noqa: E711
    # a damaged blob and an entry that leaves the section
    buf = bytearray(packs[0][1])
    h0 = hd[0]
    buf[8 + h0[2] + h0[3][1][4] + 12] ^= 1
    cut = [(packs[0][0], bytes(buf)), (packs[1][0], packs[1][1][:-1])]
    _, est, pst = rk.rekey_store(prk, B, cut, ents)
    assert est == [0, rk.ETAG, 0, 0, rk.ERANGE] and pst == [0, 0]


def test_the_library_exports_reseal_and_rekey():
    from backuwup_amd import _lib
    lib = _lib.load()
    for name in ("bw_reseal_device", "bw_reseal", "bw_rekey_store_device", "bw_rekey_store"):
        assert hasattr(lib, name)
    from backuwup_amd import rekey
    for name in ("reseal", "reseal_device", "rekey_store", "rekey"):
        assert callable(getattr(rekey, name))
