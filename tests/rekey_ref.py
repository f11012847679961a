"""What reseal and rekey must produce, restated plainly over the system OpenSSL (tests/openssl_ref.py) and
Python's hmac: open under the old PRK, seal under the new one, and complement the tag of an item that
did not open.  A helper, not a test; the yardstick of tests/test_gpu_reseal.py and test_gpu_rekey.py.

The store form goes over oracle/pack_oracle.py's layout: u64 header_len || sealed header || per entry
nonce || sealed blob."""
import ctypes
import hashlib
import hmac
import struct

import openssl_ref

OK, ETAG, ERANGE = 0, 1, 4  # BW_UNPACK_OK, BW_UNPACK_ETAG, BW_UNPACK_ERANGE


def key(prk, info):
    """HKDF-Expand (RFC 5869) to 32 bytes: one HMAC block."""
    return hmac.new(bytes(prk), bytes(info) + b"\x01", hashlib.sha256).digest()


def ctr_plain(k, nonce, body):
    """The CTR half of AES-GCM decryption alone: what the ciphertext body decrypts to, verified or not."""
    L = openssl_ref.lib()
    body = bytes(body)
    if not body:
        return b""
    c = L.EVP_CIPHER_CTX_new()
    try:
        assert L.EVP_DecryptInit_ex(c, L.EVP_aes_256_gcm(), None, bytes(k), bytes(nonce)) == 1
        out = ctypes.create_string_buffer(len(body) + 32)
        n = ctypes.c_int(0)
        assert L.EVP_DecryptUpdate(c, out, ctypes.byref(n), body, len(body)) == 1
        return out.raw[:n.value]
    finally:
        L.EVP_CIPHER_CTX_free(c)


def reseal_keys(old_key, new_key, nonce, sealed, new_nonce=None):
    """One item between two AES-256 keys -> (output bytes of len(sealed), ok).  sealed = ciphertext ||
    tag, at least 16 bytes."""
    sealed = bytes(sealed)
    assert len(sealed) >= 16
    ok = openssl_ref.gcm_open(old_key, nonce, sealed) is not None
    pt = ctr_plain(old_key, nonce, sealed[:-16])
    out = openssl_ref.gcm_seal(new_key, nonce if new_nonce is None else new_nonce, pt)
    if not ok:
        out = out[:-16] + bytes(b ^ 0xff for b in out[-16:])
    return out, int(ok)


def reseal_item(old_prk, new_prk, info, nonce, sealed, new_nonce=None):
    """reseal_keys under the two PRKs' keys for this info."""
    return reseal_keys(key(old_prk, info), key(new_prk, info), nonce, sealed, new_nonce)


def range_ok(size, header_len, offset, length):
    """BW_UNPACK_ERANGE's rule: nonce + sealed bytes inside the blob section, and a tag's worth of them."""
    base = 8 + header_len
    return not (base > size or offset + 12 + length > size - base or length < 16)


def rekey_store(old_prk, new_prk, packs, entries):
    """packs: [(id, bytes)]; entries: per packfile [(hash, kind, compression, length, offset)], as its
    header lists them.  -> (new packfile bytes per packfile, entry statuses flat, packfile statuses)."""
    out, est, pst = [], [], []
    for (pid, buf), ents in zip(packs, entries):
        buf = bytes(buf)
        new = bytearray(buf)
        hl = struct.unpack_from("<Q", buf, 0)[0] if len(buf) >= 8 else 0
        if len(buf) >= 8 and hl >= 16 and 8 + hl <= len(buf):
            new[8:8 + hl], ok = reseal_item(old_prk, new_prk, b"header", pid, buf[8:8 + hl])
            pst.append(OK if ok else ETAG)
        else:
            pst.append(ERANGE)
        for h, _, _, length, offset in ents:
            if not range_ok(len(buf), hl, offset, length):
                est.append(ERANGE)
                continue
            at = 8 + hl + offset
            new[at + 12:at + 12 + length], ok = reseal_item(old_prk, new_prk, h, buf[at:at + 12], buf[at + 12:at + 12 + length])
            est.append(OK if ok else ETAG)
        out.append(bytes(new))
    return out, est, pst
