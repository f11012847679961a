"""The read side over whole packfiles: bw_unpack_headers, bw_unpack_blobs(_device)
and Manager.get_blob against packfiles the oracle wrote (payloads compressed by the system libzstd at
mixed levels) and packfiles the device chain wrote (bw_pack_compress_device + bw_pack_build_compressed),
then damaged packfiles: every failure lands where the reference returns its error, and only there."""
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_corpus  # noqa: E402
import zstd_ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]
PRK = bytes.fromhex("5c" * 32)
LEVELS = (1, 3, 7, 13, 19)


@pytest.fixture(scope="module")
def po(oracle):
    from oracle import pack_oracle
    return pack_oracle


@pytest.fixture(scope="module")
def corpus(oracle):
    """41 blobs of 0 - 400 KB, both kinds, hashed by the oracle's BLAKE3: (blobs, hashes, kinds, nonces)."""
    rng = np.random.default_rng(77)
    kinds_c = ["random", "text", "random", "repeats", "random", "runs", "random", "mixed"]
    sizes = [0, 1, 400000, 5, 3000] + [int(x) for x in rng.integers(150000, 400000, 36)]
    blobs = [zstd_corpus.blob(kinds_c[i % 8], n, 100 + i) if n else b"" for i, n in enumerate(sizes)]
    hashes = [oracle.blake3(b) for b in blobs]
    kinds = [int(x) for x in rng.integers(0, 2, len(blobs))]
    nonces = [bytes(x) for x in rng.integers(0, 256, (len(blobs), 12), dtype=np.uint8)]
    return blobs, hashes, kinds, nonces


@pytest.fixture(scope="module")
def oracle_packs(po, corpus):
    """[(id, bytes)] from oracle/pack_oracle.py, and the queue position of every blob's packfile."""
    blobs, hashes, kinds, nonces = corpus
    rng = np.random.default_rng(78)
    sealed = [(hashes[i], kinds[i], nonces[i],
               po.seal_blob_payload(PRK, hashes[i], nonces[i], zstd_ref.compress(b, LEVELS[i % 5])))
              for i, b in enumerate(blobs)]
    ids = [bytes(x) for x in rng.integers(0, 256, (16, 12), dtype=np.uint8)]
    packs = po.write_packfiles(PRK, sealed, ids)
    assert len(packs) >= 3
    return packs


def _check_all(ctx, po, packs, corpus):
    blobs, hashes, kinds, _ = corpus
    files, ids = [b for _, b in packs], [i for i, _ in packs]
    entries = ctx.unpack_headers(PRK, files, ids)
    want = []
    for p, (pid, buf) in enumerate(packs):
        hl = struct.unpack_from("<Q", buf, 0)[0]
        pt = po.oracle.open_blob(PRK, b"header", pid, bytes(buf[8:8 + hl]))
        want += [(h, k, c, ln, off, p) for h, k, c, ln, off in po.deserialize_header(pt)]
    assert len(entries) == len(want) == len(blobs)
    for e, (h, k, c, ln, off, p) in zip(entries, want):
        assert (e["hash"].tobytes(), int(e["kind"]), int(e["compression"]), int(e["length"]), int(e["offset"]),
                int(e["packfile"])) == (h, k, c, ln, off, p)
    assert [e["hash"].tobytes() for e in entries] == hashes and [int(e["kind"]) for e in entries] == kinds
    for verify in (False, True):
        got, st = ctx.unpack_blobs(PRK, files, entries, verify=verify)
        assert not st.any(), st
        assert got == blobs
    return entries


def test_unpack_oracle_packfiles(ctx, po, oracle_packs, corpus):
    _check_all(ctx, po, oracle_packs, corpus)


def test_unpack_device_chain_packfiles(ctx, po, corpus):
    """Write then read, wholly on the device: bw_pack_compress_device + bw_pack_build_compressed, then
    bw_unpack_blobs_device over the packfiles where they were built."""
    import torch
    blobs, hashes, kinds, nonces = corpus
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    so = np.concatenate([[0], np.cumsum(lens[:-1] + np.uint64(3))]).astype(np.uint64)
    host = np.zeros(int(so[-1] + lens[-1]) + 16, dtype=np.uint8)
    for o, b in zip(so, blobs):
        host[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    d_src = torch.from_numpy(host).cuda()
    fl = ctx.pack_compress_device(d_src.data_ptr(), so, lens)
    plan, total = ctx.pack_plan(fl, flags=0)
    assert len(plan) >= 3
    ids = np.random.default_rng(79).integers(0, 256, (len(plan), 12), dtype=np.uint8)
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    h = np.frombuffer(b"".join(hashes), dtype=np.uint8).reshape(-1, 32)
    no = np.frombuffer(b"".join(nonces), dtype=np.uint8).reshape(-1, 12)
    ctx.pack_build_compressed(PRK, h, kinds, no, plan, ids, d_out.data_ptr())
    torch.cuda.synchronize()
    buf = d_out.cpu().numpy().tobytes()
    packs = [(bytes(ids[k]), buf[int(p["offset"]):int(p["offset"] + p["size"])]) for k, p in enumerate(plan)]
    entries = _check_all(ctx, po, packs, corpus)
    # the device form, over the packfiles in place
    do = np.arange(len(blobs), dtype=np.uint64) * np.uint64(3 << 20)  # 3 MiB of room each
    d_dst = torch.zeros(len(blobs) * (3 << 20), dtype=torch.uint8, device="cuda")
    for verify in (False, True):
        ol, st = ctx.unpack_blobs_device(PRK, d_out.data_ptr(), plan, entries, d_dst.data_ptr(), do, verify=verify)
        assert not st.any() and np.array_equal(ol, lens)
    back = d_dst.cpu().numpy()
    for o, b in zip(do, blobs):
        assert back[int(o):int(o) + len(b)].tobytes() == b


def test_manager_get_blob(ctx, oracle_packs, corpus):
    from backuwup_amd.packer import BlobIndex, IndexHeaderMismatch, Manager
    blobs, hashes, kinds, _ = corpus
    files = [b for _, b in oracle_packs]
    entries = ctx.unpack_headers(PRK, files, [i for i, _ in oracle_packs])
    where = {e["hash"].tobytes(): oracle_packs[int(e["packfile"])][0] for e in entries}
    second = [e["hash"].tobytes() for e in entries if e["packfile"] == 1]
    middle = second[len(second) // 2]
    stray = bytes(range(32))                      # in the index, in no header
    where[stray] = oracle_packs[0][0]
    m = Manager(index=BlobIndex(ctx=ctx), blob_packfiles=where, packfiles=dict(oracle_packs), prk=PRK)
    k = hashes.index(middle)
    assert m.get_blob(middle) == (kinds[k], blobs[k])
    assert m.get_blob(b"\xff" * 32) is None
    with pytest.raises(IndexHeaderMismatch):
        m.get_blob(stray)
    got = m.get_blobs([hashes[5], b"\xfe" * 32, hashes[30], hashes[0]], verify=True)
    assert got == [(kinds[5], blobs[5]), None, (kinds[30], blobs[30]), (kinds[0], blobs[0])]


def test_unpack_damage(ctx, po, oracle, oracle_packs, corpus):
    from backuwup_amd import _lib
    from backuwup_amd._lib import BW_ECRYPTO, BW_EFORMAT, BwError
    blobs, hashes, kinds, nonces = corpus
    files, ids = [bytearray(b) for _, b in oracle_packs], [i for i, _ in oracle_packs]
    entries = ctx.unpack_headers(PRK, files, ids)
    base = [8 + struct.unpack_from("<Q", f, 0)[0] for f in files]
    others = lambda st, i: not np.delete(st, i).any()  # noqa: E731

    # one flipped byte in one sealed blob: that blob _ETAG, every other OK
    e = entries[7]
    bad = [bytearray(f) for f in files]
    bad[int(e["packfile"])][base[int(e["packfile"])] + int(e["offset"]) + 12 + int(e["length"]) // 2] ^= 0x10
    got, st = ctx.unpack_blobs(PRK, bad, entries, verify=True)
    assert st[7] == _lib.BW_UNPACK_ETAG and others(st, 7) and got[7] is None
    assert [g for i, g in enumerate(got) if i != 7] == [b for i, b in enumerate(blobs) if i != 7]

    def headers_fail(fs, rc, bad_file, prk=PRK):
        with pytest.raises(BwError) as x:
            ctx.unpack_headers(prk, fs, ids)
        assert x.value.rc == rc and x.value.bad_file == bad_file, (x.value.rc, x.value.bad_file)

    bad = [bytearray(f) for f in files]
    bad[1][8 + 5] ^= 1                                         # one flipped byte in a header
    headers_fail(bad, BW_ECRYPTO, 1)
    headers_fail(files, BW_ECRYPTO, 0, prk=bytes(32))          # a wrong prk
    bad = [bytearray(f) for f in files]
    bad[2][:8] = struct.pack("<Q", 0)                          # header_len 0
    headers_fail(bad, BW_EFORMAT, 2)
    bad[2][:8] = struct.pack("<Q", len(bad[2]) + 1)            # header_len above the size
    headers_fail(bad, BW_EFORMAT, 2)
    headers_fail([files[0], bytes((16 << 20) + 1)], BW_EFORMAT, 1)  # PackfileTooLarge (ids[:2] are used)
    # a header that is not one varint Vec / carries an enum tag above 1
    for pt in (po.serialize_header([(hashes[0], 2, 1, 20, 0)]), po.serialize_header([(hashes[0], 0, 1, 20, 0)]) + b"\0",
               b"\x02" + po.header_entry(hashes[0], 0, 1, 20, 0)):
        hdr = oracle.seal_blob(PRK, b"header", ids[0], pt)
        headers_fail([struct.pack("<Q", len(hdr)) + hdr + bytes(64)], BW_EFORMAT, 0)

    # an entry whose offset + 12 + length runs past its packfile: _ERANGE, the others OK
    en = entries.copy()
    p = int(en[3]["packfile"])
    en[3]["length"] = len(files[p]) - base[p] - int(en[3]["offset"]) - 12 + 1
    got, st = ctx.unpack_blobs(PRK, files, en)
    assert st[3] == _lib.BW_UNPACK_ERANGE and others(st, 3)
    en[3]["length"] -= 1                                       # to the last byte: in range, so the tag fails
    assert ctx.unpack_blobs(PRK, files, en)[1][3] == _lib.BW_UNPACK_ETAG

    # one blob's frame re-sealed under another blob's hash, the header fixed to match: _EDIGEST with
    # the verify flag, OK (and the other blob's bytes) without it
    sealed = [(hashes[i], kinds[i], nonces[i],
               po.seal_blob_payload(PRK, hashes[i], nonces[i], zstd_ref.compress(blobs[9 if i == 4 else i], 3)))
              for i in range(12)]
    packs = po.write_packfiles(PRK, sealed, ids)
    fs, pid = [b for _, b in packs], [i for i, _ in packs]
    en = ctx.unpack_headers(PRK, fs, pid)
    got, st = ctx.unpack_blobs(PRK, fs, en, verify=True)
    assert st[4] == _lib.BW_UNPACK_EDIGEST and others(st, 4)
    got, st = ctx.unpack_blobs(PRK, fs, en)
    assert not st.any() and got[4] == blobs[9]
    # a frame that is not zstd, sealed properly: _EZSTD
    sealed[2] = (hashes[2], kinds[2], nonces[2], po.seal_blob_payload(PRK, hashes[2], nonces[2], b"\x00\x00\x07\x00\x00"))
    packs = po.write_packfiles(PRK, sealed, ids)
    fs = [b for _, b in packs]
    en = ctx.unpack_headers(PRK, fs, pid)
    st = ctx.unpack_blobs(PRK, fs, en)[1]
    assert st[2] == _lib.BW_UNPACK_EZSTD and others(st, 2)
