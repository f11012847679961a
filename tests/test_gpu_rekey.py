"""bw_rekey_store(_device) and backuwup_amd.rekey.rekey over small stores built the way tests/check_stores.py
builds them: the rekeyed store equals, byte for byte, the same blobs packed under the new PRK with the same
nonces and ids, and tests/rekey_ref.py's store form; check and restore accept it under the new PRK and
nothing opens under the old one; damage stays damage."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]

A, B = bytes.fromhex("a7" * 32), bytes.fromhex("19" * 32)


@pytest.fixture(scope="module")
def ck(oracle):
    try:
        import openssl_ref
        openssl_ref.lib()
    except OSError:
        pytest.skip("OpenSSL libcrypto not available")
    import check_stores
    import prune_ref
    import rekey_ref
    import restore_store
    from oracle import pack_oracle
    from backuwup_amd import _lib, check, rekey, restore

    class NS:
        pass
    ns = NS()
    ns.st, ns.pref, ns.ref, ns.store, ns.po, ns.oracle = check_stores, prune_ref, rekey_ref, restore_store, pack_oracle, oracle
    ns.lib, ns.check, ns.rekey, ns.restore = _lib, check, rekey, restore
    return ns


def build(ck, prk):
    """A few packfiles of 6: tree and file blobs in store frames, three blobs in compressed frames, and a
    packfile without entries.  The same seed gives the same nonces and ids under either PRK."""
    rng = np.random.default_rng(61)
    bb = ck.st.blob_bytes
    spec = {"docs": {"a.txt": bb(rng, 3000), "b.txt": bb(rng, 700), "empty": b""}, "src": {"m.c": bb(rng, 5000), "deep": {"x": bb(rng, 100)}}}
    b = ck.store.Builder(prk=prk, seed=61)
    root = b.add_dir("", spec)
    for k in range(3):
        data = (b"compressible line %d\n" % k) * (40 + 300 * k)
        frame = ck.oracle.zstd3_compress(data)
        assert frame != ck.po.zstd_store(data)
        b.add(data, payload=frame)
    packs, index = b.finish(target=6)
    empty_id = b"\x77" * 12
    packs.append((empty_id, ck.po.serialize_packfile(prk, empty_id, [])))
    return packs, index, root, ck.store.flatten(spec)


@pytest.fixture(scope="module")
def stores(ck):
    a, b = build(ck, A), build(ck, B)
    assert [i for i, _ in a[0]] == [i for i, _ in b[0]] and a[1] == b[1] and a[2] == b[2]
    assert [len(x) for _, x in a[0]] == [len(x) for _, x in b[0]] and all(x != y for (_, x), (_, y) in zip(a[0], b[0]))
    return a, b


def session(ctx, ck, packs, index, prk=A, entries=None):
    hd = ck.pref.headers_of(prk, packs)
    en = ck.pref.entries_array(hd) if entries is None else entries
    return ck.restore.Session(ctx, prk, [b for _, b in packs], [i for i, _ in packs], en, ck.store.items_array(index)), hd


def split(out, packs):
    res, at = [], 0
    for _, b in packs:
        res.append(out[at:at + len(b)].tobytes())
        at += len(b)
    return res


def test_rekeyed_store_is_the_store_packed_under_the_new_prk(ctx, ck, stores):
    import torch
    (pa, index, _, _), (pb, _, _, _) = stores
    pa, pb = list(pa), list(pb)
    pa[1] = (pa[1][0], pa[1][1] + b"\x01\x02\x03\x04\x05")   # trailing bytes in one blob section: copied as they are
    pb[1] = (pb[1][0], pb[1][1] + b"\x01\x02\x03\x04\x05")
    s, hd = session(ctx, ck, pa, index)
    total = sum(len(b) for _, b in pa)
    out = np.full(total, 0xC3, dtype=np.uint8)
    est, pst = ck.rekey.rekey_store(s, B, out=out)
    assert not est.any() and not pst.any() and est.size == sum(len(h[3]) for h in hd) and pst.size == len(pa)
    assert split(out, pa) == [b for _, b in pb]
    want, west, wpst = ck.ref.rekey_store(A, B, pa, [h[3] for h in hd])
    assert split(out, pa) == want and est.tolist() == west and pst.tolist() == wpst
    # the device form, canaries behind the table's extent
    d = torch.full((total + 64,), 0xC3, dtype=torch.uint8, device="cuda")
    est, pst = ck.rekey.rekey_store(s, B, d_out=d.data_ptr())
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    assert not est.any() and not pst.any() and np.array_equal(got[:total], out) and (got[total:] == 0xC3).all()
    s.close()


def test_rekeyed_store_checks_and_restores_under_the_new_prk_only(ctx, ck, stores):
    (pa, index, root, files), _ = stores
    s, hd = session(ctx, ck, pa, index)
    out = np.zeros(sum(len(b) for _, b in pa), dtype=np.uint8)
    ck.rekey.rekey_store(s, B, out=out)
    s.close()
    new, ids, items = split(out, pa), [i for i, _ in pa], ck.store.items_array(index)
    en = ck.pref.entries_array(hd)
    rep = ck.check.check(ctx, new, ids, en, items, B, roots=[root], read_data="full")
    assert rep["ok"] and rep["bad_packfiles"] == [] and not rep["data_status"].any()
    got, errors = ck.restore.unpack(ctx, new, ids, en, items, B, root)
    was, _ = ck.restore.unpack(ctx, [b for _, b in pa], ids, en, items, A, root)
    assert not errors and got == was == files
    # under the old PRK: no header opens, no blob authenticates
    with pytest.raises(ck.lib.BwError):
        ctx.unpack_headers(A, new, ids)
    with ck.restore.Session(ctx, A, new, ids, en, items) as sa:
        assert (ck.check.data(sa, "auth") == ck.lib.BW_UNPACK_ETAG).all()
    again = ctx.unpack_headers(B, new, ids)
    assert again.size == en.size and all(np.array_equal(again[f], en[f]) for f in ("hash", "packfile", "kind", "length", "offset"))


def test_damage_stays_damage(ctx, ck, stores):
    (pa, index, _, _), (pb, _, _, _) = stores
    pa = list(pa)
    hd = ck.pref.headers_of(A, pa)
    victim = hd[0][3][2][0]                                   # entry 2 of packfile 0
    ck.st._flip(pa, hd, victim, 7)
    buf = bytearray(pa[2][1])
    buf[8 + 4] ^= 0x40                                        # a byte of packfile 2's sealed header
    pa[2] = (pa[2][0], bytes(buf))
    en = ck.pref.entries_array(hd)
    s = ck.restore.Session(ctx, A, [b for _, b in pa], [i for i, _ in pa], en, ck.store.items_array(index))
    out = np.zeros(sum(len(b) for _, b in pa), dtype=np.uint8)
    est, pst = ck.rekey.rekey_store(s, B, out=out)
    s.close()
    assert est.tolist() == [ck.lib.BW_UNPACK_ETAG if e == 2 else 0 for e in range(en.size)]
    assert pst.tolist() == [ck.lib.BW_UNPACK_ETAG if p == 2 else 0 for p in range(len(pa))]
    new = split(out, pa)
    want, west, wpst = ck.ref.rekey_store(A, B, pa, [h[3] for h in hd])
    assert new == want and est.tolist() == west and pst.tolist() == wpst
    # the damaged outputs fail bw_auth under B, and everything else is the store packed under B
    e2 = hd[0][3][2]
    b_at = 8 + hd[0][2] + e2[4]
    h_len = hd[2][2]
    ok = ck.check.auth(ctx, B, np.frombuffer(new[0], dtype=np.uint8), [b_at + 12], [e2[3]], [np.frombuffer(victim, dtype=np.uint8)],
                       [np.frombuffer(new[0][b_at:b_at + 12], dtype=np.uint8)])
    assert ok.tolist() == [0]
    info = np.zeros((1, 6), dtype=np.uint8)
    info[0] = np.frombuffer(b"header", dtype=np.uint8)
    ok = ck.check.auth(ctx, B, np.frombuffer(new[2], dtype=np.uint8), [8], [h_len], info, [np.frombuffer(pa[2][0], dtype=np.uint8)])
    assert ok.tolist() == [0]
    for p, (got, (_, good)) in enumerate(zip(new, pb)):
        got, good = bytearray(got), bytearray(good)
        if p == 0:
            got[b_at + 12:b_at + 12 + e2[3]] = good[b_at + 12:b_at + 12 + e2[3]]
        if p == 2:
            got[8:8 + h_len] = good[8:8 + h_len]
        assert got == good, p


def test_overlapping_entries_are_refused_before_anything_is_written(ctx, ck, stores):
    import torch
    (pa, index, _, _), _ = stores
    hd = ck.pref.headers_of(A, pa)
    en = ck.pref.entries_array(hd)
    en[1]["offset"] = en[0]["offset"] + 12 + en[0]["length"] - 1   # entry 1 starts on entry 0's last byte, still in range
    s, _ = session(ctx, ck, pa, index, entries=en)
    total = sum(len(b) for _, b in pa)
    d = torch.full((total,), 0xC3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ck.lib.BwError) as x:
        ck.rekey.rekey_store(s, B, d_out=d.data_ptr())
    assert x.value.rc == ck.lib.BW_EINVAL
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 0xC3).all()
    s.close()


def test_entries_out_of_range_and_an_empty_session(ctx, ck, stores):
    (pa, index, _, _), (pb, _, _, _) = stores
    pa, pb = list(pa), list(pb)
    pa[1], pb[1] = (pa[1][0], pa[1][1][:-1]), (pb[1][0], pb[1][1][:-1])   # the last blob of packfile 1 loses a byte
    hd = ck.pref.headers_of(A, pa)
    s, _ = session(ctx, ck, pa, index)
    out = np.zeros(sum(len(b) for _, b in pa), dtype=np.uint8)
    est, pst = ck.rekey.rekey_store(s, B, out=out)
    s.close()
    last = len(hd[0][3]) + len(hd[1][3]) - 1
    assert est.tolist() == [ck.lib.BW_UNPACK_ERANGE if e == last else 0 for e in range(est.size)] and not pst.any()
    new = split(out, pa)
    assert new == ck.ref.rekey_store(A, B, pa, [h[3] for h in hd])[0]
    e = hd[1][3][-1]
    cut = 8 + hd[1][2] + e[4]
    assert new[1][cut:] == pa[1][1][cut:] and new[1][:cut] == pb[1][1][:cut]   # never read: copied as it is
    with ck.restore.Session(ctx, A, [], [], ck.pref.entries_array([]), ck.store.items_array([])) as s0:
        est, pst = ck.rekey.rekey_store(s0, B, out=np.zeros(1, dtype=np.uint8))
        assert est.size == 0 and pst.size == 0


def test_rekey_round_trips_packfiles_and_index_files(ctx, ck, stores):
    (pa, index, root, files), (pb, _, _, _) = stores
    ids, items = [i for i, _ in pa], ck.store.items_array(index)
    en = ck.pref.entries_array(ck.pref.headers_of(A, pa))
    index_files = ctx.index_files_build(A, items, last_file_num=4)
    new, new_index, bad_e, bad_p = ck.rekey.rekey(ctx, [b for _, b in pa], ids, en, items, index_files, A, B)
    assert new == [b for _, b in pb] and bad_e == [] and bad_p == []
    assert [n for n, _ in new_index] == [n for n, _ in index_files]
    assert np.array_equal(ctx.index_load_files(B, new_index), items)
    got, errors = ck.restore.unpack(ctx, new, ids, en, ctx.index_load_files(B, new_index), B, root)
    assert not errors and got == files
