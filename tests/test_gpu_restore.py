"""Restore on the device (bw_restore_*: locate, tree walk, file assembly) against tests/restore_ref.py,
the literal restatement of dir_unpacker.rs, over the same packfiles.  All stores are small; the
shapes are the smallest at which each kernel can go wrong."""
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]
MIB3 = 3 << 20


@pytest.fixture(scope="module")
def rs(oracle):
    import restore_ref
    import restore_store
    from backuwup_amd import _lib, restore

    class NS:
        pass
    ns = NS()
    ns.ref, ns.store, ns.lib, ns.restore, ns.po, ns.oracle = restore_ref, restore_store, _lib, restore, restore_store.po, oracle
    ns.PRK = restore_store.PRK
    return ns


def open_session(ctx, rs, packs, index, slots=0):
    files, ids = [b for _, b in packs], [i for i, _ in packs]
    entries = ctx.unpack_headers(rs.PRK, files, ids)
    return rs.restore.Session(ctx, rs.PRK, files, ids, entries, rs.store.items_array(index), slots=slots), entries


def blob_bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


# ------------------------------------------------------------------ locate
def test_locate_duplicate_in_one_header_gives_the_lower_entry(ctx, rs):
    b = rs.store.Builder(seed=2)
    hs = [b.add(bytes([i]) * 10) for i in range(5)]
    b.add(bytes([2]) * 10, again=True)  # the same hash a second time, same packfile
    b.add(b"tail")
    packs, index = b.finish(target=100)
    s, entries = open_session(ctx, rs, packs, index)
    assert [e["hash"].tobytes() for e in entries].count(hs[2]) == 2
    idx, st = s.locate(hs)
    assert not st.any() and list(idx) == [0, 1, 2, 3, 4]
    s.close()


def test_locate_statuses_over_a_mixed_query(ctx, rs):
    rng = np.random.default_rng(3)
    b = rs.store.Builder(seed=3)
    hashes = [blob_bytes(rng, 32) for _ in range(150)]
    base = blob_bytes(rng, 32)
    hashes += [base[:8] + blob_bytes(rng, 24) for _ in range(20)]       # the first 8 bytes shared
    hashes += [base[:31] + bytes([k]) for k in range(1, 21)]             # the first 31 bytes shared
    for k, h in enumerate(hashes):
        b.add(struct.pack("<I", k), blob_hash=h)                          # headers accept any hash
    packs, index = b.finish(target=23)
    only_header = set(hashes[5:150:9])                                    # in a header, not in the index
    index = [(h, pid) for h, pid in index if h not in only_header]
    only_index = [blob_bytes(rng, 32) for _ in range(15)] + [base[:31] + b"\xff", base[:8] + bytes(24)]
    index += [(h, packs[k % len(packs)][0]) for k, h in enumerate(only_index)]
    absent_id = [blob_bytes(rng, 32) for _ in range(12)]
    index += [(h, blob_bytes(rng, 12)) for h in absent_id]                # a packfile id that is not among ids
    order = rng.permutation(len(index))
    index = [index[i] for i in order]
    s, entries = open_session(ctx, rs, packs, index)
    query = hashes + only_index + absent_id + [blob_bytes(rng, 32) for _ in range(60)]
    query = [query[i] for i in rng.permutation(len(query))]
    assert len(query) > 250
    idx, st = s.locate(query)
    ref = rs.ref.Store(rs.PRK, packs, index)
    first = {}
    for k, e in enumerate(entries):
        first.setdefault(e["hash"].tobytes(), k)
    seen = set()
    for q, i, code in zip(query, idx, st):
        want = ref.get_blob(q)[0]
        assert code == want, (q.hex(), code, want)
        assert int(i) == (first[q] if want == 0 else 2**64 - 1)
        seen.add(int(code))
    assert seen == {0, rs.ref.ENOTFOUND, rs.ref.EMISMATCH, rs.ref.ENOPACKFILE}
    s.close()


# ------------------------------------------------------------------ tree parse
def _tree(rs, kind=0, name=b"n", size=None, mtime=None, ctime=None, children=b"", sib=None):
    return rs.oracle.tree_serialize(kind, name, size, mtime, ctime, children, sib)


def test_tree_parse_against_the_deserializer(ctx, rs):
    T = lambda **kw: _tree(rs, **kw)  # noqa: E731
    long_blob = T(name="nom-é".encode(), size=7, mtime=9, ctime=11, children=bytes(64))
    assert 100 < len(long_blob) < 130
    cases = {
        "empty name": T(name=b""), "multi-byte": T(name="été — 日本 \U0001f600".encode()), "300 bytes": T(name=b"x" * 300),
        "max code point": T(name="\U0010ffff퟿".encode("utf-8", "surrogatepass")),
        "overlong 2": T(name=b"\xc0\xaf"), "overlong 3": T(name=b"\xe0\x9f\xbf"), "overlong 4": T(name=b"\xf0\x8f\xbf\xbf"),
        "surrogate": T(name=b"\xed\xa0\x80"), "above 10ffff": T(name=b"\xf4\x90\x80\x80"), "f5": T(name=b"\xf5\x80\x80\x80"),
        "truncated": T(name=b"ab\xe2\x82"), "stray continuation": T(name=b"a\x80b"), "bad second": T(name=b"\xe2\x28\xa1"),
        "enum tag 2": b"\x02" + T()[1:], "size tag 2": T()[:13] + b"\x02" + T()[14:],
        "ctime tag 2": T()[:15] + b"\x02" + T()[16:], "sibling tag 2": T()[:-1] + b"\x02",
        "children one past": T(children=bytes(64))[:-73] + struct.pack("<Q", 3) + bytes(64) + b"\x00",
        "name 2^63": T()[:4] + struct.pack("<Q", 2**63) + T()[12:], "name 2^64-1": T()[:4] + struct.pack("<Q", 2**64 - 1) + T()[12:],
        "children 2^63": T()[:16] + struct.pack("<Q", 2**63) + b"\x00", "children 2^64-1": T()[:16] + struct.pack("<Q", 2**64 - 1),
        "trailing": long_blob + b"trailing bytes", "sibling cut": T(sib=bytes(32))[:-1],
    }
    for m in range(8):
        cases["meta %d" % m] = T(size=5 if m & 1 else None, mtime=2**64 - 1 if m & 2 else None, ctime=0 if m & 4 else None)
    for k in range(len(long_blob)):
        cases["prefix %d" % k] = long_blob[:k]
    b = rs.store.Builder(seed=4)
    roots = {}
    for i, (label, data) in enumerate(cases.items()):
        roots[label] = b.add_raw_tree(data, blob_hash=struct.pack("<I", i) + bytes(28))
    packs, index = b.finish(target=40)
    s, _ = open_session(ctx, rs, packs, index, slots=3)
    ref = rs.ref.Store(rs.PRK, packs, index)
    good = 0
    for label, h in roots.items():
        try:
            want = rs.ref.fetch_tree(ref, h)
        except rs.ref.RestoreError as e:
            assert e.reason == rs.ref.EFORMAT
            with pytest.raises(rs.restore.TreeError) as x:
                s.trees(h)
            assert x.value.reason == rs.lib.BW_RESTORE_EFORMAT and x.value.hash == h and x.value.rc == rs.lib.BW_EFORMAT, label
            continue
        if want.next_sibling is not None or want.kind != 0:
            continue
        good += 1
        nodes, names, chunks = s.trees(h)
        assert len(nodes) == 1, label
        nd = nodes[0]
        flags = (1 if want.size is not None else 0) | (2 if want.mtime is not None else 0) | (4 if want.ctime is not None else 0)
        assert (int(nd["kind"]), names.decode(), int(nd["flags"]), int(nd["parent"])) == (0, want.name, flags, 2**64 - 1), label
        assert (int(nd["size"]), int(nd["mtime"]), int(nd["ctime"])) == (want.size or 0, want.mtime or 0, want.ctime or 0)
        assert chunks.tobytes() == b"".join(want.children), label
    assert good == 4 + 8 + 1  # the three names, the extreme code points, the 8 option patterns, trailing bytes
    s.close()


# ------------------------------------------------------------------ chains and the walk
def _compare_walk(rs, s, ref, root, max_pieces=None):
    want_nodes, want_files, want_err = rs.ref.unpack(ref, root, max_pieces)
    nodes, names, chunks = s.trees(root)
    assert len(nodes) == len(want_nodes)
    paths = rs.restore.walk_paths(nodes, names)
    for i, (nd, w) in enumerate(zip(nodes, want_nodes)):
        t = w["tree"]
        assert paths[i].replace(os.sep, "/") == w["path"]
        assert int(nd["kind"]) == t.kind and int(nd["n_children"]) == len(t.children)
        assert int(nd["parent"]) == (2**64 - 1 if w["parent"] is None else w["parent"])
        if t.kind == 0:
            lo = int(nd["child_first"])
            assert chunks[lo:lo + len(t.children)].tobytes() == b"".join(t.children)
        else:
            lo = int(nd["child_first"])
            assert [want_nodes[k]["hash"] for k in range(lo, lo + len(t.children))] == t.children
    return nodes, names, chunks, want_files, want_err


def _chain(rs, b, kind, name, pieces):
    """A hand-cut sibling chain: pieces = lists of child hashes; returns the first piece's hash."""
    nxt = None
    for part in reversed(pieces):
        data = rs.oracle.tree_serialize(kind, name, None, 1234, None, b"".join(part), nxt)
        nxt = b.add_raw_tree(data, blob_hash=rs.oracle.blake3(data))
    return nxt


def test_sibling_chains_and_node_order(ctx, rs):
    rng = np.random.default_rng(6)
    b = rs.store.Builder(seed=6)
    ch = [b.add(blob_bytes(rng, 10 + k)) for k in range(9)]
    f1 = _chain(rs, b, 0, "one", [ch[:3]])
    f2 = _chain(rs, b, 0, "two", [ch[:2], []])
    f5 = _chain(rs, b, 0, "five", [ch[2:4], [], ch[4:5], ch[5:8], []])
    sub = b.add_dir("sub", {"deep": {"x": blob_bytes(rng, 1), "y": blob_bytes(rng, 3000), "none": b""}, "z": blob_bytes(rng, 2500)})
    d3 = _chain(rs, b, 1, "dir3", [[f1], [], [sub, f2]])                 # a directory in three pieces
    root = _chain(rs, b, 1, "", [[f5, d3], [b.add_file("last", blob_bytes(rng, 700))]])
    packs, index = b.finish(target=9)
    ref = rs.ref.Store(rs.PRK, packs, index)
    for slots in (1, 2, 0):
        s, _ = open_session(ctx, rs, packs, index, slots=slots)
        nodes, names, chunks, want_files, _ = _compare_walk(rs, s, ref, root)
        paths = [p.replace(os.sep, "/") for p in rs.restore.walk_paths(nodes, names)]
        assert paths == ["", "five", "dir3", "last", "dir3/one", "dir3/sub", "dir3/two", "dir3/sub/deep", "dir3/sub/z",
                         "dir3/sub/deep/x", "dir3/sub/deep/y", "dir3/sub/deep/none"]
        s.close()
    got, errors = ctx.restore_unpack(rs.PRK, [p for _, p in packs], [i for i, _ in packs],
                                     ctx.unpack_headers(rs.PRK, [p for _, p in packs], [i for i, _ in packs]),
                                     rs.store.items_array(index), root, slots=2)
    assert not errors and {k.replace(os.sep, "/"): v for k, v in got.items()} == want_files


def test_file_of_25001_children_over_three_pieces(ctx, rs):
    rng = np.random.default_rng(7)
    b = rs.store.Builder(seed=7)
    blobs = [blob_bytes(rng, n) for n in (1, 2, 7, 16, 23, 39, 40)]
    hs = [b.add(x) for x in blobs]
    pick = rng.integers(0, 7, 25001)
    big = b.add_tree(0, "big", None, None, None, [hs[k] for k in pick])
    root = b.add_tree(1, "", None, None, None, [big])
    packs, index = b.finish()
    s, entries = open_session(ctx, rs, packs, index)
    nodes, names, chunks = s.trees(root)
    assert len(nodes) == 2 and int(nodes[1]["n_children"]) == 25001
    assert chunks.tobytes() == b"".join(hs[k] for k in pick)
    data, st, bad = s.files(chunks, [0, 25001])
    assert not st.any() and data[0] == b"".join(blobs[k] for k in pick)
    s.close()


def test_walk_errors(ctx, rs):
    b = rs.store.Builder(seed=8)
    chunk = b.add(b"just a chunk")
    file_root = b.add_file("f", b"abc" * 500)
    dir_chunk = b.add_tree(1, "", None, None, None, [chunk])
    ha, hb, hd = b"\xaa" * 32, b"\xbb" * 32, b"\xdd" * 32
    b.add_raw_tree(_tree(rs, kind=0, children=chunk, sib=hb), blob_hash=ha)   # a sibling cycle a -> b -> a
    b.add_raw_tree(_tree(rs, kind=0, children=chunk, sib=ha), blob_hash=hb)
    b.add_raw_tree(_tree(rs, kind=1, name=b"self", children=hd), blob_hash=hd)  # a directory that contains itself
    outer = b.add_tree(1, "", None, None, None, [file_root, hd])
    packs, index = b.finish(target=4)
    ref = rs.ref.Store(rs.PRK, packs, index)
    s, entries = open_session(ctx, rs, packs, index, slots=2)
    # a root of kind File: one node; the reference restores nothing
    nodes, names, chunks = s.trees(file_root)
    assert len(nodes) == 1 and nodes[0]["kind"] == 0 and len(chunks) == nodes[0]["n_children"] > 1
    files, ids = [p for _, p in packs], [i for i, _ in packs]
    assert ctx.restore_unpack(rs.PRK, files, ids, entries, rs.store.items_array(index), file_root) == ({}, [])
    assert rs.ref.unpack(ref, file_root)[1] == {}
    for root, reason, blame in ((b"\x01" * 32, rs.ref.ENOTFOUND, b"\x01" * 32), (dir_chunk, rs.ref.ENOTTREE, chunk),
                                (ha, rs.ref.EFORMAT, None), (hd, rs.ref.EFORMAT, hd), (outer, rs.ref.EFORMAT, hd)):
        with pytest.raises(rs.ref.RestoreError) as w:
            rs.ref.unpack(ref, root, max_pieces=len(entries))
        assert w.value.reason == reason
        with pytest.raises(rs.restore.TreeError) as x:
            s.trees(root)
        assert x.value.reason == reason and (blame is None or x.value.hash == blame), (root.hex(), x.value.reason)
    s.close()


# ------------------------------------------------------------------ gather geometry
@pytest.fixture(scope="module")
def geometry(rs):
    """Blobs of the lengths at which the gather changes path, one of exactly 3 MiB."""
    rng = np.random.default_rng(9)
    lens = [0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 2, 18, 33, 32768, 32769, 100000, MIB3]
    b = rs.store.Builder(seed=9)
    blobs = {n: blob_bytes(rng, n) for n in lens}
    hs = {n: b.add(blobs[n]) for n in lens}
    packs, index = b.finish()
    return blobs, hs, packs, index


def _run_device(ctx, rs, s, rows, ff, total, flags=0, slack=4096, cap=None):
    import torch
    cap = total if cap is None else cap
    d = torch.full((cap + slack,), 0xA5, dtype=torch.uint8, device="cuda")
    res = s.files_device(np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 32) if rows else np.zeros((0, 32), np.uint8),
                         ff, d.data_ptr(), cap, flags=flags)
    torch.cuda.synchronize()
    return res, d.cpu().numpy()


def test_gather_lengths_repeats_and_slots(ctx, rs, geometry):
    blobs, hs, packs, index = geometry
    L = sorted(blobs)
    files = [[], [0], [1], [15, 16, 17], [63, 64, 65, 4095], [4096, 4097, 4097, 1], [MIB3, 1, MIB3], [], [100000, 17, 32768, 32769, 17],
             [17], [0, 0, 1, 0], L, [65, 65, 65]]
    rows = [hs[n] for f in files for n in f]
    ff = np.concatenate([[0], np.cumsum([len(f) for f in files])])
    want = [b"".join(blobs[n] for n in f) for f in files]
    total = sum(len(w) for w in want)
    outs = []
    for slots, flags in ((1, 0), (2, rs.lib.BW_RESTORE_SKEW_SLOTS), (4, 0), (0, 0), (0, rs.lib.BW_RESTORE_SKEW_SLOTS)):
        s, _ = open_session(ctx, rs, packs, index, slots=slots)
        (rc, done, off, ln, st, bad), buf = _run_device(ctx, rs, s, rows, ff, total, flags)
        assert rc == 0 and done == len(files) and not st.any() and (bad == 2**64 - 1).all()
        assert list(ln) == [len(w) for w in want] and list(off) == list(np.concatenate([[0], np.cumsum(ln[:-1])]))
        assert buf[:total].tobytes() == b"".join(want)
        assert (buf[total:] == 0xA5).all()                                # the canary behind the last file and the cap
        outs.append(buf[:total].tobytes())
        s.close()
    assert all(o == outs[0] for o in outs)


def test_gather_every_source_and_destination_alignment(ctx, rs, geometry):
    """With BW_RESTORE_SKEW_SLOTS the k-th distinct blob of a call is decoded k mod 16 bytes past a
    16-byte boundary; with one slot every row is a sub-batch of its own, so row i's source starts at
    i mod 16.  Lengths of 1 mod 16, every 16th row 2 mod 16, walk the destination through every
    residue against every source residue."""
    blobs, hs, packs, index = geometry
    cyc = [17, 65, 4097, 1, 33]
    lens = [(18 if i % 32 == 15 else 2) if i % 16 == 15 else cyc[i % 5] for i in range(16 * 17)]
    assert all(a != b for a, b in zip(lens, lens[1:]))
    dst = np.concatenate([[0], np.cumsum(lens[:-1])])
    assert len({(i & 15, int(d) & 15) for i, d in enumerate(dst)}) == 256
    rows = [hs[n] for n in lens]
    ff = np.arange(len(lens) + 1)
    want = b"".join(blobs[n] for n in lens)
    s, _ = open_session(ctx, rs, packs, index, slots=1)
    (rc, done, off, ln, st, bad), buf = _run_device(ctx, rs, s, rows, ff, len(want), rs.lib.BW_RESTORE_SKEW_SLOTS)
    assert rc == 0 and not st.any() and list(off) == list(dst)
    assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xA5).all()
    # the 3 MiB blob at every odd pairing once more: many pieces, unaligned on both sides
    rows = [hs[1], hs[MIB3], hs[2], hs[MIB3]]
    (rc, done, off, ln, st, bad), buf = _run_device(ctx, rs, s, rows, [0, 4], 2 * MIB3 + 3, rs.lib.BW_RESTORE_SKEW_SLOTS)
    assert rc == 0 and buf[:2 * MIB3 + 3].tobytes() == blobs[1] + blobs[MIB3] + blobs[2] + blobs[MIB3]
    assert (buf[2 * MIB3 + 3:] == 0xA5).all()
    s.close()


def test_window_resumes_at_file_boundaries(ctx, rs, geometry):
    blobs, hs, packs, index = geometry
    files = [[4097, 17], [65], [], [100000, 1], [4096], [63, 64]]
    want = [b"".join(blobs[n] for n in f) for f in files]
    rows = np.frombuffer(b"".join(hs[n] for f in files for n in f), dtype=np.uint8).reshape(-1, 32)
    ff = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.uint64)
    ends = np.cumsum([len(w) for w in want])
    s, _ = open_session(ctx, rs, packs, index, slots=2)
    import torch
    for cap in sorted({int(e) for e in ends} | {int(e) - 1 for e in ends} | {100, 0}):
        got, at, calls = [], 0, 0
        while at < len(files):
            d = torch.full((max(cap, len(want[at])) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            rc, done, off, ln, st, bad = s.files_device(rows, ff[at:], d.data_ptr(), cap)
            calls += 1
            if rc == rs.lib.BW_ENOSPC and done == 0:                      # one file larger than the window
                assert ln[0] > cap and ln[0] <= len(want[at])
                rc, done, off, ln, st, bad = s.files_device(rows, ff[at:at + 2], d.data_ptr(), len(want[at]))
                assert rc == 0 and done == 1
            else:
                fit = 0
                while at + fit < len(files) and sum(len(w) for w in want[at:at + fit + 1]) <= cap:
                    fit += 1
                assert done == fit and rc == (0 if at + fit == len(files) else rs.lib.BW_ENOSPC), (cap, at, done, fit)
            buf = d.cpu().numpy()
            assert (buf[max(cap, len(want[at])):] == 0xA5).all()
            got += [buf[int(off[k]):int(off[k] + ln[k])].tobytes() for k in range(done)]
            at += done
            assert calls <= 12
        assert got == want, cap
    s.close()


# ------------------------------------------------------------------ per-file failures
def test_per_file_failures_match_the_reference(ctx, rs):
    rng = np.random.default_rng(10)
    b = rs.store.Builder(seed=10)
    data = [blob_bytes(rng, 200 + 37 * k) for k in range(12)]
    hs = [None] * 12
    for k in range(12):
        if k == 4:
            hs[k] = b.add(data[k], payload=b"\x00\x00\x07\x00\x00")       # sealed properly, not a frame: EZSTD
        elif k == 9:
            hs[k] = b.add(data[k], blob_hash=rs.oracle.blake3(data[k]), payload=rs.po.zstd_store(data[3]))  # EDIGEST
        else:
            hs[k] = b.add(data[k])
    packs, index = b.finish(target=5)
    index = [(h, pid) for h, pid in index if h != hs[7]]                  # absent from the index
    files_ids = [i for i, _ in packs]
    entries = ctx.unpack_headers(rs.PRK, [p for _, p in packs], files_ids)
    e = [x for x in entries if x["hash"].tobytes() == hs[1]][0]          # one flipped byte in a sealed blob: ETAG
    p = int(e["packfile"])
    raw = bytearray(packs[p][1])
    raw[8 + struct.unpack_from("<Q", raw, 0)[0] + int(e["offset"]) + 12 + int(e["length"]) - 3] ^= 0x40
    packs[p] = (packs[p][0], bytes(raw))
    files = [[0, 2, 3], [0, 1, 2], [2, 4, 5, 4], [5, 6], [7], [6, 8, 7, 8], [9, 10], [10, 9, 11], [11, 0], []]
    rows = np.frombuffer(b"".join(hs[k] for f in files for k in f), dtype=np.uint8).reshape(-1, 32)
    ff = np.concatenate([[0], np.cumsum([len(f) for f in files])])
    for verify in (False, True):
        ref = rs.ref.Store(rs.PRK, packs, index, verify=verify)
        want = [rs.ref.restore_file(ref, rs.ref.Tree(0, "", None, None, None, [hs[k] for k in f], None)) for f in files]
        assert {w[1] for w in want} == {0, rs.ref.ETAG, rs.ref.EZSTD, rs.ref.ENOTFOUND} | ({rs.ref.EDIGEST} if verify else set())
        for slots in (1, 3, 0):
            s = rs.restore.Session(ctx, rs.PRK, [p for _, p in packs], files_ids, entries, rs.store.items_array(index), slots=slots)
            got, st, bad = s.files(rows, ff, flags=rs.lib.BW_UNPACK_VERIFY if verify else 0)
            for k, (g, w) in enumerate(zip(got, want)):
                assert (g, int(st[k]), None if bad[k] == 2**64 - 1 else int(bad[k])) == w, (verify, slots, k)
            s.close()


# ------------------------------------------------------------------ write then read on the device
def test_write_then_read_on_the_device(ctx, rs, tmp_path):
    import torch
    from backuwup_amd.context import make_params, make_tree, tree_serialize
    rng = np.random.default_rng(11)
    sizes = [0, 1, 2 << 20, 5000] + [int(x) for x in rng.integers(0, 1 << 20, 36)]
    datas = [blob_bytes(rng, n) for n in sizes]
    datas[7] = datas[6]                                                  # one file twice: every chunk shared
    names = ["f%02d.bin" % i for i in range(len(sizes))]
    mt = [1_500_000_000 + 1000 * i for i in range(len(sizes))]
    lens = np.array([len(d) for d in datas], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    host = np.frombuffer(b"".join(datas), dtype=np.uint8)
    ctx.index_reset()
    recs = ctx.process_files(host, offs, lens, make_params(4096, 16384, 65536, small_file_threshold=0))
    # trees: a file per input in one subdirectory each third, all below the root
    by_file = [recs[recs["file"] == i] for i in range(len(sizes))]
    trees = [make_tree(0, names[i], len(datas[i]), mt[i], None, by_file[i]["digest"].tobytes()) for i in range(len(sizes))]
    fh, _ = ctx.tree_blobs(trees, dedup=False)
    sub = [make_tree(1, "dir%d" % g, None, 1_400_000_000 + g, None, fh[g::3].tobytes()) for g in range(3)]
    sh, _ = ctx.tree_blobs(sub, dedup=False)
    root_t = [make_tree(1, "", None, None, None, sh.tobytes())]
    rh, _ = ctx.tree_blobs(root_t, dedup=False)
    tree_bytes = [tree_serialize(t) for t in trees + sub + root_t]
    tree_hash = [bytes(h) for h in list(fh) + list(sh) + list(rh)]
    # the queue of unique blobs: chunks, then tree blobs
    uniq = recs[recs["is_dup"] == 0]
    q_hash = [bytes(r["digest"]) for r in uniq]
    q_src = [host[int(offs[int(r["file"])] + r["offset"]):int(offs[int(r["file"])] + r["offset"] + r["length"])].tobytes() for r in uniq]
    seen = set(q_hash)
    kinds = [0] * len(q_hash)
    for h, t in zip(tree_hash, tree_bytes):
        if h not in seen:
            seen.add(h)
            q_hash.append(h)
            q_src.append(t)
            kinds.append(1)
    ql = np.array([len(x) for x in q_src], dtype=np.uint64)
    qo = np.concatenate([[0], np.cumsum(ql[:-1])]).astype(np.uint64)
    d_src = torch.from_numpy(np.frombuffer(b"".join(q_src) + bytes(16), dtype=np.uint8).copy()).cuda()
    fl = ctx.pack_compress_device(d_src.data_ptr(), qo, ql)
    plan, total = ctx.pack_plan(fl, flags=0)
    ids = rng.integers(0, 256, (len(plan), 12), dtype=np.uint8)
    nonces = rng.integers(0, 256, (len(q_hash), 12), dtype=np.uint8)
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    ctx.pack_build_compressed(rs.PRK, np.frombuffer(b"".join(q_hash), dtype=np.uint8).reshape(-1, 32), kinds, nonces, plan, ids,
                              d_out.data_ptr())
    torch.cuda.synchronize()
    which = np.zeros(len(q_hash), dtype=np.int64)
    for k, p in enumerate(plan):
        which[int(p["first_blob"]):int(p["first_blob"] + p["n_blobs"])] = k
    items = np.concatenate([np.frombuffer(b"".join(q_hash), dtype=np.uint8).reshape(-1, 32), ids[which]], axis=1)
    index_files = ctx.index_files_build(rs.PRK, items)
    # the read side, from what was written
    loaded = ctx.index_load_files(rs.PRK, index_files)
    assert len(loaded) == len(q_hash)
    buf = d_out.cpu().numpy().tobytes()
    pf_bytes = [buf[int(p["offset"]):int(p["offset"] + p["size"])] for p in plan]
    entries = ctx.unpack_headers(rs.PRK, pf_bytes, [bytes(i) for i in ids])
    got, errors = rs.restore.unpack(ctx, d_out.data_ptr(), ids, entries, loaded, rs.PRK, bytes(rh[0]), plan=plan, verify=True)
    want = {"dir%d/%s" % (i % 3, names[i]): datas[i] for i in range(len(sizes))}
    assert not errors and {k.replace(os.sep, "/"): v for k, v in got.items()} == want
    dest = tmp_path / "restored"
    none, errors = rs.restore.unpack(ctx, d_out.data_ptr(), ids, entries, loaded, rs.PRK, bytes(rh[0]), str(dest), plan=plan,
                                     window=3 << 20)
    assert none is None and not errors
    for i in range(len(sizes)):
        p = dest / ("dir%d" % (i % 3)) / names[i]
        assert p.read_bytes() == datas[i] and int(p.stat().st_mtime) == mt[i]
    assert sorted(x.name for x in dest.iterdir()) == ["dir0", "dir1", "dir2"]
