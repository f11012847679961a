"""Prune on the device (bw_prune_mark, bw_prune_plan, bw_prune_repack) against tests/prune_ref.py over
the same packfiles: live bits, per-packfile sums, counts and the error records as a multiset.  All
stores are small; the shapes are the smallest at which each kernel can go wrong."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]
NONE = 2**64 - 1


@pytest.fixture(scope="module")
def pr(oracle):
    import prune_ref
    import restore_ref
    import restore_store
    from backuwup_amd import _lib, prune, restore

    class NS:
        pass
    ns = NS()
    ns.pref, ns.ref, ns.store, ns.lib, ns.prune, ns.restore = prune_ref, restore_ref, restore_store, _lib, prune, restore
    ns.po, ns.oracle, ns.PRK = restore_store.po, oracle, restore_store.PRK
    return ns


def open_session(ctx, pr, packs, index, slots=0):
    files, ids = [b for _, b in packs], [i for i, _ in packs]
    entries = ctx.unpack_headers(pr.PRK, files, ids)
    return pr.restore.Session(ctx, pr.PRK, files, ids, entries, pr.store.items_array(index), slots=slots), entries


def blob_bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _tree(pr, kind=0, name=b"n", children=b"", sib=None):
    return pr.oracle.tree_serialize(kind, name, None, None, None, children, sib)


def err_multiset(errs):
    return Counter((e["hash"].tobytes(), e["parent"].tobytes(), int(e["child_pos"]), int(e["reason"])) for e in errs)


def check_mark(pr, s, packs, index, roots, verify=False, hd=None):
    """mark() against prune_ref.mark: everything the call returns.  -> (live set, errors, info, counts)"""
    live, stats, counts, errs = pr.prune.mark(s, roots, verify=verify)
    hd = hd or pr.pref.headers_of(pr.PRK, packs)
    want, werrs, info = pr.pref.mark(pr.ref.Store(pr.PRK, packs, index, verify=verify), hd, roots)
    got = set(int(e) for e in np.flatnonzero(live))
    assert got == want, (sorted(got - want), sorted(want - got))
    assert [tuple(int(x) for x in st) for st in stats] == info["stats"]
    assert counts["n_trees_expanded"] == info["n_trees_expanded"] and counts["n_levels"] == info["n_levels"]
    assert counts["n_errors"] == sum(werrs.values()) == len(errs)
    assert err_multiset(errs) == werrs
    for k, f in enumerate(("live_blobs", "live_bytes", "total_blobs", "total_bytes")):
        assert counts[f] == sum(st[k] for st in info["stats"])
    return want, werrs, info, counts


# ------------------------------------------------------------------ 1. shared snapshots
@pytest.fixture(scope="module")
def snapshots(pr):
    rng = np.random.default_rng(31)
    shared = {"docs": {"a.txt": blob_bytes(rng, 3000), "b.txt": blob_bytes(rng, 700), "empty": b""},
              "src": {"m.c": blob_bytes(rng, 5000), "deep": {"x": blob_bytes(rng, 100)}}}
    spec_a = dict(shared, only_a=blob_bytes(rng, 2500))
    spec_b = dict(shared, only_b={"y": blob_bytes(rng, 1800)})
    b = pr.store.Builder(seed=31)
    root_a, root_b = b.add_dir("", spec_a), b.add_dir("", spec_b)
    packs, index = b.finish(target=7)
    return packs, index, root_a, root_b, spec_a, spec_b


def test_shared_snapshots(ctx, pr, snapshots):
    packs, index, root_a, root_b, _, _ = snapshots
    s, entries = open_session(ctx, pr, packs, index)
    trees = {k for k, e in enumerate(entries) if e["kind"] == pr.lib.BW_BLOB_TREE}
    lives = {}
    for name, roots in (("a", [root_a]), ("b", [root_b]), ("ab", [root_a, root_b]), ("ba", [root_b, root_a, root_a]), ("none", [])):
        live, errs, info, counts = check_mark(pr, s, packs, index, roots)
        assert not errs and counts["n_trees_expanded"] == len(live & trees)   # each distinct tree blob once
        lives[name] = live
    assert not lives["none"] and lives["ab"] == lives["ba"] == lives["a"] | lives["b"] == set(range(len(entries)))
    assert lives["a"] - lives["b"] and lives["b"] - lives["a"]
    s.close()


# ------------------------------------------------------------------ 2. shapes
def test_shapes_chain_empty_file_file_root_and_one_hash_many_times(ctx, pr):
    rng = np.random.default_rng(32)
    b = pr.store.Builder(seed=32)
    hs = [b.add(blob_bytes(rng, n)) for n in (1, 2, 7, 16, 23, 39, 40)]
    pick = rng.integers(0, 7, 25001)
    big = b.add_tree(0, "big", None, None, None, [hs[k] for k in pick])       # three pieces, as restore's test builds it
    empty = b.add_file("empty", b"")
    sub = b.add_dir("sub", {"f": blob_bytes(rng, 900)})
    many = b.add_tree(1, "many", None, None, None, [sub] * 300)                # one hash, 300 children of one level
    root = b.add_tree(1, "", None, None, None, [big, empty, many])
    packs, index = b.finish()
    s, entries = open_session(ctx, pr, packs, index)
    live, errs, info, counts = check_mark(pr, s, packs, index, [root])
    assert not errs and live == set(range(len(entries)))
    assert counts["n_trees_expanded"] == 3 + 1 + 1 + 2 + 1                     # big's pieces, empty, many, sub + f, root
    assert counts["n_levels"] == 4                                             # root; big, empty, many; piece 2, sub; piece 3, f
    live, errs, info, counts = check_mark(pr, s, packs, index, [big])          # a root of kind File
    assert not errs and counts["n_trees_expanded"] == 3 and len(live) == 3 + 7
    live, errs, info, counts = check_mark(pr, s, packs, index, [empty])
    assert len(live) == 1 and counts["n_levels"] == 1
    s.close()


# ------------------------------------------------------------------ 3. the two-bit trap
def test_tree_blob_first_named_as_a_files_chunk_is_still_expanded(ctx, pr):
    b = pr.store.Builder(seed=33)
    leaf = b.add(b"leaf chunk of the hidden subtree")
    hidden_file = b.add_tree(0, "hf", None, None, None, [leaf])
    hidden = b.add_tree(1, "hidden", None, None, None, [hidden_file])
    trap = b.add_tree(0, "trap", None, None, None, [hidden])       # level 1: a File whose chunk is the tree blob
    late = b.add_tree(1, "late", None, None, None, [hidden])       # level 2: a Dir that names it as a child
    mid = b.add_tree(1, "mid", None, None, None, [late])
    root = b.add_tree(1, "", None, None, None, [trap, mid])
    packs, index = b.finish(target=3)
    s, entries = open_session(ctx, pr, packs, index)
    live, errs, info, counts = check_mark(pr, s, packs, index, [root])
    assert not errs and live == set(range(7)) and counts["n_trees_expanded"] == 6
    live, errs, info, counts = check_mark(pr, s, packs, index, [trap])
    assert len(live) == 2 and counts["n_trees_expanded"] == 1
    s.close()


# ------------------------------------------------------------------ 4. frontier sub-batching and compaction
def test_sub_batches_of_four_slots_and_compaction_with_holes(ctx, pr):
    """slots = 4: a level of 11 tree blobs goes 4 + 4 + 3.  A directory of 333 children (more than one
    workgroup of 256 lanes, not a multiple of 64) is expanded two levels after every third child was
    queued through another root, so the ballots have holes across wave and workgroup boundaries."""
    b = pr.store.Builder(seed=34)
    chunk = b.add(b"shared chunk")
    kids = [b.add_tree(0, "f%03d" % k, 12, None, None, [chunk]) for k in range(333)]
    big = b.add_tree(1, "big", None, None, None, kids)
    deep = b.add_tree(1, "", None, None, None, [b.add_tree(1, "d", None, None, None, [big])])
    third = b.add_tree(1, "", None, None, None, kids[1::3])
    eleven = b.add_dir("", {"g%d" % k: bytes([k]) * 50 for k in range(11)})
    packs, index = b.finish(target=50)
    s, entries = open_session(ctx, pr, packs, index, slots=4)
    live, errs, info, counts = check_mark(pr, s, packs, index, [eleven])
    assert not errs and counts["n_trees_expanded"] == 12 and counts["n_levels"] == 2
    live, errs, info, counts = check_mark(pr, s, packs, index, [third, deep])
    assert not errs and counts["n_trees_expanded"] == 333 + 4 and counts["n_levels"] == 4
    only_deep, _, _, c2 = check_mark(pr, s, packs, index, [deep])
    assert c2["n_trees_expanded"] == 333 + 3 and len(live - only_deep) == 1
    s.close()


# ------------------------------------------------------------------ 5. duplicate hashes
def test_duplicate_hashes_mark_the_entry_locate_returns(ctx, pr):
    rng = np.random.default_rng(35)
    b = pr.store.Builder(seed=35)
    data = [blob_bytes(rng, 40 + k) for k in range(6)]
    hs = [b.add(d) for d in data]
    b.add(data[1], again=True)            # twice in one header (target 8)
    b.add(b"filler")
    b.add(data[2], again=True)            # and in a second packfile
    b.add(data[1], again=True)
    f = b.add_tree(0, "f", None, None, None, hs)
    root = b.add_tree(1, "", None, None, None, [f])
    packs, index = b.finish(target=8)
    s, entries = open_session(ctx, pr, packs, index)
    hashes = [e["hash"].tobytes() for e in entries]
    assert hashes.count(hs[1]) == 3 and hashes.count(hs[2]) == 2 and len({int(e["packfile"]) for e in entries}) == 2
    live, errs, info, counts = check_mark(pr, s, packs, index, [root])
    idx, st = s.locate(hs)
    assert not st.any() and not errs
    for h, want in zip(hs, idx):
        assert [k for k in live if hashes[k] == h] == [int(want)]    # exactly one entry per hash, the located one
    assert len(live) == 6 + 2 and len(entries) == 6 + 3 + 1 + 2
    s.close()


# ------------------------------------------------------------------ 6. errors
@pytest.fixture(scope="module")
def damaged(pr):
    """One store where the walk must carry on past every kind of damage.  Every bad node has a good
    sibling behind it."""
    rng = np.random.default_rng(36)
    b = pr.store.Builder(seed=36)
    good = [b.add_file("good%d" % k, blob_bytes(rng, 600 + k)) for k in range(10)]
    chunk = b.add(b"a chunk a Dir names")
    absent_tree, absent_chunk = b"\x01" * 32, b"\x02" * 32
    nopack_chunk, mismatch_chunk = b.add(b"indexed under an absent id"), b.add(b"indexed under the wrong packfile")
    f_missing = b.add_tree(0, "fm", None, None, None, [absent_chunk, chunk, nopack_chunk, mismatch_chunk])
    flipped = b.add_tree(1, "flipped", None, None, None, [good[0]])
    malformed = b.add_raw_tree(b"\x02not a tree")
    forged = b.add_raw_tree(_tree(pr, kind=1, name=b"forged", children=good[1]), blob_hash=b"\x04" * 32)
    top = b.add_tree(1, "", None, None, None, [good[2], absent_tree, good[3], chunk, good[4], flipped, good[5], malformed,
                                               good[6], forged, good[7], f_missing, good[8]])
    cut = b.add(blob_bytes(rng, 500))                               # the store's last blob: its packfile is cut short
    f_cut = b.add_tree(0, "fc", None, None, None, [cut, chunk])
    b.blobs[-2], b.blobs[-1] = b.blobs[-1], b.blobs[-2]
    root = top
    packs, index = b.finish(target=9)
    flat = [h for h, _ in index]
    # the tag byte of `flipped`
    hd = pr.pref.headers_of(pr.PRK, packs)
    for p, (_, _, hl, ents) in enumerate(hd):
        for h, _, _, length, offset in ents:
            if h == flipped:
                buf = bytearray(packs[p][1])
                buf[8 + hl + offset + 12 + length - 1] ^= 1
                packs[p] = (packs[p][0], bytes(buf))
    assert hd[-1][3][-1][0] == cut
    packs[-1] = (packs[-1][0], packs[-1][1][:-5])
    other = next(pid for pid, _ in packs if pid != dict(index)[mismatch_chunk])
    index = [(h, b"\xee" * 12 if h == nopack_chunk else other if h == mismatch_chunk else pid) for h, pid in index]
    assert len(flat) == len(index)
    return packs, index, [root, f_cut], dict(good=good, chunk=chunk, flipped=flipped, forged=forged, cut=cut)


def test_errors_never_stop_the_walk(ctx, pr, damaged):
    packs, index, roots, names = damaged
    R = pr.ref
    s, entries = open_session(ctx, pr, packs, index, slots=3)
    hashes = [e["hash"].tobytes() for e in entries]
    for verify in (False, True):
        live, errs, info, counts = check_mark(pr, s, packs, index, roots, verify=verify)
        reasons = Counter(k[3] for k in errs.elements())
        want = {R.ENOTFOUND: 2, R.ENOPACKFILE: 1, R.EMISMATCH: 1, R.ENOTTREE: 1, R.ETAG: 1, R.EFORMAT: 1, R.ERANGE: 1}
        if verify:
            want[R.EDIGEST] = 1
        assert reasons == want
        live_hashes = {hashes[k] for k in live}
        assert names["chunk"] in live_hashes and names["flipped"] in live_hashes and names["cut"] in live_hashes
        # the siblings of every bad node are marked; what only the forged tree names is live unless verify refuses it
        assert all((g in live_hashes) == (k != 0 and (k != 1 or not verify) and k != 9) for k, g in enumerate(names["good"]))
    # err_cap one below the count: BW_ENOSPC, everything else filled
    n = counts["n_errors"]
    live2, stats2, counts2, errs2 = pr.prune.mark(s, roots, verify=True, err_cap=n - 1)
    assert counts2 == counts and len(errs2) == n - 1 and set(int(e) for e in np.flatnonzero(live2)) == live
    assert [tuple(int(x) for x in st) for st in stats2] == info["stats"]
    assert not err_multiset(errs2) - errs
    import ctypes
    cnt = pr.lib.BwPruneCounts()
    r = np.frombuffer(b"".join(roots), dtype=np.uint8)
    lv, st = np.zeros(len(entries), np.uint8), np.zeros(len(packs), pr.prune.STAT_DTYPE)
    eb = np.zeros(n, pr.prune.ERROR_DTYPE)
    rc = s._L.bw_prune_mark(s.h, r.ctypes.data, len(roots), 1, lv.ctypes.data_as(pr.lib.u8p),
                            st.ctypes.data_as(ctypes.POINTER(pr.lib.BwPrunePackfileStat)), ctypes.byref(cnt),
                            eb.ctypes.data_as(ctypes.POINTER(pr.lib.BwPruneError)), n - 1)
    assert rc == pr.lib.BW_ENOSPC and cnt.n_errors == n
    s.close()


def test_more_errors_than_the_device_list_holds(ctx, pr):
    """The device's error list holds 65,536 records whatever err_cap is; a walk that meets more is run again
    with a list of the size it needs.  One File of 66,000 absent chunks (seven pieces) and one good one."""
    rng = np.random.default_rng(40)
    b = pr.store.Builder(seed=40)
    good = b.add(b"the one chunk that is there")
    absent = [blob_bytes(rng, 32) for _ in range(66000)]
    huge = b.add_tree(0, "huge", None, None, None, absent[:33000] + [good] + absent[33000:])
    packs, index = b.finish()
    s, entries = open_session(ctx, pr, packs, index)
    live, errs, info, counts = check_mark(pr, s, packs, index, [huge])
    assert counts["n_errors"] == 66000 and set(k[3] for k in errs) == {pr.ref.ENOTFOUND} and len(live) == 7 + 1
    live2, _, counts2, errs2 = pr.prune.mark(s, [huge], err_cap=65536 + 100)     # between the list's size and the count
    assert counts2 == counts and len(errs2) == 65636 and not err_multiset(errs2) - errs
    s.close()


def test_spare_packfile_ids_do_not_add_packfiles(ctx, pr, snapshots):
    packs, index, root_a, _, _, _ = snapshots
    files, ids = [b for _, b in packs], [i for i, _ in packs]
    entries = ctx.unpack_headers(pr.PRK, files, ids)
    with pr.restore.Session(ctx, pr.PRK, files, ids + [b"\x99" * 12, b"\x98" * 12], entries, pr.store.items_array(index)) as s:
        assert s.n_packfiles == len(packs) and s.n_entries == len(entries)
        live, stats, counts, errs = pr.prune.mark(s, [root_a])
        assert len(stats) == len(packs) and len(pr.prune.choose_rewrite(stats)) == len(packs)


# ------------------------------------------------------------------ 7. cycles
def test_cycles_end_and_are_no_error(ctx, pr):
    b = pr.store.Builder(seed=37)
    chunk = b.add(b"just a chunk")
    ha, hb, hc, hd_, he = (bytes([x]) * 32 for x in (0xaa, 0xbb, 0xcc, 0xdd, 0xee))
    b.add_raw_tree(_tree(pr, kind=0, children=chunk, sib=hb), blob_hash=ha)    # a sibling cycle a -> b -> c -> a
    b.add_raw_tree(_tree(pr, kind=0, children=chunk, sib=hc), blob_hash=hb)
    b.add_raw_tree(_tree(pr, kind=0, children=chunk, sib=ha), blob_hash=hc)
    b.add_raw_tree(_tree(pr, kind=1, name=b"self", children=hd_ + he), blob_hash=hd_)  # a directory that contains itself
    b.add_raw_tree(_tree(pr, kind=1, name=b"back", children=hd_), blob_hash=he)        # and a cycle of two
    outer = b.add_tree(1, "", None, None, None, [ha, hd_])
    packs, index = b.finish(target=4)
    s, entries = open_session(ctx, pr, packs, index, slots=2)
    live, errs, info, counts = check_mark(pr, s, packs, index, [outer])
    assert not errs and live == set(range(len(entries))) and counts["n_trees_expanded"] == 6
    live, errs, info, counts = check_mark(pr, s, packs, index, [hb])
    assert not errs and len(live) == 4
    s.close()


# ------------------------------------------------------------------ 8. repack bytes
GEOMETRY = [0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 32767, 32768, 32769, 100000]


def build_tagged(pr, b, target, tag0=()):
    """Builder.finish with the compression tag 0 stored for the hashes in tag0."""
    n = len(b.blobs)
    groups = [(f, min(target, n - f)) for f in range(0, n, target)] if target else pr.po.plan_packfiles([len(x[3]) for x in b.blobs])
    ids = [bytes(b.rng.integers(0, 256, 12, dtype=np.uint8)) for _ in groups]
    packs = [(ids[g], pr.pref.serialize_packfile(pr.PRK, ids[g], [(h, k, 0 if h in tag0 else 1, nc, sl) for h, k, nc, sl in b.blobs[f:f + c]]))
             for g, (f, c) in enumerate(groups)]
    return packs, [(b.blobs[i][0], ids[g]) for g, (f, c) in enumerate(groups) for i in range(f, f + c)]


def repack_both_ways(ctx, pr, packs, index, live, rewrite, slack=4096):
    """plan + repack (host and device form) against prune_ref.repack; -> (plan, order, entries, new packs)"""
    import torch
    s, entries = open_session(ctx, pr, packs, index)
    hd = pr.pref.headers_of(pr.PRK, packs)
    lv = np.array([1 if e in live else 0 for e in range(len(entries))], dtype=np.uint8)
    tab = pr.prune.packfile_table([p for _, p in packs])
    order, plan, total = pr.prune.plan(entries, tab, lv, np.asarray(rewrite, dtype=np.uint8))
    ids = [bytes([0x40 + g]) * 12 for g in range(len(plan))]
    want, items, worder, groups = pr.pref.repack(pr.PRK, packs, hd, live, rewrite, ids)
    assert list(order) == worder and [(int(p["first_blob"]), int(p["n_blobs"])) for p in plan] == groups
    assert total == sum(len(w) for _, w in want)
    got = pr.prune.repack(s, order, plan, ids)
    assert len(got) == len(want)
    for g, (w, x) in enumerate(zip(want, got)):
        assert x == w[1], "new packfile %d differs (host form)" % g
    d = torch.full((total + slack,), 0xA5, dtype=torch.uint8, device="cuda")
    pr.prune.repack_device(s, order, plan, ids, d.data_ptr())
    torch.cuda.synchronize()
    buf = d.cpu().numpy()
    assert buf[:total].tobytes() == b"".join(w for _, w in want)
    assert (buf[total:] == 0xA5).all()                               # nothing behind total_bytes is written
    # an order or a plan that does not match the session's entries
    if order.size > 2:
        bad_plan = plan.copy()
        bad_plan[0]["size"] += 1
        for o, p in ((order[::-1].copy(), plan), (order[:-1], plan), (order, bad_plan),
                     (np.concatenate([order[:-1], [len(entries)]]).astype(np.uint64), plan)):
            with pytest.raises(pr.lib.BwError) as x:
                pr.prune.repack_device(s, o, p, ids, d.data_ptr())
            assert x.value.rc == pr.lib.BW_EINVAL
        torch.cuda.synchronize()
        assert (d.cpu().numpy()[total:] == 0xA5).all()
    s.close()
    return plan, order, entries, tab, d.data_ptr(), got


def test_repack_lengths_alignments_and_the_stored_compression_tag(ctx, pr):
    rng = np.random.default_rng(38)
    b = pr.store.Builder(seed=38)
    hs = []
    for n in GEOMETRY:                                               # every second blob is dead
        hs.append(b.add(blob_bytes(rng, n), payload=blob_bytes(rng, n)))   # payload length = the blob's payload bytes
        b.add(blob_bytes(rng, 1 + int(rng.integers(0, 40))))
    for pad in range(0, 400, 40):                                    # padding blobs until the pairs spread
        for k in range(40):
            h = b.add(blob_bytes(rng, 20 + pad + k), payload=blob_bytes(rng, int(rng.integers(0, 90))))
            if k % 2 == 0:
                hs.append(h)
        packs, index = build_tagged(pr, b, 60, tag0={hs[3]})
        hd = pr.pref.headers_of(pr.PRK, packs)
        ents = pr.pref.flat_entries(hd)
        live = {e for e, x in enumerate(ents) if x[1] in set(hs)}
        plan, order, entries, tab, d_ptr, got = repack_both_ways(ctx, pr, packs, index, live, [1] * len(packs))
        # (source mod 16, destination mod 16) of every moved blob: the session's upload is 16-byte aligned
        pairs = set()
        for p in plan:
            at = int(p["offset"] + 8 + p["header_len"])
            for e in order[int(p["first_blob"]):int(p["first_blob"] + p["n_blobs"])]:
                x = entries[int(e)]
                src = int(tab[int(x["packfile"])]["offset"] + 8 + tab[int(x["packfile"])]["header_len"] + x["offset"])
                pairs.add((src % 16, (d_ptr + at) % 16))
                at += 12 + int(x["length"])
        if len(pairs) >= 64:
            break
    assert len(pairs) >= 64, len(pairs)
    assert sorted(int(entries[int(e)]["length"]) - 16 for e in order[:len(GEOMETRY)]) == sorted(GEOMETRY)
    # the tag stored as 0 stays 0 in the new header
    new_entries = ctx.unpack_headers(pr.PRK, got, [bytes([0x40 + g]) * 12 for g in range(len(got))])
    tags = {e["hash"].tobytes(): int(e["compression"]) for e in new_entries}
    assert tags[hs[3]] == 0 and sorted(tags.values()).count(0) == 1 and len(tags) == len(order)


def test_repack_splits_at_the_oracles_boundary(ctx, pr):
    rng = np.random.default_rng(39)
    b = pr.store.Builder(seed=39)
    hs = [b.add(blob_bytes(rng, 10), payload=blob_bytes(rng, 99000 + 7 * k)) for k in range(80)]
    packs, index = b.finish()
    assert len(packs) >= 2
    n = len(hs)
    live = {e for e in range(n) if e % 2 == 0 or e > 70}
    plan, order, *_ = repack_both_ways(ctx, pr, packs, index, live, [1] * len(packs))
    assert len(plan) >= 2 and int(plan["size"].sum()) > 3 << 20
    # a packfile that is not rewritten keeps its dead blobs and contributes nothing
    plan2, order2, *_ = repack_both_ways(ctx, pr, packs, index, live, [0] + [1] * (len(packs) - 1))
    assert 0 < order2.size < order.size


# ------------------------------------------------------------------ 9. end to end
def test_prune_end_to_end(ctx, pr, snapshots):
    packs, index, root_a, root_b, spec_a, spec_b = snapshots
    files, ids = [b for _, b in packs], [i for i, _ in packs]
    entries = ctx.unpack_headers(pr.PRK, files, ids)
    items = pr.store.items_array(index)
    new_ids = [bytes([0x70 + g]) * 12 for g in range(4)]
    p2, i2, it2, rep = pr.prune.prune(ctx, files, ids, entries, items, pr.PRK, [root_a], new_ids, last_file_num=4)
    assert not len(rep["errors"]) and 0 < rep["order"].size < len(entries) and rep["rewrite"].any()
    kept = [p for p in range(len(ids)) if not rep["rewrite"][p]]
    assert p2[:len(kept)] == [files[p] for p in kept] and i2 == [ids[p] for p in kept] + new_ids[:len(rep["plan"])]
    # the headers of the pruned store parse; the kept root restores byte for byte
    e2 = ctx.unpack_headers(pr.PRK, p2, i2)
    assert len(e2) == int(rep["counts"]["live_blobs"]) + sum(int(rep["stats"][p]["total_blobs"] - rep["stats"][p]["live_blobs"]) for p in kept)
    got, errors = pr.restore.unpack(ctx, p2, i2, e2, it2, pr.PRK, root_a, verify=True)
    _, want, werr = pr.ref.unpack(pr.ref.Store(pr.PRK, packs, index), root_a)
    assert not errors and not werr and got == want == pr.store.flatten(spec_a)
    # what only the dropped root reached is gone
    with pr.restore.Session(ctx, pr.PRK, p2, i2, e2, it2) as s2:
        only_b = pr.oracle.blake3(spec_b["only_b"]["y"][:1])  # not a blob of the store at all
        dropped = [e["hash"].tobytes() for k, e in enumerate(entries) if not rep["live"][k]]
        assert dropped
        idx, st = s2.locate(dropped + [only_b])
        assert (st == pr.lib.BW_RESTORE_ENOTFOUND).all()
        with pytest.raises(pr.restore.TreeError) as x:
            s2.trees(root_b)
        assert x.value.reason == pr.lib.BW_RESTORE_ENOTFOUND
        # a second mark finds no dead byte in the new packfiles
        live, stats, counts, errs = pr.prune.mark(s2, [root_a])
        assert not len(errs) and all(int(st_["live_bytes"]) == int(st_["total_bytes"]) for st_ in stats[len(kept):])
        assert live.all()
    # and a second prune moves nothing
    p3, i3, it3, rep3 = pr.prune.prune(ctx, p2, i2, e2, it2, pr.PRK, [root_a], [b"\x7f" * 12])
    assert rep3["order"].size == 0 and p3 == p2 and i3 == i2 and it3.tobytes() == it2.tobytes()
    # the index items: the old ones of kept packfiles in the old order, then (hash, new id) per moved blob
    gone = {ids[p] for p in range(len(ids)) if rep["rewrite"][p]}
    old = [bytes(r) for r in items if bytes(r[32:]) not in gone]
    moved = [entries[int(e)]["hash"].tobytes() for e in rep["order"]]
    assert [bytes(r) for r in it2[:len(old)]] == old and [bytes(r[:32]) for r in it2[len(old):]] == moved
    # the index files are built and load back
    loaded = ctx.index_load_files(pr.PRK, rep["index_files"])
    assert np.asarray(loaded).reshape(-1, 44).tobytes() == it2.tobytes() and rep["index_files"][0][0] == 5


def test_prune_over_a_damaged_graph_is_a_decision(ctx, pr, damaged):
    packs, index, roots, _ = damaged
    files, ids = [b for _, b in packs], [i for i, _ in packs]
    entries = ctx.unpack_headers(pr.PRK, files, ids)
    items = pr.store.items_array(index)
    new_ids = [bytes([0x50 + g]) * 12 for g in range(4)]
    with pytest.raises(pr.prune.PruneError) as x:
        pr.prune.prune(ctx, files, ids, entries, items, pr.PRK, roots[:1], new_ids)
    assert len(x.value.errors) == 7
    p2, i2, it2, rep = pr.prune.prune(ctx, files, ids, entries, items, pr.PRK, roots[:1], new_ids, allow_errors=True)
    assert len(rep["errors"]) == 7 and rep["order"].size
