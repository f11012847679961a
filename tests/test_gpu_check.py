"""Check on the device (bw_check_structure, bw_check_data, backuwup_amd.check.check) against
tests/check_ref.py over the same packfiles, every output array elementwise.  check_ref decides tags
with OpenSSL, frames with libzstd and digests with the oracle's BLAKE3; tests/test_check.py pins it to
hand-written findings for the very stores used here (tests/check_stores.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]


@pytest.fixture(scope="module")
def ck(oracle):
    import check_ref
    import check_stores
    import prune_ref
    import restore_ref
    import restore_store
    from backuwup_amd import _lib, check, prune, restore

    class NS:
        pass
    ns = NS()
    ns.cr, ns.st, ns.pref, ns.rr, ns.store = check_ref, check_stores, prune_ref, restore_ref, restore_store
    ns.lib, ns.check, ns.prune, ns.restore, ns.PRK = _lib, check, prune, restore, check_stores.PRK
    return ns


def open_session(ctx, ck, packs, index, slots=0):
    """-> (session, headers as check_ref takes them).  The entries are the oracle's reading of the headers."""
    hd = ck.pref.headers_of(ck.PRK, packs)
    entries = ck.pref.entries_array(hd)
    s = ck.restore.Session(ctx, ck.PRK, [b for _, b in packs], [i for i, _ in packs], entries, ck.store.items_array(index),
                           slots=slots)
    return s, hd


def check_structure(ck, s, hd, index):
    """bw_check_structure against check_ref.structure: every array, every count."""
    flags, items, stats, counts = ck.check.structure(s)
    wf, wi, ws, wc = ck.cr.structure(hd, index)
    assert flags.tolist() == wf, [(e, int(flags[e]), wf[e]) for e in range(len(wf)) if flags[e] != wf[e]][:8]
    assert items.tolist() == wi, [(i, int(items[i]), wi[i]) for i in range(len(wi)) if items[i] != wi[i]][:8]
    assert [{k: int(st[k]) for k in ck.cr.STAT_FIELDS} for st in stats] == ws
    assert counts == wc
    return wf, wi, ws


def check_data(ck, s, packs, hd, select=None):
    """Both modes against check_ref.data, and the AUTH / FULL invariant over every selected entry."""
    out = []
    for mode in ("auth", "full"):
        got = ck.check.data(s, mode, select)
        want = ck.cr.data(ck.PRK, packs, hd, mode, select)
        assert got.tolist() == want, (mode, [(e, int(got[e]), want[e]) for e in range(len(want)) if got[e] != want[e]][:8])
        out.append(want)
    for a, f in zip(*out):
        if a != ck.cr.SKIPPED:
            assert (a == ck.rr.OK) == (f not in (ck.rr.ETAG, ck.rr.ERANGE))
        else:
            assert f == ck.cr.SKIPPED
    return out


# ------------------------------------------------------------------ clean stores
@pytest.fixture(scope="module")
def snapshots(ck):
    """The shared-snapshots store of the prune tests."""
    rng = np.random.default_rng(31)
    bb = ck.st.blob_bytes
    shared = {"docs": {"a.txt": bb(rng, 3000), "b.txt": bb(rng, 700), "empty": b""},
              "src": {"m.c": bb(rng, 5000), "deep": {"x": bb(rng, 100)}}}
    spec_a = dict(shared, only_a=bb(rng, 2500))
    spec_b = dict(shared, only_b={"y": bb(rng, 1800)})
    b = ck.store.Builder(seed=31)
    root_a, root_b = b.add_dir("", spec_a), b.add_dir("", spec_b)
    packs, index = b.finish(target=7)
    return packs, index, root_a, root_b


def test_clean_snapshots_store(ctx, ck, snapshots):
    packs, index = snapshots[:2]
    s, hd = open_session(ctx, ck, packs, index)
    wf, wi, ws = check_structure(ck, s, hd, index)
    assert not any(wf) and not any(wi) and all(st["tail"] == 0 for st in ws)
    auth, full = check_data(ck, s, packs, hd)
    assert not any(auth) and not any(full)
    s.close()


def test_one_packfile_of_300_entries(ctx, ck):
    """300 entries: the 64 / 65 wave border and more than one 256-lane workgroup inside one packfile."""
    packs, index = ck.st.one_packfile_of_300()
    s, hd = open_session(ctx, ck, packs, index)
    wf, wi, ws = check_structure(ck, s, hd, index)
    assert not any(wf) and ws[0]["n_entries"] == 300 and ws[0]["tail"] == 0
    # the same packfile with the offsets of entries 63 / 64 and 255 / 256 swapped, and entry 299 one byte late
    def edit(ents):
        for a in (63, 255):
            ents[a][4], ents[a + 1][4] = ents[a + 1][4], ents[a][4]
        ents[299][4] += 1
        return ents
    bad = [ck.st.reheader(packs[0], edit)]
    s2, hd2 = open_session(ctx, ck, bad, index)
    wf, _, _ = check_structure(ck, s2, hd2, index)
    assert [e for e, f in enumerate(wf) if f] == [63, 64, 255, 256, 299]
    s.close()
    s2.close()


def test_thousand_packfiles_of_one_entry(ctx, ck):
    """Every entry starts a segment; with 1,024 entries per scan workgroup all of them lie in one."""
    packs, index = ck.st.thousand_packfiles_of_one()
    s, hd = open_session(ctx, ck, packs, index)
    wf, wi, ws = check_structure(ck, s, hd, index)
    assert not any(wf) and not any(wi) and len(ws) == 1000
    auth, full = check_data(ck, s, packs, hd, select=[k % 7 == 0 for k in range(1000)])
    assert auth.count(ck.rr.OK) == 143 and full.count(ck.rr.OK) == 143
    s.close()


def test_segments_across_scan_workgroups(ctx, ck):
    """2,500 entries in packfiles of 700: segments start inside the second and third scan workgroup and
    one runs across the border between them, so the carry of k_check_carry is used and is cut."""
    rng = np.random.default_rng(56)
    b = ck.store.Builder(seed=56)
    for k in range(2500):
        b.add(ck.st.blob_bytes(rng, 3 + k % 5) + k.to_bytes(4, "little"))
    packs, index = b.finish(target=700)
    packs[2] = ck.st.reheader(packs[2], lambda ents: ents[:699] + [ents[699][:4] + [ents[699][4] + 3]])
    s, hd = open_session(ctx, ck, packs, index)
    wf, wi, ws = check_structure(ck, s, hd, index)
    assert [e for e, f in enumerate(wf) if f] == [2099] and len(ws) == 4
    s.close()


def test_store_without_items_and_session_without_entries(ctx, ck):
    packs, index = ck.st.base_store()
    s, hd = open_session(ctx, ck, packs, [])
    wf, wi, ws = check_structure(ck, s, hd, [])
    assert wf == [ck.cr.E_UNINDEXED] * 14 and wi == []
    s.close()
    with ck.restore.Session(ctx, ck.PRK, [], [], ck.pref.entries_array([]), ck.store.items_array(index)) as s0:
        flags, items, stats, counts = ck.check.structure(s0)
        assert flags.size == 0 and stats.size == 0 and items.tolist() == [ck.rr.ENOPACKFILE] * 14
        assert counts["n_items_nopackfile"] == 14 and counts["n_entries"] == 0 and counts["n_packfiles_clean"] == 0
        assert ck.check.data(s0, "auth").size == 0 and ck.check.data(s0, "full").size == 0
    with ck.restore.Session(ctx, ck.PRK, [], [], ck.pref.entries_array([]), ck.store.items_array([])) as s0:
        flags, items, stats, counts = ck.check.structure(s0)
        assert not flags.size and not items.size and not any(counts.values())


# ------------------------------------------------------------------ structure damage
@pytest.fixture(scope="module")
def cases(ck):
    return ck.st.structure_cases()


@pytest.mark.parametrize("name", ["clean", "length past the section", "length 15", "offsets swapped", "overlap by one byte",
                                  "truncated by one byte", "five trailing bytes", "dropped index item",
                                  "item with an unknown id", "item naming a packfile that lacks the hash", "item three times",
                                  "one hash twice in a packfile", "one hash twice, indexed twice", "all together"])
def test_structure_damage(ctx, ck, cases, name):
    packs, index, finding = cases[name]
    s, hd = open_session(ctx, ck, packs, index)
    wf, wi, ws = check_structure(ck, s, hd, index)
    ef, ei, et = ck.st.expected(hd, index, finding)
    assert (wf, wi, [st["tail"] for st in ws]) == (ef, ei, et)
    auth, full = check_data(ck, s, packs, hd)   # an entry out of range is ERANGE and never read; the invariant holds
    assert [e for e, a in enumerate(auth) if a == ck.rr.ERANGE] == [e for e, f in enumerate(wf) if f & ck.cr.E_RANGE]
    s.close()


# ------------------------------------------------------------------ data damage
@pytest.fixture(scope="module")
def damaged_data(ck):
    return ck.st.data_store()


def test_data_damage(ctx, ck, damaged_data):
    packs, index, exp, _ = damaged_data
    s, hd = open_session(ctx, ck, packs, index)
    hashes = [e[1] for e in ck.pref.flat_entries(hd)]
    auth, full = check_data(ck, s, packs, hd)
    assert auth == [exp.get(h, (0, 0))[0] for h in hashes] and full == [exp.get(h, (0, 0))[1] for h in hashes]
    check_structure(ck, s, hd, index)
    s.close()


def test_sub_batches_of_four_slots_and_select_with_holes(ctx, ck, damaged_data):
    """slots = 4 with 11 selected entries: FULL goes 4 + 4 + 3; the failures lie on both sides of both borders."""
    packs, index, exp, _ = damaged_data
    s, hd = open_session(ctx, ck, packs, index, slots=4)
    hashes = [e[1] for e in ck.pref.flat_entries(hd)]
    sel = [False] * len(hashes)
    for e in (2, 4, 5, 6, 7, 8, 9, 11, 13, 17, 21):   # 4 ETAG (4, 5, 6, 7), EZSTD 8, EDIGEST 9, EFORMAT 11
        sel[e] = True
    assert sum(sel) == 11 and [hashes[e] in exp for e in (3, 4, 7, 8)] == [False, True, True, True]
    auth, full = check_data(ck, s, packs, hd, select=sel)
    chosen = [f for f, c in zip(full, sel) if c]
    assert [bool(f) for f in chosen] == [False, True, True, True, True, True, True, True, False, False, False]
    assert full.count(ck.cr.SKIPPED) == len(hashes) - 11
    auth_all, full_all = check_data(ck, s, packs, hd)
    assert full_all == [exp.get(h, (0, 0))[1] for h in hashes]
    s.close()


# ------------------------------------------------------------------ the whole check
def _entries(ck, packs):
    return ck.pref.entries_array(ck.pref.headers_of(ck.PRK, packs))


def test_check_clean_store_with_each_read_data(ctx, ck, snapshots):
    packs, index, root_a, root_b = snapshots
    files, ids, items = [b for _, b in packs], [i for i, _ in packs], ck.store.items_array(index)
    en = _entries(ck, packs)
    for read_data in (None, "auth", "full"):
        rep = ck.check.check(ctx, files, ids, en, items, ck.PRK, roots=[root_a, root_b], read_data=read_data)
        assert rep["ok"] and rep["bad_packfiles"] == [] and not len(rep["mark_errors"]) and rep["unreachable_blobs"] == 0
        assert (rep["data_status"] is None) == (read_data is None)
    rep = ck.check.check(ctx, files, ids, en, items, ck.PRK, roots=[root_a])
    assert rep["ok"] and rep["unreachable_blobs"] > 0 and rep["unreachable_bytes"] > 0 and not rep["live"].all()
    assert ck.check.check(ctx, files, ids, en, items, ck.PRK, read_data=None)["ok"]


def test_check_after_prune(ctx, ck, snapshots):
    packs, index, root_a, _ = snapshots
    files, ids, items = [b for _, b in packs], [i for i, _ in packs], ck.store.items_array(index)
    p2, i2, it2, _ = ck.prune.prune(ctx, files, ids, _entries(ck, packs), items, ck.PRK, [root_a],
                                    [bytes([0x70 + g]) * 12 for g in range(4)])
    packs2 = list(zip(i2, p2))
    rep = ck.check.check(ctx, p2, i2, _entries(ck, packs2), it2, ck.PRK, roots=[root_a], read_data="full")
    assert rep["ok"] and rep["unreachable_blobs"] == 0
    hd2 = ck.pref.headers_of(ck.PRK, packs2)
    wf, wi, ws, wc = ck.cr.structure(hd2, [(bytes(r[:32]), bytes(r[32:])) for r in it2])
    assert rep["entry_flags"].tolist() == wf and rep["item_status"].tolist() == wi and rep["counts"] == wc


def test_check_packfiles_selected_and_bad_packfiles(ctx, ck, damaged_data):
    packs, index, exp, _ = damaged_data
    files, ids, items = [b for _, b in packs], [i for i, _ in packs], ck.store.items_array(index)
    hd = ck.pref.headers_of(ck.PRK, packs)
    en = ck.pref.entries_array(hd)
    flags, _, stats, _ = ck.cr.structure(hd, index)
    for read_data in ("auth", "full"):
        rep = ck.check.check(ctx, files, ids, en, items, ck.PRK, read_data=read_data)
        want = ck.cr.data(ck.PRK, packs, hd, read_data)
        assert not rep["ok"] and rep["data_status"].tolist() == want
        assert rep["bad_packfiles"] == ck.cr.bad_packfiles(hd, flags, stats, want)
    # "a peer just returned packfiles 1 and 3": only their entries are read
    sel = [int(e["packfile"]) in (1, 3) for e in en]
    rep = ck.check.check(ctx, files, ids, en, items, ck.PRK, read_data="full", packfiles_selected=[1, 3])
    want = ck.cr.data(ck.PRK, packs, hd, "full", sel)
    assert rep["data_status"].tolist() == want and rep["bad_packfiles"] == ck.cr.bad_packfiles(hd, flags, stats, want)
    assert set(rep["bad_packfiles"]) <= {1, 3} and rep["bad_packfiles"]


def test_check_damaged_graph_with_roots(ctx, ck):
    """The damaged-graph store of the prune tests: the mark's errors are in the report, and the packfiles to
    fetch again are check_ref's."""
    rng = np.random.default_rng(36)
    bb = ck.st.blob_bytes
    b = ck.store.Builder(seed=36)
    good = [b.add_file("good%d" % k, bb(rng, 600 + k)) for k in range(10)]
    chunk = b.add(b"a chunk a Dir names")
    absent_tree, absent_chunk = b"\x01" * 32, b"\x02" * 32
    nopack_chunk, mismatch_chunk = b.add(b"indexed under an absent id"), b.add(b"indexed under the wrong packfile")
    f_missing = b.add_tree(0, "fm", None, None, None, [absent_chunk, chunk, nopack_chunk, mismatch_chunk])
    flipped = b.add_tree(1, "flipped", None, None, None, [good[0]])
    malformed = b.add_raw_tree(b"\x02not a tree")
    top = b.add_tree(1, "", None, None, None, [good[2], absent_tree, good[3], chunk, good[4], flipped, good[5], malformed,
                                               good[6], f_missing, good[8]])
    cut = b.add(bb(rng, 500))
    f_cut = b.add_tree(0, "fc", None, None, None, [cut, chunk])
    b.blobs[-2], b.blobs[-1] = b.blobs[-1], b.blobs[-2]
    packs, index = b.finish(target=9)
    hd = ck.pref.headers_of(ck.PRK, packs)
    ck.st._flip(packs, hd, flipped, "tag")
    packs[-1] = (packs[-1][0], packs[-1][1][:-5])
    other = next(pid for pid, _ in packs if pid != dict(index)[mismatch_chunk])
    index = [(h, b"\xee" * 12 if h == nopack_chunk else other if h == mismatch_chunk else pid) for h, pid in index]
    roots = [top, f_cut]
    hd = ck.pref.headers_of(ck.PRK, packs)
    files, ids, items = [x for _, x in packs], [i for i, _ in packs], ck.store.items_array(index)
    for read_data in ("auth", "full"):
        rep = ck.check.check(ctx, files, ids, ck.pref.entries_array(hd), items, ck.PRK, roots=roots, read_data=read_data, slots=3)
        verify = read_data == "full"
        _, werrs, _ = ck.pref.mark(ck.rr.Store(ck.PRK, packs, index, verify=verify), hd, roots)
        got = sorted((e["hash"].tobytes(), e["parent"].tobytes(), int(e["child_pos"]), int(e["reason"])) for e in rep["mark_errors"])
        assert got == sorted(werrs.elements()) and len(got) >= 7 and not rep["ok"]
        flags, wi, stats, _ = ck.cr.structure(hd, index)
        want = ck.cr.data(ck.PRK, packs, hd, read_data)
        assert rep["entry_flags"].tolist() == flags and rep["item_status"].tolist() == wi and rep["data_status"].tolist() == want
        assert rep["bad_packfiles"] == ck.cr.bad_packfiles(hd, flags, stats, want, [k[0] for k in werrs])
