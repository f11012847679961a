"""bw_parent_match (backuwup_amd.parent.match) against tests/parent_ref.py over the stores of
tests/parent_stores.py.  Per case five things are compared, and all must be equal: the status and hash of
every scan node, the multiset of errors, the set of entries read, the number of levels, and n_unchanged
with unchanged_bytes.  Small stores; every session is opened in a with statement; a store and its
reference result are built once per process and shared."""
import ctypes
import functools
import os
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]

NEW, UNCHANGED, CHANGED, RACY, DIR, TYPE_CHANGED = range(6)
NONE = 2**64 - 1
ZERO = bytes(32)


@pytest.fixture(scope="module")
def pm(oracle):
    import parent_ref
    import parent_stores
    import prune_ref
    import restore_ref
    import restore_store
    from backuwup_amd import _lib, parent, restore

    class NS:
        pass
    ns = NS()
    ns.ref, ns.stores, ns.pref, ns.rr, ns.PRK, ns.rs = parent_ref, parent_stores, prune_ref, restore_ref, restore_store.PRK, restore_store
    ns.parent, ns.restore, ns.L = parent, restore, _lib
    return ns


@functools.lru_cache(maxsize=None)
def built(name, arg=None):
    """(case, Store, headers) of a builder, once per process."""
    import parent_stores
    import prune_ref
    import restore_ref
    import restore_store
    fn = getattr(parent_stores, name)
    c = fn() if arg is None else fn(arg)
    return c, restore_ref.Store(restore_store.PRK, c["packs"], c["index"]), prune_ref.headers_of(restore_store.PRK, c["packs"])


@functools.lru_cache(maxsize=None)
def wanted(name, arg=None, root="case", trust=None):
    import parent_ref
    c, store, hd = built(name, arg)
    return parent_ref.match(store, hd, c["root"] if root == "case" else root, c["scan"], c["trust"] if trust is None else trust)


def arrays(pm, scan):
    """A parent_ref scan as (NODE_DTYPE, names)."""
    nodes = np.zeros(len(scan), dtype=pm.restore.NODE_DTYPE)
    names = bytearray()
    for i, n in enumerate(scan):
        nodes[i] = (n["kind"], n["flags"], n["size"], n["mtime"], n["ctime"], NONE, n["child_first"], n["n_children"],
                    len(names), len(n["name"]))
        names += n["name"]
    return nodes, bytes(names)


def session(ctx, pm, c, slots=16):
    files, ids = [b for _, b in c["packs"]], [i for i, _ in c["packs"]]
    return pm.restore.Session(ctx, pm.PRK, files, ids, ctx.unpack_headers(pm.PRK, files, ids), pm.rs.items_array(c["index"]),
                              slots=slots)


def compare(got, want):
    results, read, counts, errors = got
    want_res, want_errors, want_read, want_levels, want_unch, want_bytes = want
    got_res = [(int(r["status"]), bytes(r["hash"])) for r in results]
    assert got_res == want_res, [(i, g, w) for i, (g, w) in enumerate(zip(got_res, want_res)) if g != w][:3]
    got_errors = Counter((bytes(e["hash"]), bytes(e["parent"]), int(e["child_pos"]), int(e["reason"])) for e in errors)
    assert got_errors == want_errors, (sorted(got_errors - want_errors, key=str)[:3], sorted(want_errors - got_errors, key=str)[:3])
    assert set(np.flatnonzero(read).tolist()) == set(want_read) and set(np.unique(read).tolist()) <= {0, 1}
    assert counts["n_levels"] == want_levels and counts["n_read"] == len(want_read) and counts["n_errors"] == len(errors)
    assert (counts["n_unchanged"], counts["unchanged_bytes"]) == (want_unch, want_bytes)


def walk(ctx, pm, name, arg=None, slots=16, verify=False, root="case", trust=None):
    c = built(name, arg)[0]
    with session(ctx, pm, c, slots) as s:
        got = pm.parent.match(s, c["root"] if root == "case" else root, *arrays(pm, c["scan"]),
                              trust_before=c["trust"] if trust is None else trust, verify=verify)
    compare(got, wanted(name, arg, root, trust))
    return c, got


def status(pm, c, got, path):
    return int(got[0][pm.stores.where(c["scan"], path)]["status"])


# ------------------------------------------------------------------ 1, 18
@pytest.mark.parametrize("slots,verify", [(16, False), (0, False), (4, True)])      # 0: the default, 1,024 slots
def test_identity(ctx, pm, slots, verify):
    c, (results, read, counts, errors) = walk(ctx, pm, "identity", slots=slots, verify=verify)
    for sn, r in zip(c["scan"], results):
        assert r["status"] == (DIR if sn["kind"] == 1 else UNCHANGED)
    ents = pm.pref.flat_entries(built("identity")[2])
    # exactly the Tree first pieces (no Dir here has a later one), and no chunk
    assert set(np.flatnonzero(read).tolist()) == {e for e, ent in enumerate(ents) if ent[2] == 1}
    assert counts["n_unchanged"] == 11 and counts["unchanged_bytes"] == 3370 and len(errors) == 0


# ------------------------------------------------------------------ 2
def test_one_field_off(ctx, pm):
    c, got = walk(ctx, pm, "fields")
    assert {k: status(pm, c, got, k) for k in c["want"]} == c["want"]


# ------------------------------------------------------------------ 3
def test_names_compare_whole(ctx, pm):
    c, got = walk(ctx, pm, "names")
    assert got[2]["n_unchanged"] == c["n_same"] and status(pm, c, got, "names/last2") == NEW


# ------------------------------------------------------------------ 4
def test_trust_before(ctx, pm):
    T = pm.stores.TRUST
    c, got = walk(ctx, pm, "trust", T)
    assert [status(pm, c, got, p) for p in ("before", "at", "after", "changed")] == [UNCHANGED, RACY, RACY, CHANGED]
    c, got = walk(ctx, pm, "trust", T, trust=NONE)
    assert [status(pm, c, got, p) for p in ("before", "at", "after", "changed")] == [UNCHANGED] * 3 + [CHANGED]


# ------------------------------------------------------------------ 5
def test_content_replaced_is_unchanged_that_is_the_heuristic(ctx, pm):
    """The parent holds other bytes under an equal name, size, mtime and ctime.  A stat-only scan cannot
    see that: the node is UNCHANGED and carries the parent's hash.  This is the heuristic every
    parent-snapshot backup rests on, not a defect; trust_before is what narrows it."""
    c, got = walk(ctx, pm, "content_replaced")
    i = pm.stores.where(c["scan"], "d/f")
    assert got[0][i]["status"] == UNCHANGED
    assert pm.rr.restore_file(built("content_replaced")[1], pm.rr.fetch_tree(built("content_replaced")[1], bytes(got[0][i]["hash"])))[0] == b"old!"


# ------------------------------------------------------------------ 6, 7
def test_duplicate_names(ctx, pm):
    c, got = walk(ctx, pm, "duplicates")
    d = c["scan"][pm.stores.where(c["scan"], "d")]
    assert [int(got[0][k]["status"]) for k in range(d["child_first"], d["child_first"] + 4)] == [1, 1, 1, 2]


def test_the_item_is_part_of_the_key(ctx, pm):
    c, got = walk(ctx, pm, "same_name_in_many_dirs", slots=0)
    assert got[2]["n_unchanged"] == 300 - 43 and got[2]["n_levels"] == 2


# ------------------------------------------------------------------ 8, 9
@pytest.mark.parametrize("slots", [0, 16])
def test_children_counts_at_the_wave_and_block_boundaries(ctx, pm, slots):
    c, got = walk(ctx, pm, "children_counts", slots=slots)
    want = sum(1 for n in pm.stores.COUNTS for k in range(n) if k % 5 != 4)
    assert got[2]["n_unchanged"] == want


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_a_level_of_n_items(ctx, pm, n):
    c, got = walk(ctx, pm, "level_of", n, slots=0)
    assert got[2]["n_unchanged"] == n and got[2]["n_levels"] == 2


# ------------------------------------------------------------------ 10, 11
def test_planted_dir_chain(ctx, pm):
    c, got = walk(ctx, pm, "dir_chains", slots=4)
    assert [status(pm, c, got, "split/k%d" % k) for k in (0, 1, 2, 3, 4, 5, 9)] == [1, 1, 1, 1, 2, 1, 0]


def test_a_dir_of_10001_children_matches_on_both_sides_of_the_piece_boundary(ctx, pm):
    c, got = walk(ctx, pm, "big_dir", slots=0)
    assert [status(pm, c, got, "big/e%05d" % k) for k in c["picks"]] == [UNCHANGED] * 5 + [UNCHANGED]
    assert got[2]["n_unchanged"] == 6 and got[2]["n_read"] == 10001 + 2 + 1   # the files, big's two pieces, the root


def test_a_files_later_pieces_are_never_opened_and_a_chain_that_names_itself_ends(ctx, pm):
    c, got = walk(ctx, pm, "file_chain_and_loop", slots=4)
    ents = pm.pref.flat_entries(built("file_chain_and_loop")[2])
    assert status(pm, c, got, "f3") == UNCHANGED
    assert not [e for e in np.flatnonzero(got[1]).tolist() if ents[e][1] in c["later"]]
    assert [(bytes(e["hash"]), int(e["reason"])) for e in got[3]] == [(c["loop"], pm.L.BW_RESTORE_EFORMAT)]


# ------------------------------------------------------------------ 12, 13
def test_structure(ctx, pm):
    c, got = walk(ctx, pm, "structure")
    assert status(pm, c, got, "was_file") == TYPE_CHANGED and status(pm, c, got, "was_dir") == TYPE_CHANGED
    assert status(pm, c, got, "was_file/sub/x") == NEW and status(pm, c, got, "added/deep/g") == NEW
    store, ents = built("structure")[1], pm.pref.flat_entries(built("structure")[2])
    names = {pm.rr.fetch_tree(store, ents[e][1]).name for e in np.flatnonzero(got[1]).tolist()}
    assert names == {"", "kept", "removed", "was_file", "was_dir", "f"}   # nothing below removed, added or was_dir


def test_no_parent_root_a_file_root_unreadable(ctx, pm):
    c, (results, read, counts, errors) = walk(ctx, pm, "structure", root=None)
    assert not results["status"].any() and not results["hash"].any() and not read.any() and counts["n_levels"] == 0
    c, got = walk(ctx, pm, "root_is_file")
    assert [int(s) for s in got[0]["status"]] == [TYPE_CHANGED, NEW] and got[2]["n_levels"] == 1
    c, got = walk(ctx, pm, "root_unreadable")
    assert not got[0]["status"].any() and got[2]["n_errors"] == 1 and got[2]["n_levels"] == 1 and not got[1].any()


# ------------------------------------------------------------------ 14, 15, 18
@pytest.mark.parametrize("kind", ["absent", "no_packfile", "not_in_header", "bad_tag", "bad_zstd", "garbage", "chunk"])
def test_damage_to_a_childs_first_piece(ctx, pm, kind):
    c, got = walk(ctx, pm, "damaged", slots=4, verify=kind in ("bad_tag", "garbage"))
    k = pm.stores.DAMAGE.index(kind)
    recs = [e for e in got[3] if bytes(e["hash"]) == c["bad"][kind]]
    assert len(recs) == 1 and bytes(recs[0]["parent"]) == c["root"] and recs[0]["child_pos"] == 2 * k + 1
    assert recs[0]["reason"] == c["reasons"][kind]
    i = pm.stores.where(c["scan"], kind)
    assert got[0][i]["status"] == NEW and bytes(got[0][i]["hash"]) == ZERO and got[2]["n_unchanged"] == 8


def test_a_dir_chain_whose_second_piece_is_unreadable_ends_there(ctx, pm):
    c, got = walk(ctx, pm, "broken_dir_chain")
    assert [status(pm, c, got, "d/k%d" % k) for k in range(5)] == [1, 1, 0, 0, 0]
    assert [(bytes(e["hash"]), bytes(e["parent"]), int(e["child_pos"])) for e in got[3]] == [(c["lost"], c["first"], NONE)]


# ------------------------------------------------------------------ 16, 17
CANARY = 0xA5


def raw(pm, s, root, scan, err_cap, trust=NONE):
    """bw_parent_match with exactly this err_cap and a canary behind each array."""
    from backuwup_amd.prune import ERROR_DTYPE
    nodes, names = arrays(pm, scan)
    nm = np.frombuffer(names, dtype=np.uint8)
    res = np.full((len(nodes) + 1) * pm.parent.RESULT_DTYPE.itemsize, CANARY, dtype=np.uint8)
    errs = np.full((err_cap + 1) * ERROR_DTYPE.itemsize, CANARY, dtype=np.uint8)
    read = np.full(s.n_entries + 64, CANARY, dtype=np.uint8)
    cnt = pm.L.BwParentCounts()
    r = None if root is None else (ctypes.c_uint8 * 32).from_buffer_copy(bytes(root))
    rc = s._L.bw_parent_match(s.h, r, trust, 0, nodes.ctypes.data_as(ctypes.POINTER(pm.L.BwRestoreNode)), len(nodes),
                              ctypes.c_void_p(nm.ctypes.data), nm.size, res.ctypes.data_as(ctypes.POINTER(pm.L.BwParentResult)),
                              read.ctypes.data_as(pm.L.u8p), ctypes.byref(cnt),
                              errs.ctypes.data_as(ctypes.POINTER(pm.L.BwPruneError)), err_cap)
    assert (res[len(nodes) * pm.parent.RESULT_DTYPE.itemsize:] == CANARY).all() and (read[s.n_entries:] == CANARY).all()
    assert (errs[err_cap * ERROR_DTYPE.itemsize:] == CANARY).all()
    counts = {f: int(getattr(cnt, f)) for f in pm.parent.COUNT_FIELDS}
    return (rc, res[:len(nodes) * pm.parent.RESULT_DTYPE.itemsize].view(pm.parent.RESULT_DTYPE), read[:s.n_entries], counts,
            errs[:err_cap * ERROR_DTYPE.itemsize].view(ERROR_DTYPE))


def test_err_cap_one_short_is_enospc_with_everything_else_filled(ctx, pm):
    c = built("damaged")[0]
    want = wanted("damaged")
    with session(ctx, pm, c, 4) as s:
        rc, results, read, counts, errs = raw(pm, s, c["root"], c["scan"], 6)
        assert rc == pm.L.BW_ENOSPC and counts["n_errors"] == 7
        got_errors = Counter((bytes(e["hash"]), bytes(e["parent"]), int(e["child_pos"]), int(e["reason"])) for e in errs)
        assert len(errs) == 6 and not got_errors - want[1]
        compare((results, read, dict(counts, n_errors=0), errs[:0]), want[:1] + (Counter(),) + want[2:])
        rc, results, read, counts, errs = raw(pm, s, c["root"], c["scan"], 7)
        assert rc == pm.L.BW_OK
        compare((results, read, counts, errs), want)


def test_an_invalid_scan_is_einval_and_nothing_is_read(ctx, pm):
    ok, bad = pm.stores.invalid_scans()
    c = built("identity")[0]
    with session(ctx, pm, c) as s:
        for what, scan in bad.items():
            rc, results, read, counts, errs = raw(pm, s, c["root"], scan, 4)
            assert rc == pm.L.BW_EINVAL and not read.any() and counts["n_read"] == 0, what
        nodes, names = arrays(pm, ok)
        nodes[3]["name_off"] = len(names)                 # a name that runs past the arena
        with pytest.raises(pm.L.BwError) as e:
            pm.parent.match(s, c["root"], nodes, names)
        assert e.value.rc == pm.L.BW_EINVAL
        rc, results, read, counts, errs = raw(pm, s, c["root"], ok, 4)
        assert rc == pm.L.BW_OK and counts["n_levels"] == 1   # the scan's Dirs are not the parent's: all NEW below the root
