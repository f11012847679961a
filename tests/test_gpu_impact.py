"""bw_impact_mark and bw_impact_paths (backuwup_amd.impact) against tests/impact_ref.py over the stores of
tests/impact_stores.py.  Every case goes through both entry points on a fresh session; compared are the
taint and root_affected bytes, the records as a multiset per level with parents resolved to paths,
per_root, the errors of both calls as multisets, and n_trees_expanded, n_edges and n_levels.  Small
stores; a store and its reference results are built once (impact_stores.reference) and shared."""
import ctypes
import os
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402
from impact_stores import reference as ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]

NONE = 2**64 - 1
CANARY = 0xA5


def store_args(ctx, case):
    import restore_store
    files, ids = [b for _, b in case["packs"]], [i for i, _ in case["packs"]]
    return files, ids, ctx.unpack_headers(restore_store.PRK, files, ids), restore_store.items_array(case["index"])


def session(ctx, case):
    import restore_store
    from backuwup_amd import restore
    return restore.Session(ctx, restore_store.PRK, *store_args(ctx, case), slots=case["slots"])


def bad_of(case):
    bad = np.zeros(case["n_entries"], dtype=np.uint8)
    bad[list(case["bad"])] = 1
    return bad


def as_errors(errors):
    return Counter((bytes(e["hash"]), bytes(e["parent"]), int(e["child_pos"]), int(e["reason"])) for e in errors)


def as_ref_records(records, names):
    """The library's records as impact_ref.resolve gives the reference's: level and path through parent."""
    import impact_ref
    out, level, path = [], [], []
    for i, r in enumerate(records):
        parent = int(r["parent"])
        assert parent == NONE or parent < i
        h = bytes(r["hash"])
        name = bytes(names[int(r["name_off"]):int(r["name_off"]) + int(r["name_len"])])
        own = b"?" + h if int(r["flags"]) & impact_ref.UNREADABLE else name
        level.append(0 if parent == NONE else level[parent] + 1)
        path.append((() if parent == NONE else path[parent]) + (own,))
        assert parent == NONE or int(records[parent]["root"]) == int(r["root"])
        out.append(dict(level=level[i], root=int(r["root"]), path=path[i], hash=h, name=name, kind=int(r["kind"]),
                        meta_flags=int(r["meta_flags"]), size=int(r["size"]), mtime=int(r["mtime"]), ctime=int(r["ctime"]),
                        n_children=int(r["n_children"]), n_affected=int(r["n_affected"]),
                        first_affected=int(r["first_affected"]), flags=int(r["flags"])))
    return impact_ref.resolve(out)


def run(ctx, name, arg=None):
    """Both entry points over a fresh session, each output against the reference.  -> (mark counts, records)."""
    import impact_ref
    from backuwup_amd import impact
    case, taint, affected, errors, info, records, per_root, perrors = ref(name, arg)
    with session(ctx, case) as s:
        t, ra, counts, errs = impact.mark(s, case["roots"], bad_of(case), verify=case["verify"])
        recs, names, pr, pcounts, perrs = impact.paths(s, case["roots"], t, verify=case["verify"])
    assert t.tolist() == taint and ra.tolist() == affected and set(np.unique(t).tolist()) <= {0, 1, 2, 3}
    assert as_errors(errs) == errors and counts["n_errors"] == sum(errors.values())
    for f in ("n_trees_expanded", "n_edges", "n_levels", "n_tainted", "n_roots_affected"):
        assert counts[f] == info[f], f
    assert counts["n_sweeps"] >= 1
    got, want = as_ref_records(recs, names), impact_ref.resolve(records)
    assert got == want, (sorted(got - want, key=str)[:3], sorted(want - got, key=str)[:3])
    assert [{f: int(x[f]) for f in impact.ROOT_DTYPE.names} for x in pr] == per_root
    assert as_errors(perrs) == perrors and pcounts["n_errors"] == sum(perrors.values())
    assert pcounts["n_records"] == len(records) and pcounts["n_levels"] == 1 + max([r["level"] for r in records], default=-1)
    return counts, recs


def test_clean(ctx, oracle):
    counts, recs = run(ctx, "clean")
    assert counts["n_sweeps"] >= 1 and counts["n_tainted"] == 0 and len(recs) == 0


def test_shared_chunk_expands_each_tree_blob_once_as_prune_does(ctx, oracle):
    from backuwup_amd import prune
    counts, _ = run(ctx, "shared_chunk")
    case = ref("shared_chunk")[0]
    with session(ctx, case) as s:
        assert prune.mark(s, case["roots"])[2]["n_trees_expanded"] == counts["n_trees_expanded"] == 8


@pytest.mark.parametrize("name", ["lost_directory", "lost_later_piece", "wide", "four_slots", "real_damage",
                                  "dir_contains_itself", "chain_names_itself"])
def test_cases(ctx, oracle, name):
    run(ctx, name)


def test_late_parent_needs_more_than_one_sweep(ctx, oracle):
    counts, _ = run(ctx, "late_parent")
    if ref("late_parent")[4]["n_sweeps"] >= 2:  # the reference's own count in that order (it is 3)
        assert counts["n_sweeps"] >= 2


@pytest.mark.parametrize("which", [0, 1])
def test_duplicate_hashes(ctx, oracle, which):
    run(ctx, "duplicate_hashes", which)


@pytest.mark.parametrize("p", range(6))
def test_whole_packfile(ctx, oracle, p):
    from backuwup_amd import impact
    case = ref("whole_packfile", p)[0]
    assert impact.lost_packfiles(store_args(ctx, case)[2], [p]).tolist() == bad_of(case).tolist()
    run(ctx, "whole_packfile", p)


@pytest.mark.parametrize("which", ["none", "file_root", "unlocatable", "twice", "hundred"])
def test_edges(ctx, oracle, which):
    run(ctx, "edges", which)


# ------------------------------------------------------------------ capacity
def raw_paths(s, roots, taint, record_cap, names_cap, err_cap):
    """bw_impact_paths with exactly these caps and a canary behind each array: (rc, records, names, counts)."""
    L = sys.modules["backuwup_amd._lib"]
    from backuwup_amd import impact
    from backuwup_amd.prune import ERROR_DTYPE
    r = np.frombuffer(b"".join(roots), dtype=np.uint8)
    size = impact.RECORD_DTYPE.itemsize
    records = np.full((record_cap + 1) * size, CANARY, dtype=np.uint8)
    names = np.full(names_cap + 64, CANARY, dtype=np.uint8)
    errs = np.full((err_cap + 1) * ERROR_DTYPE.itemsize, CANARY, dtype=np.uint8)
    per_root = np.full((len(roots) + 1) * 32, CANARY, dtype=np.uint8)
    cnt = L.BwImpactPathsCounts()
    t = np.ascontiguousarray(taint, dtype=np.uint8)
    rc = s._L.bw_impact_paths(s.h, r.ctypes.data_as(ctypes.c_void_p), len(roots), t.ctypes.data_as(L.u8p), 0,
                              records.ctypes.data_as(ctypes.POINTER(L.BwImpactRecord)), record_cap,
                              names.ctypes.data_as(ctypes.c_void_p), names_cap,
                              per_root.ctypes.data_as(ctypes.POINTER(L.BwImpactRoot)), ctypes.byref(cnt),
                              errs.ctypes.data_as(ctypes.POINTER(L.BwPruneError)), err_cap)
    assert (records[record_cap * size:] == CANARY).all() and (names[names_cap:] == CANARY).all()
    assert (errs[err_cap * ERROR_DTYPE.itemsize:] == CANARY).all() and (per_root[len(roots) * 32:] == CANARY).all()
    counts = {f: int(getattr(cnt, f)) for f in impact.PATHS_FIELDS}
    return rc, records[:record_cap * size].view(impact.RECORD_DTYPE), names[:names_cap].tobytes(), counts


def test_caps_one_short_at_the_first_a_middle_and_the_last_level(ctx, oracle):
    # late_parent: the levels hold 1, 2, 2, 1, 1, 1, 1, 1 records and 1, 3, 3, 2, 2, 2, 1, 1 name bytes
    import impact_ref
    L = sys.modules["backuwup_amd._lib"]
    case, taint, _, _, _, records, _, _ = ref("late_parent")
    want = impact_ref.resolve(records)
    with session(ctx, case) as s:
        rc, recs, names, counts = raw_paths(s, case["roots"], taint, 10, 15, 4)
        assert rc == L.BW_OK and counts["n_records"] == 10 and counts["name_bytes"] == 15 and counts["n_levels"] == 8
        assert as_ref_records(recs, names) == want
        for record_cap, names_cap, n_records, name_bytes, n_levels, fit in (
                (0, 15, 1, 1, 1, 0), (4, 15, 5, 7, 3, 3), (9, 15, 10, 15, 8, 9),
                (10, 0, 1, 1, 1, 0), (10, 6, 5, 7, 3, 3), (10, 14, 10, 15, 8, 9)):
            rc, recs, names, counts = raw_paths(s, case["roots"], taint, record_cap, names_cap, 4)
            assert rc == L.BW_ENOSPC
            assert (counts["n_records"], counts["name_bytes"], counts["n_levels"]) == (n_records, name_bytes, n_levels)
            got = as_ref_records(recs[:fit], names)  # the levels before are intact
            assert not got - want and sum(got.values()) == fit


def test_more_errors_than_err_cap_is_enospc_with_everything_else_filled(ctx, oracle):
    L = sys.modules["backuwup_amd._lib"]
    from backuwup_amd import impact
    case, taint, affected, errors, info, records, _, perrors = ref("edges", "unlocatable")
    assert sum(errors.values()) == sum(perrors.values()) == 1
    with session(ctx, case) as s:
        t, ra, counts, errs = impact.mark(s, case["roots"], bad_of(case), err_cap=0)
        assert counts["n_errors"] == 1 and len(errs) == 0 and t.tolist() == taint and ra.tolist() == affected
        rc, recs, names, pcounts = raw_paths(s, case["roots"], taint, 8, 64, 0)
        assert rc == L.BW_ENOSPC and pcounts["n_errors"] == 1 and pcounts["n_records"] == len(records) == 3
        import impact_ref
        assert as_ref_records(recs[:3], names) == impact_ref.resolve(records)


def test_a_taint_byte_with_another_bit_is_refused(ctx, oracle):
    L = sys.modules["backuwup_amd._lib"]
    case, taint = ref("clean")[:2]
    with session(ctx, case) as s:
        rc, _, _, _ = raw_paths(s, case["roots"], [0, 4] + taint[2:], 8, 64, 4)
    assert rc == L.BW_EINVAL
