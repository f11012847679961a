"""bw_retain_mark and bw_retain_drop (backuwup_amd.retain) against tests/retain_ref.py over the stores of
tests/retain_stores.py, each case on a fresh session.  The mark: masks, damaged, per_root, n_trees_expanded,
n_levels, n_edges and the totals equal the reference, the errors are the reference's multiset, and both
the errors and n_trees_expanded are bw_prune_mark's over all roots on the same session.  The drop, which
is the point: for forgetting nothing, each single root (seven at most), all roots and four seeded random
subsets, live and stats are bw_prune_mark's over the kept roots byte for byte, and freed is the
reference's.  Small stores; a store and its reference results are built once (retain_stores.reference)."""
import ctypes
import os
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402
from retain_stores import CASES, drop_sets, reference as ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]


def store_args(ctx, case):
    import restore_store
    files, ids = [b for _, b in case["packs"]], [i for i, _ in case["packs"]]
    return files, ids, ctx.unpack_headers(restore_store.PRK, files, ids), restore_store.items_array(case["index"])


def session(ctx, case):
    import restore_store
    from backuwup_amd import restore
    return restore.Session(ctx, restore_store.PRK, *store_args(ctx, case), slots=case["slots"])


def as_errors(errors):
    return Counter((bytes(e["hash"]), bytes(e["parent"]), int(e["child_pos"]), int(e["reason"])) for e in errors)


def as_ints(masks):
    """(n_entries, W) u64 -> one Python int per entry."""
    return [sum(int(x) << (64 * w) for w, x in enumerate(row)) for row in masks.tolist()]


@pytest.mark.parametrize("name,arg", CASES, ids=["%s%s" % (n, "" if a is None else "-%d" % a) for n, a in CASES])
def test_case(ctx, oracle, name, arg):
    import retain_ref
    from backuwup_amd import prune, retain
    case, hd, masks, damaged, per_root, errors, info = ref(name, arg)
    roots, n = case["roots"], len(case["roots"])
    sets = drop_sets(n)
    with session(ctx, case) as s:
        m, dmg, pr, counts, errs = retain.mark(s, roots, verify=case["verify"])
        live, stats, freed = retain.drop(s, m, n, sets)
        _, _, pcounts, perrs = prune.mark(s, roots, verify=case["verify"])
        kept_marks = [prune.mark(s, [r for k, r in enumerate(roots) if k not in d], verify=case["verify"]) for d in sets]
    # the mark
    assert m.shape == (case["n_entries"], retain.words(n)) and as_ints(m) == masks
    assert dmg.tolist() == damaged
    assert [{f: int(x[f]) for f in retain.ROOT_DTYPE.names} for x in pr] == per_root
    for f in ("n_trees_expanded", "n_levels", "n_edges", "reached_blobs", "reached_bytes", "orphan_blobs", "orphan_bytes"):
        assert counts[f] == info[f], f
    print(name, arg, "sweeps", counts["n_sweeps"], "reference", info["n_sweeps"])
    assert counts["n_sweeps"] >= 1
    if info["n_sweeps"] >= 2:  # the reference's own count in forward order
        assert counts["n_sweeps"] >= 2
    assert as_errors(errs) == errors and counts["n_errors"] == sum(errors.values())
    assert as_errors(errs) == as_errors(perrs) and counts["n_trees_expanded"] == pcounts["n_trees_expanded"]
    # the drop
    assert live.shape == (len(sets), case["n_entries"]) and stats.shape == (len(sets), len(case["packs"]))
    for q, d in enumerate(sets):
        plive, pstats, _, _ = kept_marks[q]
        assert live[q].tobytes() == plive.tobytes(), (q, d)
        assert stats[q].tobytes() == pstats.tobytes(), (q, d)
        assert {f: int(freed[q][f]) for f in retain.FREED_DTYPE.names} == retain_ref.drop(hd, masks, d)[2], (q, d)


def test_late_parent_takes_a_second_productive_sweep(ctx, oracle):
    from backuwup_amd import retain
    case, _, masks, _, _, _, info = ref("late_parent")
    assert info["n_sweeps"] == 3
    with session(ctx, case) as s:
        m, _, _, counts, _ = retain.mark(s, case["roots"])
    assert counts["n_sweeps"] >= 2 and as_ints(m) == masks


def test_err_cap_one_short_is_enospc_with_everything_else_filled(ctx, oracle):
    from backuwup_amd import _lib, retain
    from backuwup_amd.prune import ERROR_DTYPE
    case, _, masks, damaged, per_root, errors, info = ref("real_damage")
    n_err = sum(errors.values())
    assert n_err == 2
    with session(ctx, case) as s:
        m, dmg, pr, counts, errs = retain.mark(s, case["roots"], verify=True, err_cap=n_err - 1)
        assert counts["n_errors"] == n_err and len(errs) == n_err - 1 and not as_errors(errs) - errors
        assert as_ints(m) == masks and dmg.tolist() == damaged
        assert [{f: int(x[f]) for f in retain.ROOT_DTYPE.names} for x in pr] == per_root
        # the return code itself
        r = np.frombuffer(b"".join(case["roots"]), dtype=np.uint8)
        mm, dd = np.zeros((case["n_entries"], 1), dtype=np.uint64), np.zeros(case["n_entries"], dtype=np.uint8)
        pp, cnt = np.zeros(2, dtype=retain.ROOT_DTYPE), _lib.BwRetainCounts()
        ee = np.zeros(1, dtype=ERROR_DTYPE)
        rc = s._L.bw_retain_mark(s.h, r.ctypes.data_as(ctypes.c_void_p), 2, _lib.BW_UNPACK_VERIFY, mm.ctypes.data_as(_lib.u64p),
                                 dd.ctypes.data_as(_lib.u8p), pp.ctypes.data_as(ctypes.POINTER(_lib.BwRetainRoot)),
                                 ctypes.byref(cnt), ee.ctypes.data_as(ctypes.POINTER(_lib.BwPruneError)), 1)
        assert rc == _lib.BW_ENOSPC and as_ints(mm) == masks and int(cnt.n_errors) == 2


def test_the_live_of_a_drop_set_plans_what_prune_plans_for_the_kept_roots(ctx, oracle):
    import restore_store
    from backuwup_amd import prune, retain
    case, _, _, _, _, _, _ = ref("shared")
    files, ids, entries, items = store_args(ctx, case)
    new_ids = [bytes([0xE0 + k]) * 12 for k in range(8)]
    with session(ctx, case) as s:
        m, _, _, _, _ = retain.mark(s, case["roots"])
        live, stats, _ = retain.drop(s, m, 2, [[0]])
    rewrite = prune.choose_rewrite(stats[0])
    order, pl, total = prune.plan(entries, prune.packfile_table(files), live[0], rewrite)
    report = prune.prune(ctx, files, ids, entries, items, restore_store.PRK, [case["roots"][1]], new_ids)[3]
    assert rewrite.any() and rewrite.tolist() == report["rewrite"].tolist()
    assert order.tolist() == report["order"].tolist() and pl.tobytes() == report["plan"].tobytes() and total == report["total_bytes"]


def test_foreign_bits_and_too_many_roots_are_refused(ctx, oracle):
    from backuwup_amd import _lib, retain
    case, _, _, _, _, _, _ = ref("clean")
    with session(ctx, case) as s:
        m, _, _, _, _ = retain.mark(s, case["roots"])
        freed = _lib.BwRetainFreed()
        one = np.array([1], dtype=np.uint64)
        two = np.array([2], dtype=np.uint64)

        def call(masks, n_roots, drop):
            return s._L.bw_retain_drop(s.h, masks.ctypes.data_as(_lib.u64p), n_roots, drop.ctypes.data_as(_lib.u64p), 1, None, None,
                                       ctypes.byref(freed))
        flat = np.ascontiguousarray(m).reshape(-1)
        assert call(flat, 1, one) == _lib.BW_OK and int(freed.freed_blobs) == case["n_entries"]
        assert call(flat, 1, two) == _lib.BW_EINVAL  # a drop word with root 1's bit
        bad = flat.copy()
        bad[3] |= np.uint64(4)
        assert call(bad, 1, one) == _lib.BW_EINVAL  # a mask word with root 2's bit
        assert call(flat, 0, np.zeros(1, dtype=np.uint64)) == _lib.BW_EINVAL  # no roots: every bit is foreign
        wide = np.zeros(case["n_entries"] * 65, dtype=np.uint64)
        assert call(wide, 4097, np.zeros(65, dtype=np.uint64)) == _lib.BW_ENOMEM
        with pytest.raises(_lib.BwError) as e:
            retain.mark(s, [case["roots"][0]] * 4097)
        assert e.value.rc == _lib.BW_ENOMEM
