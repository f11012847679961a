"""tests/retain_ref.py, the plain Python restatement of retain (include/backuwup_gpu_pack.h, "retain"),
pinned to hand-written expectations over the stores of tests/retain_stores.py: the masks below are worked
out by hand from the builder calls (a blob's entry index is its position in add order; bit r = root r).
The reference's masks are prune_ref.mark once per root; the edge rule taken to its fixed point over the
edges of one walk must give the same, on every case.  Then what needs no device of the library: the
exports, the refusals that come before the session is looked at, and retain.mask_of.  The device runs the
same cases in tests/test_gpu_retain.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402

needs_zstd = pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")
ENOTFOUND, ENOTTREE, ETAG, EDIGEST = 16, 19, 1, 3
NONE = 2**64 - 1


def ref(name, arg=None):
    import retain_stores
    return retain_stores.reference(name, arg)


def roots_figures(per_root):
    return [(p["reached_blobs"], p["unique_blobs"], p["n_damaged"], p["status"]) for p in per_root]


@needs_zstd
def test_clean_and_duplicate_hashes(oracle):
    _, _, masks, damaged, per_root, errors, info = ref("clean")
    assert masks == [1] * 6 and damaged == [0] * 6 and not errors and roots_figures(per_root) == [(6, 6, 0, 0)]
    assert info["n_trees_expanded"] == 4 and info["n_edges"] == 5 and info["orphan_blobs"] == 0
    # entries: D, D again, f, r: the shadowed entry is an orphan
    _, hd, masks, _, per_root, _, info = ref("duplicate_hashes")
    assert masks == [1, 0, 1, 1] and info["orphan_blobs"] == 1 and info["reached_blobs"] == 3
    assert info["orphan_bytes"] == 12 + hd[0][3][1][3]


@needs_zstd
def test_shared(oracle):
    # entries: X, f, d1, g, Y, h, d2, r, Z, z, w, r2
    _, _, masks, _, per_root, errors, info = ref("shared")
    assert masks == [3, 1, 1, 3, 3, 3, 3, 1, 2, 2, 2, 2] and not errors
    assert roots_figures(per_root) == [(8, 3, 0, 0), (9, 4, 0, 0)]
    assert info["n_trees_expanded"] == 9  # every tree blob once, d2's three for both roots together


@needs_zstd
def test_late_parent_needs_a_second_productive_sweep(oracle):
    # entries: X, x, s, a, b5, b4, b3, b2, b1, b.  s is expanded at level 1 under a, and named again by b5 at level 5
    _, _, masks, _, per_root, _, info = ref("late_parent")
    assert masks == [3, 3, 3, 1, 2, 2, 2, 2, 2, 2]
    assert info["n_sweeps"] == 3 and info["n_levels"] == 6 and info["n_edges"] == 9
    assert roots_figures(per_root) == [(4, 1, 0, 0), (9, 6, 0, 0)]


@needs_zstd
def test_a_file_row_reaches_a_tree_and_does_not_open_it(oracle):
    # entries: K, k, d, f, a, b: d is reached by both, opened for B alone
    _, _, masks, _, _, errors, info = ref("file_row_names_a_tree")
    assert masks == [2, 2, 3, 1, 1, 2] and not errors
    w = info["walk"]
    assert (3, 2, False) in w["levels"][1] and (5, 2, True) in w["levels"][0]  # f -> d is no tree edge, b -> d is one


@needs_zstd
def test_root_is_a_later_piece(oracle):
    # entries: P, p, Q, q, big piece 1, big piece 2
    _, _, masks, _, per_root, _, info = ref("root_is_a_later_piece")
    assert masks == [1, 1, 3, 3, 1, 3] and info["n_edges"] == 10001 + 3
    assert roots_figures(per_root) == [(6, 3, 0, 0), (3, 0, 0, 0)]


@needs_zstd
def test_roots_at_the_edges(oracle):
    # entries: F, f, G, g, r
    _, _, masks, _, per_root, _, info = ref("duplicate_roots")
    assert masks == [3] * 5 and roots_figures(per_root) == [(5, 0, 0, 0)] * 2 and info["n_trees_expanded"] == 3
    _, _, masks, _, per_root, errors, info = ref("zero_roots")
    assert masks == [0] * 5 and per_root == [] and not errors and info["orphan_blobs"] == 5 and info["n_sweeps"] == 1
    _, _, masks, _, per_root, errors, _ = ref("root_missing")
    assert masks == [2] * 5 and roots_figures(per_root) == [(0, 0, 0, ENOTFOUND), (5, 5, 0, 0)]
    assert dict(errors) == {(b"\x11" * 32, bytes(32), 0, ENOTFOUND): 1}
    _, _, masks, _, per_root, errors, _ = ref("root_is_a_chunk")
    assert masks == [3, 2, 2, 2, 2] and roots_figures(per_root) == [(1, 0, 0, ENOTTREE), (5, 4, 0, 0)]
    assert [k[3] for k in errors] == [ENOTTREE]


@needs_zstd
def test_many_roots_and_wide(oracle):
    for n in (2, 65):
        _, _, masks, _, per_root, _, _ = ref("many_roots", n)
        # entries: C, common, then per root: its chunk, its file, its Dir
        assert masks[:2] == [2**n - 1] * 2 and all(masks[2 + 3 * i + k] == 1 << i for i in range(n) for k in range(3))
        assert roots_figures(per_root) == [(5, 3, 0, 0)] * n
    _, _, masks, _, per_root, _, info = ref("wide")
    n1, n2 = 63 + 64 + 65 + 256 + 257, 63 + 65 + 257
    assert (per_root[0]["reached_blobs"], per_root[1]["reached_blobs"]) == (2 * n1 + 5 + 1, 2 * n2 + 3 + 1)
    assert per_root[1]["unique_blobs"] == 1 and sum(1 for m in masks if m == 3) == 2 * n2 + 3
    assert ref("wide", 4)[2] == masks and ref("wide", 4)[0]["slots"] == 4


@needs_zstd
def test_real_damage(oracle):
    # entries: A, a, B, b, t, C, c, u (under the forged hash), r, r2: t and u are not opened, so B and b are orphans
    case, _, masks, damaged, per_root, errors, info = ref("real_damage")
    i, zero = case["info"], bytes(32)
    assert masks == [1, 1, 0, 0, 3, 2, 2, 1, 1, 2] and damaged == [0, 0, 0, 0, 1, 0, 0, 1, 0, 0]
    assert dict(errors) == {(i["tag"], zero, NONE, ETAG): 1, (i["digest"], zero, NONE, EDIGEST): 1}
    assert roots_figures(per_root) == [(5, 4, 2, 0), (4, 3, 1, 0)] and info["orphan_blobs"] == 2


@needs_zstd
def test_the_edge_rule_reaches_the_definition_on_every_case(oracle):
    import retain_ref
    import retain_stores
    for name, arg in retain_stores.CASES:
        _, _, masks, _, _, _, info = ref(name, arg)
        assert retain_ref.fixed_point(info["walk"])[0] == masks, (name, arg)


@needs_zstd
def test_drop_against_a_prune_mark_over_the_kept_roots(oracle):
    import prune_ref
    import restore_ref
    import restore_store
    import retain_ref
    import retain_stores
    for name, arg in (("shared", None), ("late_parent", None), ("file_row_names_a_tree", None), ("many_roots", 65)):
        case, hd, masks, _, _, _, _ = ref(name, arg)
        store = restore_ref.Store(restore_store.PRK, case["packs"], case["index"])
        n = len(case["roots"])
        for dropped in retain_stores.drop_sets(n):
            live, stats, freed = retain_ref.drop(hd, masks, dropped)
            kept = [r for k, r in enumerate(case["roots"]) if k not in dropped]
            plive, _, pinfo = prune_ref.mark(store, hd, kept)
            assert {e for e, v in enumerate(live) if v} == plive and stats == pinfo["stats"], (name, dropped)
            assert freed["live_blobs"] == len(plive) and freed["freed_blobs"] + freed["live_blobs"] == sum(1 for m in masks if m)


def test_drop_sets_are_what_the_issue_lists():
    import retain_stores
    sets = retain_stores.drop_sets(129)
    assert sets[0] == [] and sets[8] == list(range(129)) and len(sets) == 13
    assert [s[0] for s in sets[1:8]] == [0, 21, 42, 64, 85, 106, 128] and all(len(s) == 1 for s in sets[1:8])
    assert retain_stores.drop_sets(0) == [[], [], [], [], [], []] and retain_stores.drop_sets(2)[:4] == [[], [0], [1], [0, 1]]


# ------------------------------------------------------------------ the library, without a device
def test_mask_of_and_roots_of():
    from backuwup_amd import retain
    assert retain.words(0) == 1 and retain.words(64) == 1 and retain.words(65) == 2 and retain.words(4096) == 64
    assert retain.mask_of([], 0).tolist() == [0] and retain.mask_of([0, 63], 64).tolist() == [1 | 1 << 63]
    assert retain.mask_of([64, 1, 128], 129).tolist() == [2, 1, 1]
    assert retain.roots_of(retain.mask_of([5, 64, 128, 70], 129)) == [5, 64, 70, 128]
    for bad in ([64], [-1]):
        with pytest.raises(ValueError):
            retain.mask_of(bad, 64)
    import retain_ref
    assert retain_ref.words_of((1 << 128) | 2, 129) == retain.mask_of([1, 128], 129).tolist()


def test_library_exports_both_symbols_and_refuses_before_the_session_is_read():
    from backuwup_amd import _lib, retain
    L = _lib.load()
    assert hasattr(L, "bw_retain_mark") and hasattr(L, "bw_retain_drop") and retain.MAX_ROOTS == 4096
    cnt, root, freed = _lib.BwRetainCounts(), _lib.BwRetainRoot(), _lib.BwRetainFreed()
    roots = np.zeros(32, dtype=np.uint8)
    words = np.zeros(65, dtype=np.uint64)
    r8, w64 = roots.ctypes.data_as(ctypes.c_void_p), words.ctypes.data_as(_lib.u64p)
    # no session: null arguments are BW_EINVAL, the size limit is the walks' BW_ENOMEM whatever else is given
    assert L.bw_retain_mark(None, r8, 1, 0, w64, None, ctypes.byref(root), ctypes.byref(cnt), None, 0) == _lib.BW_EINVAL
    assert L.bw_retain_mark(None, None, 0, 0, None, None, None, None, None, 0) == _lib.BW_EINVAL
    assert L.bw_retain_mark(None, r8, 4097, 0, w64, None, ctypes.byref(root), ctypes.byref(cnt), None, 0) == _lib.BW_ENOMEM
    assert L.bw_retain_mark(None, r8, 4096, 0, w64, None, ctypes.byref(root), ctypes.byref(cnt), None, 0) == _lib.BW_EINVAL
    assert L.bw_retain_drop(None, w64, 1, w64, 1, None, None, ctypes.byref(freed)) == _lib.BW_EINVAL
    assert L.bw_retain_drop(None, w64, 4097, w64, 1, None, None, ctypes.byref(freed)) == _lib.BW_ENOMEM
    words[0] = 2  # a bit of root 1 where one root was given: refused with or without a session
    assert L.bw_retain_drop(None, w64, 1, w64, 1, None, None, ctypes.byref(freed)) == _lib.BW_EINVAL
    assert ctypes.sizeof(_lib.BwRetainRoot) == 48 and ctypes.sizeof(_lib.BwRetainCounts) == 72
    assert [f for f, _ in _lib.BwRetainFreed._fields_] == list(retain.FREED_DTYPE.names)
    assert [f for f, _ in _lib.BwRetainRoot._fields_] == list(retain.ROOT_DTYPE.names)
