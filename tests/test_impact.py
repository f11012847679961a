"""tests/impact_ref.py, the plain Python restatement of impact (include/backuwup_gpu_pack.h, "impact"),
pinned to hand-written expectations over the stores of tests/impact_stores.py: the taint bytes and the
path lists below are worked out by hand from the builder calls (a blob's entry index is its position in
add order).  For chunk-only damage the reference's affected File paths are also what restore_ref's
restore fails on when the bad chunks are taken out of the index.  The device runs the same cases in
tests/test_gpu_impact.py."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402

pytestmark = pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")

U, T, C = 1, 2, 4  # UNREADABLE, TRUNCATED, CYCLIC
NONE = 2**64 - 1


def ref(name, arg=None):
    import impact_stores
    return impact_stores.reference(name, arg)


def listing(records):
    """[(root, path below the root's own name, kind, flags, n_affected, n_children)] sorted; an unreadable
    item's last component is '?'."""
    out = []
    for r in records:
        parts = [p.decode() if not p.startswith(b"?") else "?" for p in r["path"][1:]]
        if len(r["path"]) == 1 and r["flags"] & U:
            parts = ["?"]
        out.append((r["root"], "/".join(parts), r["kind"], r["flags"], r["n_affected"], r["n_children"]))
    return sorted(out)


def test_clean(oracle):
    _, taint, affected, errors, info, records, per_root, perrors = ref("clean")
    assert taint == [0, 0, 0, 0, 0, 0] and affected == [0] and not errors and not records and not perrors
    assert info["n_sweeps"] == 1 and info["n_trees_expanded"] == 4 and info["n_tainted"] == 0


def test_shared_chunk(oracle):
    # entries: X, f, d1, g, Y, h, d2, r, Z, z, r2
    case, taint, affected, errors, info, records, per_root, _ = ref("shared_chunk")
    assert taint == [1, 2, 2, 2, 0, 0, 2, 2, 0, 0, 2] and affected == [1, 1] and not errors
    assert info["n_trees_expanded"] == case["info"]["n_tree_blobs"] == 8
    assert listing(records) == [(0, "", 1, 0, 2, 2), (0, "d1", 1, 0, 1, 1), (0, "d1/f", 0, 0, 1, 1), (0, "d2", 1, 0, 1, 2),
                                (0, "d2/g", 0, 0, 1, 1), (1, "", 1, 0, 1, 2), (1, "d2", 1, 0, 1, 2), (1, "d2/g", 0, 0, 1, 1)]
    assert per_root == [dict(n_records=5, n_files=2, n_unreadable=0, lost_chunk_refs=2),
                        dict(n_records=3, n_files=1, n_unreadable=0, lost_chunk_refs=1)]


def test_lost_directory(oracle):
    # entries: A, a, B, b, d, m, r; d is lost: it is never opened, so B and b are never reached
    _, taint, affected, errors, info, records, per_root, perrors = ref("lost_directory")
    assert taint == [0, 0, 0, 0, 1, 2, 2] and affected == [1] and not errors and not perrors
    assert info["n_trees_expanded"] == 3
    assert listing(records) == [(0, "", 1, 0, 1, 2), (0, "m", 1, 0, 1, 1), (0, "m/?", 0, U, 0, 0)]
    lost = [r for r in records if r["flags"] & U][0]
    assert lost["name"] == b"" and lost["hash"] == ref("lost_directory")[0]["info"]["lost"]
    assert per_root == [dict(n_records=3, n_files=0, n_unreadable=1, lost_chunk_refs=0)]


def test_lost_later_piece(oracle):
    _, taint, affected, errors, info, records, per_root, perrors = ref("lost_later_piece")
    assert affected == [1] and not errors and not perrors
    assert listing(records) == [(0, "", 1, 0, 2, 2), (0, "big", 1, T, 0, 10000), (0, "f", 0, T, 0, 10000)]
    # entries: S, s, C, big (two pieces), f (two pieces), r: the second pieces are lost, the first ones and the root BELOW
    assert taint == [0, 0, 0, 2, 1, 2, 1, 2]


def test_late_parent(oracle):
    # entries: X, x, s, a5, a4, a3, a2, a1, r.  s is expanded at level 2 and named again by a5 at level 6
    _, taint, affected, errors, info, records, per_root, _ = ref("late_parent")
    assert taint == [1, 2, 2, 2, 2, 2, 2, 2, 2] and affected == [1] and not errors
    assert info["n_sweeps"] == 3 and info["n_edges"] == 8 and info["n_levels"] == 6
    deep = "a1/a2/a3/a4/a5"
    want = [(0, "", 1, 0, 2, 2), (0, "s", 1, 0, 1, 1), (0, "s/x", 0, 0, 1, 1)]
    want += [(0, deep[:2 + 3 * k], 1, 0, 1, 1) for k in range(5)] + [(0, deep + "/s", 1, 0, 1, 1), (0, deep + "/s/x", 0, 0, 1, 1)]
    assert listing(records) == sorted(want)


def test_wide_and_four_slots(oracle):
    case, taint, affected, errors, info, records, per_root, _ = ref("wide")
    n_bad = sum(len(range(0, n, 7)) for n in (63, 64, 65, 256, 257))
    assert len(case["bad"]) == n_bad == 103 and not errors
    assert sum(1 for t in taint if t == 1) == n_bad and sum(1 for t in taint if t == 2) == n_bad + 6
    got = listing(records)
    assert [x for x in got if x[2] == 1] == [(0, "", 1, 0, 5, 5)] + sorted(
        (0, "d%d" % n, 1, 0, len(range(0, n, 7)), n) for n in (63, 64, 65, 256, 257))
    assert [x[1] for x in got if x[2] == 0] == sorted("d%d/f%03d" % (n, i) for n in (63, 64, 65, 256, 257) for i in range(0, n, 7))
    assert ref("four_slots")[1] == taint


def test_duplicate_hashes(oracle):
    # entries: D, D again, f, r; locate resolves the hash to entry 0
    assert ref("duplicate_hashes", 1)[1] == [0, 0, 0, 0] and ref("duplicate_hashes", 1)[2] == [0] and not ref("duplicate_hashes", 1)[5]
    _, taint, affected, _, _, records, _, _ = ref("duplicate_hashes", 0)
    assert taint == [1, 0, 2, 2] and affected == [1]
    assert listing(records) == [(0, "", 1, 0, 1, 1), (0, "f", 0, 0, 1, 1)]


@pytest.mark.parametrize("p", range(6))
def test_whole_packfile_against_a_restore_without_it(oracle, p):
    import impact_ref
    case, taint, _, _, _, records, _, _ = ref("whole_packfile", p)
    assert len(case["packs"]) == case["info"]["n_packfiles"] == 6
    lost = [e for e, t in enumerate(taint) if t & 1]  # a lost tree blob is never opened: what only it names is not reached
    assert lost and set(lost) <= set(case["bad"]) and len(case["bad"]) == (4 if p < 5 else 2)
    if all(chunk_only(case)):
        assert impact_ref.file_paths(records, 0) == restore_failures(case)


def chunk_only(case):
    import prune_ref
    import restore_store
    ents = prune_ref.flat_entries(prune_ref.headers_of(restore_store.PRK, case["packs"]))
    return [ents[e][2] == 0 for e in case["bad"]]


def restore_failures(case, root=0):
    """The paths restore_ref's restore fails on once the bad chunks are gone from the index."""
    import prune_ref
    import restore_ref
    import restore_store
    ents = prune_ref.flat_entries(prune_ref.headers_of(restore_store.PRK, case["packs"]))
    gone = {ents[e][1] for e in case["bad"]}
    store = restore_ref.Store(restore_store.PRK, case["packs"], [(h, pid) for h, pid in case["index"] if h not in gone])
    return sorted(restore_ref.unpack(store, case["roots"][root])[2])


@pytest.mark.parametrize("name,arg", [("shared_chunk", None), ("late_parent", None), ("wide", None), ("duplicate_hashes", 0)])
def test_affected_files_are_what_restore_fails_on(oracle, name, arg):
    import impact_ref
    case, _, _, _, _, records, _, _ = ref(name, arg)
    assert all(chunk_only(case))
    for r in range(len(case["roots"])):
        assert impact_ref.file_paths(records, r) == restore_failures(case, r) != []


def test_real_damage(oracle):
    # entries: A, a, B, b, t, C, c, u (under the forged hash), r
    case, taint, affected, errors, info, records, per_root, perrors = ref("real_damage")
    i = case["info"]
    zero = bytes(32)
    assert dict(errors) == {(i["tag"], zero, NONE, 1): 1, (i["digest"], zero, NONE, 3): 1}  # ETAG, EDIGEST; the chunk is not found
    assert taint == [0, 0, 0, 0, 1, 0, 0, 1, 2] and affected == [1] and not perrors
    assert listing(records) == [(0, "", 1, 0, 2, 3), (0, "?", 0, U, 0, 0), (0, "?", 0, U, 0, 0)]
    assert {r["hash"] for r in records if r["flags"] & U} == {i["tag"], i["digest"]}


def test_forged_directory_that_contains_itself(oracle):
    # entries: F, f, loop
    case, taint, affected, errors, info, records, per_root, perrors = ref("dir_contains_itself")
    loop = case["info"]["loop"]
    assert taint == [1, 2, 2] and affected == [1] and not errors and info["n_trees_expanded"] == 2
    assert listing(records) == [(0, "", 1, 0, 2, 2), (0, "f", 0, 0, 1, 1), (0, "loop", 1, C, 0, 0)]
    assert dict(perrors) == {(loop, loop, 0, 20): 1}


def test_forged_chain_that_names_itself(oracle):
    # entries: F, f, loop, r: the chain is followed for as many pieces as the store has entries
    case, taint, affected, errors, info, records, per_root, perrors = ref("chain_names_itself")
    loop = case["info"]["loop"]
    assert taint == [1, 2, 2, 2] and not errors and info["n_trees_expanded"] == 3
    assert dict(perrors) == {(loop, loop, NONE, 20): 1}
    rec = [r for r in records if r["name"] == b"loop"][0]
    assert rec["flags"] == T and rec["n_children"] == rec["n_affected"] == 5 and rec["first_affected"] == 0
    assert sum(1 for r in records if r["name"] == b"f") == 5


def test_edges(oracle):
    # entries: F, f, G, g, r
    assert ref("edges", "none")[1] == [0] * 5 and ref("edges", "none")[2] == [] and not ref("edges", "none")[5]
    _, taint, affected, _, _, records, per_root, _ = ref("edges", "file_root")
    assert taint == [1, 2, 0, 0, 0] and affected == [1] and listing(records) == [(0, "", 0, 0, 1, 1)]
    assert per_root == [dict(n_records=1, n_files=1, n_unreadable=0, lost_chunk_refs=1)]
    _, taint, affected, errors, _, records, per_root, perrors = ref("edges", "unlocatable")
    assert taint == [1, 2, 0, 0, 2] and affected == [1, 1]
    assert dict(errors) == dict(perrors) == {(b"\x11" * 32, bytes(32), 0, 16): 1}
    assert listing(records) == [(0, "?", 0, U, 0, 0), (1, "", 1, 0, 1, 2), (1, "f", 0, 0, 1, 1)]
    _, taint, affected, _, info, records, per_root, _ = ref("edges", "twice")
    assert taint == [1, 2, 0, 0, 2] and affected == [1, 1] and info["n_trees_expanded"] == 3
    assert listing(records) == [(r, p, k, 0, 1, n) for r in (0, 1) for (p, k, n) in (("", 1, 2), ("f", 0, 1))]
    _, taint, affected, _, info, records, per_root, _ = ref("edges", "hundred")
    assert affected == [1] * 100 and info["n_trees_expanded"] == 3 and len(records) == 200
    assert per_root == [dict(n_records=2, n_files=1, n_unreadable=0, lost_chunk_refs=1)] * 100
