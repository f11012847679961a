"""The planted cases of tests/table_plant.py on the device: the locator's three tables through
Session.locate, the diff walk's name join and row set through diff.trees, the parent match's join through
parent.match.  Every comparison is exact, with the case's answer by construction and with the reference
(prune_ref.Locator over restore_ref.Store, diff_ref.diff, parent_ref.match).  That a case reaches the
path it is planted for is tests/test_table_plant.py's to show, on the CPU: the occupied set of linear
probing does not depend on the order the lanes claim in.  Every case opens a session of its own; all
walks run with verify off (planted tree hashes are no BLAKE3 outputs)."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import table_plant as P  # noqa: E402
import zstd_ref  # noqa: E402
from test_gpu_diff_walk import as_ref_errors, as_ref_records  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]

NONE = 2**64 - 1


def session(ctx, c, slots=16):
    import restore_store
    from backuwup_amd import restore
    files, ids = [b for _, b in c["packs"]], [i for i, _ in c["packs"]]
    return restore.Session(ctx, P.PRK, files, ids, ctx.unpack_headers(P.PRK, files, ids), restore_store.items_array(c["index"]),
                           slots=slots)


# ------------------------------------------------------------------ the locator
@pytest.mark.parametrize("name,slots", [(n, 16) for n in P.LOCATE] + [("crowd", 4)])
def test_locate(ctx, oracle, name, slots):
    c = P.case(name)
    ref = P.reference_locate(c)
    with session(ctx, c, slots) as s:
        assert s.n_entries == len(c["entries"])
        idx, st = s.locate(c["queries"])
    got = [(int(code), None if code else int(i)) for i, code in zip(idx, st)]
    assert [int(i) for i, code in zip(idx, st) if code] == [NONE] * sum(1 for code in st if code)
    bad = [(k, g, w, r) for k, (g, w, r) in enumerate(zip(got, c["want"], ref)) if not g == w == r]
    assert not bad, bad[:5]


# ------------------------------------------------------------------ the diff walk
@pytest.mark.parametrize("name,slots", [(n, 16) for n in P.DIFF] + [("names_crowd", 4)])
def test_diff(ctx, oracle, name, slots):
    import diff_ref
    from backuwup_amd import diff
    c = P.case(name)
    want_records, want_errors, want_read, want_levels = P.reference_diff(c)
    with session(ctx, c, slots) as s:
        records, names, read, counts, errors = diff.trees(s, c["root_a"], c["root_b"], verify=False)
    got = as_ref_records(records, names)
    # the seed of the planted homes: the roots' record is record 0, and every other record is its child
    assert got[0]["parent"] == NONE and all(r["parent"] == 0 for r in got[1:])
    assert P.level1_records(got) == c["want"]
    got_multi, want_multi = Counter(diff_ref.resolve(got)), Counter(diff_ref.resolve(want_records))
    assert got_multi == want_multi, (sorted(got_multi - want_multi, key=str)[:3], sorted(want_multi - got_multi, key=str)[:3])
    assert as_ref_errors(errors) == want_errors == Counter()
    assert set(np.flatnonzero(read).tolist()) == set(want_read) and set(np.unique(read).tolist()) <= {0, 1}
    assert counts["n_levels"] == want_levels == 2 and counts["n_read"] == len(want_read)
    assert counts["n_records"] == len(records) == len(want_records) and counts["n_errors"] == 0
    assert counts["name_bytes"] == len(names)
    if "file_want" in c:
        f, w = got[1], c["file_want"]
        assert (f["n_new"], f["common_prefix"], f["common_suffix"], f["a"][6], f["b"][6]) == \
            (w["n_new"], w["common_prefix"], w["common_suffix"], w["n_a"], w["n_b"])


# ------------------------------------------------------------------ the parent match
@pytest.mark.parametrize("name", P.PARENT)
def test_parent_match(ctx, oracle, name):
    from backuwup_amd import parent, restore
    from test_gpu_parent_match import compare
    c = P.case(name)
    want = P.reference_parent(c)
    nodes, names = np.zeros(len(c["scan"]), dtype=restore.NODE_DTYPE), bytearray()
    for i, n in enumerate(c["scan"]):
        nodes[i] = (n["kind"], n["flags"], n["size"], n["mtime"], n["ctime"], NONE, n["child_first"], n["n_children"],
                    len(names), len(n["name"]))
        names += n["name"]
    with session(ctx, c) as s:
        got = parent.match(s, c["root"], nodes, bytes(names), verify=False)
    results = got[0]
    # the seed of the planted homes: the roots paired as Dir against Dir, so the children are item 0's
    assert (int(results[0]["status"]), bytes(results[0]["hash"])) == (4, c["root"]) and got[2]["n_levels"] == 1
    assert [None if bytes(r["hash"]) == P.ZERO else bytes(r["hash"]) for r in results[1:]] == c["want"]
    assert [int(r["status"]) for r in results[1:]] == c["status"]
    compare(got, want)
