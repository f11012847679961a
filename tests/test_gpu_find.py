"""bw_find_paths (backuwup_amd.find) against tests/find_ref.py over the stores of tests/find_stores.py.
Every query of every case on a fresh session: the records in order with parents resolved to paths, the
names, the chunk rows, per_root, all counts and the errors as a multiset equal the reference's exactly.
Then the caps: one too small gives BW_ENOSPC with the earlier levels filled in and nothing written past a
cap.  Small stores; a store and its reference results are built once (find_stores.reference) and shared."""
import ctypes
import os
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import find_stores  # noqa: E402
import zstd_ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]

NONE = 2**64 - 1
CANARY = 0xA5


def session(ctx, case):
    import restore_store
    from backuwup_amd import restore
    files, ids = [b for _, b in case["packs"]], [i for i, _ in case["packs"]]
    return restore.Session(ctx, restore_store.PRK, files, ids, ctx.unpack_headers(restore_store.PRK, files, ids),
                           restore_store.items_array(case["index"]), slots=case["slots"])


def as_errors(errors):
    return Counter((bytes(e["hash"]), bytes(e["parent"]), int(e["child_pos"]), int(e["reason"])) for e in errors)


def as_ref_records(records, names):
    """The library's records as find_ref.resolve gives the reference's: level and path through parent."""
    import find_ref
    out, level, path = [], [], []
    for i, r in enumerate(records):
        parent = int(r["parent"])
        assert parent == NONE or parent < i
        h = bytes(r["hash"])
        name = bytes(names[int(r["name_off"]):int(r["name_off"]) + int(r["name_len"])])
        unreadable = int(r["flags"]) & find_ref.UNREADABLE
        level.append(0 if parent == NONE else level[parent] + 1)
        path.append((() if parent == NONE else path[parent]) + ((b"?" + h,) if unreadable else () if parent == NONE else (name,)))
        assert parent == NONE or int(records[parent]["root"]) == int(r["root"])
        out.append(dict(level=level[i], root=int(r["root"]), parent=None if parent == NONE else parent, path=path[i], hash=h,
                        name=name, kind=int(r["kind"]), meta_flags=int(r["meta_flags"]), size=int(r["size"]), mtime=int(r["mtime"]),
                        ctime=int(r["ctime"]), child_first=int(r["child_first"]), n_children=int(r["n_children"]),
                        patterns=int(r["patterns"]), flags=int(r["flags"])))
    return find_ref.resolve(out)


@pytest.mark.parametrize("name, qi", find_stores.all_queries())
def test_every_query_of_every_case(ctx, oracle, name, qi):
    import find_ref
    from backuwup_amd import find
    case, query, want = find_stores.reference(name, qi)
    with session(ctx, case) as s:
        recs, names, rows, per_root, counts, errs = find.paths(s, case["roots"], verify=case["verify"], **query)
    got, ref = as_ref_records(recs, names), find_ref.resolve(want["records"])
    assert got == ref, next((g, w) for g, w in zip(got + [None], ref + [None]) if g != w)
    assert [bytes(r) for r in rows] == want["chunks"]
    assert [{f: int(x[f]) for f in find.ROOT_DTYPE.names} for x in per_root] == want["per_root"]
    assert counts == want["counts"]
    assert as_errors(errs) == want["errors"]
    assert len(names) == sum(len(r["name"]) for r in want["records"])


# ------------------------------------------------------------------ capacity
def raw_paths(s, roots, query, record_cap, names_cap, chunks_cap, err_cap):
    """bw_find_paths with exactly these caps and a canary behind each array: (rc, records, names, rows, counts)."""
    L = sys.modules["backuwup_amd._lib"]
    from backuwup_amd import find
    from backuwup_amd.prune import ERROR_DTYPE
    r = np.frombuffer(b"".join(roots), dtype=np.uint8)
    size = find.RECORD_DTYPE.itemsize
    records = np.full((record_cap + 1) * size, CANARY, dtype=np.uint8)
    names = np.full(names_cap + 64, CANARY, dtype=np.uint8)
    rows = np.full((chunks_cap + 1) * 32, CANARY, dtype=np.uint8)
    errs = np.full((err_cap + 1) * ERROR_DTYPE.itemsize, CANARY, dtype=np.uint8)
    per_root = np.full((len(roots) + 1) * 40, CANARY, dtype=np.uint8)
    cnt = L.BwFindCounts()
    fq = find.Query(query["patterns"], query.get("kinds"), query.get("size"), query.get("mtime"))
    flags = find.flags_of(query.get("icase", False), query.get("subtree", False), query.get("chunks", False))
    rc = s._L.bw_find_paths(s.h, r.ctypes.data_as(ctypes.c_void_p), len(roots), ctypes.byref(fq.q), flags,
                            records.ctypes.data_as(ctypes.POINTER(L.BwFindRecord)), record_cap, names.ctypes.data_as(ctypes.c_void_p),
                            names_cap, rows.ctypes.data_as(ctypes.c_void_p), chunks_cap,
                            per_root.ctypes.data_as(ctypes.POINTER(L.BwFindRoot)), ctypes.byref(cnt),
                            errs.ctypes.data_as(ctypes.POINTER(L.BwPruneError)), err_cap)
    assert (records[record_cap * size:] == CANARY).all() and (names[names_cap:] == CANARY).all()
    assert (rows[chunks_cap * 32:] == CANARY).all() and (errs[err_cap * ERROR_DTYPE.itemsize:] == CANARY).all()
    assert (per_root[len(roots) * 40:] == CANARY).all()
    counts = {f: int(getattr(cnt, f)) for f in find.COUNT_FIELDS}
    return rc, records[:record_cap * size].view(find.RECORD_DTYPE), names[:names_cap].tobytes(), rows[:chunks_cap * 32].reshape(-1, 32), counts


@pytest.mark.parametrize("name, qi", find_stores.all_queries())
def test_caps_one_short_at_the_first_a_middle_and_the_last_level(ctx, oracle, name, qi):
    """Every query of every case.  The totals per level come from the reference's records; record_cap, names_cap
    and chunks_cap are each tried one short of the total after the first, a middle and the last level (a level
    that adds nothing to a cap cannot be one short of it and is passed over), and err_cap one short of the errors."""
    import find_ref
    L = sys.modules["backuwup_amd._lib"]
    case, query, want = find_stores.reference(name, qi)
    recs = want["records"]
    n_levels, n_err = want["counts"]["n_levels"], want["counts"]["n_errors"]
    with_rows = bool(query.get("chunks"))
    after = []  # (records, name bytes, chunk rows) up to and including each level
    for lv in range(n_levels):
        upto = [r for r in recs if r["level"] <= lv]
        after.append((len(upto), sum(len(r["name"]) for r in upto),
                      sum(r["n_children"] for r in upto if with_rows and r["kind"] == 0 and r["flags"] & find_ref.HIT
                          and not r["flags"] & find_ref.UNREADABLE)))
    total = after[-1]
    assert total == (len(recs), want["counts"]["name_bytes"], want["counts"]["n_chunks"])
    ref = find_ref.resolve(recs)
    tried = 0
    with session(ctx, case) as s:
        rc, got, names, rows, counts = raw_paths(s, case["roots"], query, total[0], total[1], total[2], n_err)
        assert rc == L.BW_OK and as_ref_records(got, names) == ref and [bytes(r) for r in rows] == want["chunks"]
        for which in range(3):
            for lv in sorted({0, n_levels // 2, n_levels - 1}):
                before = after[lv - 1] if lv else (0, 0, 0)
                if after[lv][which] == before[which]:
                    continue
                caps = list(total)
                caps[which] = after[lv][which] - 1
                rc, got, names, rows, counts = raw_paths(s, case["roots"], query, caps[0], caps[1], caps[2], n_err)
                assert rc == L.BW_ENOSPC, (which, lv)
                assert (counts["n_records"], counts["name_bytes"], counts["n_chunks"], counts["n_levels"]) == after[lv] + (lv + 1,)
                assert as_ref_records(got[:before[0]], names) == ref[:before[0]]  # the levels before are intact
                assert [bytes(r) for r in rows[:before[2]]] == want["chunks"][:before[2]]
                tried += 1
        if n_err:
            rc, got, names, rows, counts = raw_paths(s, case["roots"], query, total[0], total[1], total[2], n_err - 1)
            assert rc == L.BW_ENOSPC and counts["n_errors"] == n_err and counts["n_records"] == len(recs)
            assert as_ref_records(got, names) == ref and [bytes(r) for r in rows] == want["chunks"]
    assert tried >= 1  # every query has a record at level 0


def test_the_cap_cases_cover_chunk_rows_of_two_pieces_and_of_the_damaged_store(oracle):
    for name, qi in (("two_pieces", 1), ("two_pieces", 2), ("damaged", 1), ("shared", 2), ("wide", 2)):
        _, query, want = find_stores.reference(name, qi)
        assert query.get("chunks") and want["counts"]["n_chunks"] > 0, (name, qi)
    assert find_stores.reference("damaged", 1)[2]["counts"]["n_errors"] >= 2


def test_more_errors_than_err_cap_is_enospc_with_everything_else_filled(ctx, oracle):
    import find_ref
    L = sys.modules["backuwup_amd._lib"]
    case, query, want = find_stores.reference("damaged", 0)
    n_err = sum(want["errors"].values())
    assert n_err >= 2
    with session(ctx, case) as s:
        rc, got, names, _, counts = raw_paths(s, case["roots"], query, len(want["records"]), 256, 0, n_err - 1)
    assert rc == L.BW_ENOSPC and counts["n_errors"] == n_err and counts["n_records"] == len(want["records"])
    assert as_ref_records(got, names) == find_ref.resolve(want["records"])


@pytest.mark.parametrize("patterns", [[], [b"a"] * 33, [b"a//b"], [b"ok", b"[ab"], [b"/" + b"a" * 64]])
def test_refused_queries_are_einval(ctx, oracle, patterns):
    L = sys.modules["backuwup_amd._lib"]
    case = find_stores.case("shared")[0]
    with session(ctx, case) as s:
        rc = raw_paths(s, case["roots"], dict(patterns=patterns), 8, 64, 0, 4)[0]
        assert rc == L.BW_EINVAL
