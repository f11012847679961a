"""bw_diff_trees (backuwup_amd.diff.trees / diff.diff), the device walk that opens only the tree blobs on
changed paths, against tests/diff_ref.py over the stores of tests/diff_stores.py and
tests/diff_walk_stores.py.  Per case and pair of roots four things are compared, and all four must be
equal: the multiset of resolved records, the multiset of errors, the set of entries read and the
number of levels.  Small stores; every session is opened in a with statement; a store and its
reference results are built once and shared."""
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
from test_diff_listing import df  # noqa: E402,F401

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]

NONE = 2**64 - 1
SIDE = ("kind", "flags", "size", "mtime", "ctime", "n_children")


@functools.lru_cache(maxsize=None)
def built(name, arg=None):
    """(case, Store, headers) of a builder, once per process."""
    import diff_stores
    import diff_walk_stores
    import prune_ref
    import restore_ref
    import restore_store
    fn = getattr(diff_walk_stores, name, None) or getattr(diff_stores, name)
    case = fn() if arg is None else fn(arg)
    return case, restore_ref.Store(restore_store.PRK, case[0], case[1]), prune_ref.headers_of(restore_store.PRK, case[0])


@functools.lru_cache(maxsize=None)
def wanted(name, arg, which):
    """diff_ref.diff for one pair of roots of a case: (records Counter, errors Counter, read set, levels)."""
    import diff_ref
    case, store, hd = built(name, arg)
    ra, rb = roots_of(case, which)
    records, errors, read, levels = diff_ref.diff(store, hd, ra, rb)
    return Counter(diff_ref.resolve(records)), errors, frozenset(read), levels


def roots_of(case, which):
    ra, rb = case[2], case[3]
    return {"ab": (ra, rb), "ba": (rb, ra), "0b": (None, rb), "a0": (ra, None), "aa": (ra, ra), "00": (None, None)}[which]


def store_args(ctx, df, case):
    import restore_store
    files, ids = [b for _, b in case[0]], [i for i, _ in case[0]]
    return files, ids, ctx.unpack_headers(df.PRK, files, ids), restore_store.items_array(case[1])


def as_ref_records(records, names):
    """The library's records in diff_ref's shape."""
    def side(s):
        return (bytes(s["hash"]),) + tuple(int(s[f]) for f in SIDE)
    return [dict(change=int(r["change"]), flags=int(r["flags"]), parent=int(r["parent"]),
                 name=names[int(r["name_off"]):int(r["name_off"]) + int(r["name_len"])], a=side(r["a"]), b=side(r["b"]),
                 common_prefix=int(r["common_prefix"]), common_suffix=int(r["common_suffix"]), n_new=int(r["n_new"]))
            for r in records]


def as_ref_errors(errors):
    return Counter((bytes(e["hash"]), bytes(e["parent"]), int(e["child_pos"]), int(e["reason"])) for e in errors)


def compare(df, got, want):
    records, names, read, counts, errors = got
    want_records, want_errors, want_read, want_levels = want
    for i, r in enumerate(records):                       # rule 6
        assert r["parent"] == NONE or r["parent"] < i
    got_records = Counter(df.dref.resolve(as_ref_records(records, names)))
    assert got_records == want_records, (sorted(got_records - want_records, key=str)[:3],
                                         sorted(want_records - got_records, key=str)[:3])
    got_errors = as_ref_errors(errors)
    assert got_errors == want_errors, (sorted(got_errors - want_errors, key=str)[:3], sorted(want_errors - got_errors, key=str)[:3])
    assert set(np.flatnonzero(read).tolist()) == set(want_read) and set(np.unique(read).tolist()) <= {0, 1}
    assert counts["n_levels"] == want_levels and counts["n_read"] == len(want_read)
    assert counts["n_records"] == len(records) and counts["n_errors"] == len(errors) and counts["name_bytes"] == len(names)


def walk(ctx, df, name, arg=None, which=("ab", "ba", "0b", "a0"), slots=16, verify=False):
    """One session over the case's store; the walk for every pair of roots, each against the reference."""
    case = built(name, arg)[0]
    out = {}
    with df.restore.Session(ctx, df.PRK, *store_args(ctx, df, case), slots=slots) as s:
        for w in which:
            out[w] = df.diff.trees(s, *roots_of(case, w), verify=verify)
            compare(df, out[w], wanted(name, arg, w))
    return out


@pytest.mark.parametrize("kind", ["depth4", "rename", "mtime", "swap"])
def test_basic_walks(ctx, df, kind):
    out = walk(ctx, df, "basic", kind, which=("ab", "ba", "0b", "a0", "aa", "00"))
    for w in ("aa", "00"):                                # identical roots, both NULL: nothing, and nothing read
        records, names, read, counts, errors = out[w]
        assert len(records) == 0 and len(errors) == 0 and not read.any() and counts["n_levels"] == 0 and counts["n_read"] == 0
    if kind == "depth4":                                  # the point of the walk: the changed path only
        _, _, hd = built("basic", kind)
        n_tree = sum(1 for e in df.pref.flat_entries(hd) if e[2] == 1)
        counts = out["ab"][3]
        assert counts["n_read"] == len(wanted("basic", kind, "ab")[2]) and counts["n_read"] < n_tree
        assert counts["n_records"] == 5 and counts["n_levels"] == 5


def test_directory_metadata_only(ctx, df):
    walk(ctx, df, "dir_metadata_only")


@pytest.mark.parametrize("slots,verify", [(0, False), (4, False), (16, True)])   # 0: the default, 1,024 slots
def test_membership_at_the_wave_boundaries(ctx, df, slots, verify):
    walk(ctx, df, "membership", slots=slots, verify=verify)


@pytest.mark.parametrize("name", ["duplicates", "names"])
def test_duplicates_and_names(ctx, df, name):
    walk(ctx, df, name)


def test_chunk_lists(ctx, df):
    out = walk(ctx, df, "chunk_lists")
    records, names, _, _, _ = out["ab"]
    want = built("chunk_lists")[0][4]["want"]
    seen = {}
    for r in as_ref_records(records, names):
        if r["parent"] != NONE:
            seen[r["name"].decode()] = (r["common_prefix"], r["common_suffix"], r["n_new"])
    assert seen == want


def test_chains(ctx, df):
    out = walk(ctx, df, "chains", slots=8)
    by_name = {r["name"]: r for r in as_ref_records(*out["ab"][:2])}
    big = by_name[b"big"]
    assert (big["a"][6], big["b"][6], big["common_prefix"], big["common_suffix"], big["n_new"]) == (25001, 25001, 20000, 5000, 1)
    assert by_name[b"split"]["change"] == df.diff.MODIFIED and by_name[b"split"]["a"][6] == by_name[b"split"]["b"][6] == 6


def test_damage_is_collected_and_the_walk_goes_on(ctx, df):
    out = walk(ctx, df, "damaged", slots=8)               # diff.trees raises unless the call returns BW_OK
    records, names, _, counts, errors = out["ab"]
    info = built("damaged")[0][4]
    flags = Counter(int(r["flags"]) for r in records)
    assert flags[df.diff.F_UNREADABLE] >= 4 and flags[df.diff.F_TRUNCATED] == 2
    reasons = Counter(int(e["reason"]) for e in errors)
    L = sys.modules["backuwup_amd._lib"]
    assert {L.BW_RESTORE_ENOTFOUND, L.BW_RESTORE_ENOTTREE, L.BW_UNPACK_ETAG, L.BW_RESTORE_EFORMAT} <= set(reasons)
    assert any(bytes(e["hash"]) == info["cyc"] and bytes(e["parent"]) == info["inner"] for e in errors)
    assert counts["n_errors"] == len(errors) > 0


def test_a_chain_that_names_itself_is_refused_unread(ctx, df):
    # the fetch's bounded refusal (round > n_e) with the diff walk's hooks: one EFORMAT error, F_TRUNCATED
    out = walk(ctx, df, "chain_names_itself", which=("ab", "ba"), slots=4)
    hl = built("chain_names_itself")[0][4]["loop"]
    L = sys.modules["backuwup_amd._lib"]
    for w in ("ab", "ba"):
        records, _, _, counts, errors = out[w]
        assert [(bytes(e["hash"]), bytes(e["parent"]), int(e["child_pos"]), int(e["reason"])) for e in errors] == \
            [(hl, hl, NONE, L.BW_RESTORE_EFORMAT)]
        assert Counter(int(r["flags"]) for r in records) == {0: 3, df.diff.F_TRUNCATED: 1}


@pytest.mark.parametrize("seed", [0, 4, 8, 12, 16])
def test_seeded_mutations(ctx, df, seed):
    walk(ctx, df, "mutation", seed, slots=4 if seed % 8 else 16)


@pytest.mark.parametrize("slots", [0, 16])           # 0: the default, a level of hundreds of blobs in one sub-batch
def test_wide_directory_and_a_hash_shared_between_parents(ctx, df, slots):
    out = walk(ctx, df, "wide_and_shared", slots=slots)
    paths = Counter((t[0], t[1]) for t in df.dref.resolve(as_ref_records(*out["ab"][:2])))
    assert paths[(b"/p/q/sub", df.diff.REMOVED)] == 1 and paths[(b"/r/s/sub", df.diff.ADDED)] == 1
    assert paths[(b"/p/q/sub/deeper/in2", df.diff.REMOVED)] == 1 and paths[(b"/r/s/sub/deeper/in2", df.diff.ADDED)] == 1
    assert sum(1 for (p, c) in paths if p.startswith(b"/wide/c") and c == df.diff.MODIFIED) == 150


# ------------------------------------------------------------------ capacity
CANARY = 0xA5


def raw(df, s, ra, rb, record_cap, names_cap, err_cap):
    """bw_diff_trees with exactly these caps and a canary behind each array: (rc, records, names, counts, errors)."""
    L = sys.modules["backuwup_amd._lib"]
    from backuwup_amd.prune import ERROR_DTYPE
    roots = [None if r is None else (ctypes.c_uint8 * 32).from_buffer_copy(bytes(r)) for r in (ra, rb)]
    records = np.full((record_cap + 1) * df.diff.RECORD_DTYPE.itemsize, CANARY, dtype=np.uint8)
    names = np.full(names_cap + 64, CANARY, dtype=np.uint8)
    errs = np.full((err_cap + 1) * ERROR_DTYPE.itemsize, CANARY, dtype=np.uint8)
    read = np.zeros(s.n_entries + 64, dtype=np.uint8)
    read[s.n_entries:] = CANARY
    cnt = L.BwDiffCounts()
    rc = s._L.bw_diff_trees(s.h, roots[0], roots[1], 0, records.ctypes.data_as(ctypes.POINTER(L.BwDiffRecord)), record_cap,
                            names.ctypes.data_as(ctypes.c_void_p), names_cap, read.ctypes.data_as(L.u8p), ctypes.byref(cnt),
                            errs.ctypes.data_as(ctypes.POINTER(L.BwPruneError)), err_cap)
    assert (records[record_cap * df.diff.RECORD_DTYPE.itemsize:] == CANARY).all()
    assert (names[names_cap:] == CANARY).all() and (read[s.n_entries:] == CANARY).all()
    assert (errs[err_cap * ERROR_DTYPE.itemsize:] == CANARY).all()
    counts = {f: int(getattr(cnt, f)) for f in df.diff.COUNT_FIELDS}
    return (rc, records[:record_cap * df.diff.RECORD_DTYPE.itemsize].view(df.diff.RECORD_DTYPE), names[:names_cap], counts,
            errs[:err_cap * ERROR_DTYPE.itemsize].view(ERROR_DTYPE))


def test_caps_one_short_give_enospc_and_write_nothing_past_them(ctx, df):
    L = sys.modules["backuwup_amd._lib"]
    case = built("basic", "swap")[0]
    ra, rb = case[2], case[3]
    with df.restore.Session(ctx, df.PRK, *store_args(ctx, df, case), slots=16) as s:
        records, names, read, counts, errors = df.diff.trees(s, ra, rb)
        need_r, need_n = counts["n_records"], counts["name_bytes"]
        assert need_r == 8 and need_n > 0
        rc, _, _, c1, _ = raw(df, s, ra, rb, need_r - 1, need_n, 4)
        assert rc == L.BW_ENOSPC and c1["n_records"] == need_r and c1["n_levels"] == counts["n_levels"]
        rc, _, _, c2, _ = raw(df, s, ra, rb, need_r, need_n - 1, 4)
        assert rc == L.BW_ENOSPC and c2["name_bytes"] == need_n
        rc, _, _, c3, _ = raw(df, s, ra, rb, 1, need_n, 4)      # the walk stops at the first level that does not fit
        assert rc == L.BW_ENOSPC and 1 < c3["n_records"] < need_r and c3["n_levels"] == 2
        rc, r4, n4, c4, e4 = raw(df, s, ra, rb, need_r, need_n, 4)
        assert rc == L.BW_OK
        compare(df, (r4[:c4["n_records"]], n4[:c4["name_bytes"]].tobytes(), read, c4, e4[:0]), wanted("basic", "swap", "ab"))


def test_more_errors_than_err_cap_is_enospc_with_everything_else_filled(ctx, df):
    L = sys.modules["backuwup_amd._lib"]
    case = built("damaged")[0]
    want = wanted("damaged", None, "ab")
    with df.restore.Session(ctx, df.PRK, *store_args(ctx, df, case), slots=8) as s:
        rc, records, names, counts, errs = raw(df, s, case[2], case[3], 64, 4096, 2)
    assert rc == L.BW_ENOSPC and counts["n_errors"] == sum(want[1].values()) > 2
    got = Counter(df.dref.resolve(as_ref_records(records[:counts["n_records"]], names[:counts["name_bytes"]].tobytes())))
    assert got == want[0] and not as_ref_errors(errs) - want[1]


# ------------------------------------------------------------------ diff.diff beside full_walk_diff
@pytest.mark.parametrize("name,arg", [("basic", "depth4"), ("basic", "rename"), ("basic", "mtime"), ("basic", "swap"),
                                      ("dir_metadata_only", None), ("membership", None), ("duplicates", None),
                                      ("names", None), ("chunk_lists", None), ("mutation", 0), ("mutation", 4),
                                      ("mutation", 8), ("mutation", 12), ("mutation", 16)])
def test_diff_lists_the_paths_full_walk_diff_lists(ctx, df, name, arg):
    case = built(name, arg)[0]
    args = store_args(ctx, df, case)
    changes, errors, counts = df.diff.diff(ctx, *args, df.PRK, case[2], case[3], slots=16)
    full = df.diff.full_walk_diff(ctx, *args, df.PRK, case[2], case[3], slots=16)
    assert len(errors) == 0 and counts["n_records"] == len(changes)
    assert [(c["path"], c["change"]) for c in changes] == [(c["path"], c["change"]) for c in full]
    def whole(c):                                          # records of one path and change come in no fixed order
        return str((c["path"], c["change"], c["a"], c["b"], c["common_prefix"], c["common_suffix"], c["n_new"]))
    assert Counter(map(whole, changes)) == Counter(map(whole, full))


def test_on_chains_the_two_differ_exactly_at_split(ctx, df):
    case = built("chains")[0]
    args = store_args(ctx, df, case)
    changes, errors, _ = df.diff.diff(ctx, *args, df.PRK, case[2], case[3], slots=8)
    full = df.diff.full_walk_diff(ctx, *args, df.PRK, case[2], case[3], slots=8)
    got = [(c["path"], c["change"]) for c in changes]
    assert len(errors) == 0 and ("split", df.diff.MODIFIED) in got
    assert [x for x in got if x[0] != "split"] == [(c["path"], c["change"]) for c in full]
