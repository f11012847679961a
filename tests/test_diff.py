"""Diff on the CPU: tests/diff_ref.py (the rules of a snapshot diff, stated in Python) pinned by
hand-written expectations for small cases and by an independent check: two restore_ref.unpack listings
compared as path maps give the same added / removed / modified / type-changed path sets."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402

pytestmark = pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")


@pytest.fixture(scope="module")
def df(oracle):
    import diff_ref
    import diff_stores
    import prune_ref
    import restore_ref
    import restore_store

    class NS:
        pass
    ns = NS()
    ns.dref, ns.stores, ns.pref, ns.ref, ns.PRK = diff_ref, diff_stores, prune_ref, restore_ref, restore_store.PRK
    return ns


def run(df, case, swap=False):
    packs, index, ra, rb, info = case
    if swap:
        ra, rb = rb, ra
    store = df.ref.Store(df.PRK, packs, index)
    hd = df.pref.headers_of(df.PRK, packs)
    records, errors, read, levels = df.dref.diff(store, hd, ra, rb)
    return store, hd, records, errors, read, levels


def by_path(df, records):
    out = {}
    for t, r in zip(df.dref.resolve(records), records):
        out.setdefault(t[0].decode("latin-1"), []).append(r)
    return out


def check_listing(df, store, ra, rb, records):
    na, _, ea = df.ref.unpack(store, ra)
    nb, _, eb = df.ref.unpack(store, rb)
    assert not ea and not eb
    assert df.dref.path_sets(records) == df.dref.listing_diff(na, nb)


def test_identical_and_empty_roots(df):
    case = df.stores.basic("depth4")
    packs, index, ra, rb, _ = case
    store = df.ref.Store(df.PRK, packs, index)
    hd = df.pref.headers_of(df.PRK, packs)
    for a, b in ((ra, ra), (None, None)):
        records, errors, read, levels = df.dref.diff(store, hd, a, b)
        assert not records and not errors and not read and levels == 0
    # NULL against B lists all of B; the swap lists it as REMOVED
    nodes, _, _ = df.ref.unpack(store, rb)
    added = df.dref.diff(store, hd, None, rb)[0]
    removed = df.dref.diff(store, hd, rb, None)[0]
    assert len(added) == len(removed) == len(nodes)
    assert {r["change"] for r in added} == {df.dref.ADDED} and {r["change"] for r in removed} == {df.dref.REMOVED}
    assert sorted(p for p in df.dref.path_sets(added)[df.dref.ADDED]) == sorted(n["path"] for n in nodes)
    assert added[0]["parent"] == df.dref.NONE and added[0]["name"] == b""


def test_one_file_changed_at_depth_four(df):
    case = df.stores.basic("depth4")
    store, hd, records, errors, read, levels = run(df, case)
    assert not errors and levels == 5
    got = by_path(df, records)
    assert sorted(got) == ["", "/deep", "/deep/l2", "/deep/l2/l3", "/deep/l2/l3/target"]
    assert all(len(v) == 1 and v[0]["change"] == df.dref.MODIFIED for v in got.values())
    root = got[""][0]
    assert root["a"][6] == root["b"][6] == 16 and root["n_new"] == 1 and root["common_prefix"] + root["common_suffix"] == 15
    assert len(read) == 10                                   # five pieces per side, none of the wide siblings
    assert [r["parent"] for r in records] == [df.dref.NONE, 0, 1, 2, 3]
    check_listing(df, store, case[2], case[3], records)


def test_rename_mtime_and_type_change(df):
    D = df.dref
    case = df.stores.basic("rename")
    store, hd, records, errors, read, levels = run(df, case)
    got = by_path(df, records)
    assert sorted(got) == ["", "/renamed", "/top"] and not errors
    old, new = got["/top"][0], got["/renamed"][0]
    assert (old["change"], new["change"]) == (D.REMOVED, D.ADDED) and old["a"][1:] == new["b"][1:] and old["a"][6] > 0
    check_listing(df, store, case[2], case[3], records)

    case = df.stores.basic("mtime")
    store, hd, records, errors, read, levels = run(df, case)
    got = by_path(df, records)
    assert sorted(got) == ["", "/top"]
    top = got["/top"][0]
    n = top["a"][6]
    assert top["change"] == D.MODIFIED and top["n_new"] == 0 and top["common_prefix"] == n == top["b"][6] and n > 1
    assert top["common_suffix"] == 0 and top["b"][2] == 3 and top["b"][4] == 1700000000 and top["a"][2] == 1
    check_listing(df, store, case[2], case[3], records)

    case = df.stores.basic("swap")
    store, hd, records, errors, read, levels = run(df, case)
    got = by_path(df, records)
    assert sorted(got) == ["", "/meta", "/meta/m1", "/meta/m2", "/swap", "/swap/inner", "/swap/more", "/swap/more/x"]
    assert got["/swap"][0]["change"] == got["/meta"][0]["change"] == D.TYPE_CHANGED
    assert {got[p][0]["change"] for p in ("/swap/inner", "/swap/more", "/swap/more/x")} == {D.ADDED}
    assert {got[p][0]["change"] for p in ("/meta/m1", "/meta/m2")} == {D.REMOVED}
    assert got["/swap"][0]["common_prefix"] == got["/swap"][0]["n_new"] == 0
    check_listing(df, store, case[2], case[3], records)
    # the swap of the snapshots swaps ADDED and REMOVED
    _, _, back, _, read2, _ = run(df, case, swap=True)
    assert D.path_sets(back)[D.ADDED] == D.path_sets(records)[D.REMOVED] and read2 == read


def test_directory_metadata_only(df):
    case = df.stores.dir_metadata_only()
    store, hd, records, errors, read, levels = run(df, case)
    got = by_path(df, records)
    assert sorted(got) == ["", "/d"] and levels == 2 and len(read) == 4
    d = got["/d"][0]
    assert d["change"] == df.dref.MODIFIED and d["n_new"] == 0 and d["common_prefix"] == 5 and d["a"][4] == 1000 and d["b"][4] == 2000


def test_chunk_lists_and_the_suffix_cap(df):
    case = df.stores.chunk_lists()
    store, hd, records, errors, read, levels = run(df, case)
    got = by_path(df, records)
    for name, want in case[4]["want"].items():
        r = got["/" + name][0]
        assert (r["common_prefix"], r["common_suffix"], r["n_new"]) == want, name
    assert len(read) == 2 + 2 * len(case[4]["want"]) and not errors


def test_chains(df):
    case = df.stores.chains()
    store, hd, records, errors, read, levels = run(df, case)
    got = by_path(df, records)
    D = df.dref
    assert sorted(got) == ["", "/big", "/gone", "/gone/extra", "/gone/k0", "/gone/k1", "/grown", "/grown/extra", "/grown/k5", "/split"]
    s = got["/split"][0]
    assert s["change"] == D.MODIFIED and s["a"][6] == s["b"][6] == s["common_prefix"] == 6 and s["n_new"] == 0
    g = got["/grown"][0]
    assert (g["a"][6], g["b"][6], g["common_prefix"], g["common_suffix"], g["n_new"]) == (6, 6, 5, 0, 1)
    big = got["/big"][0]
    assert (big["a"][6], big["common_prefix"], big["common_suffix"], big["n_new"]) == (25001, 20000, 5000, 1)
    assert got["/gone"][0]["change"] == D.REMOVED and got["/gone"][0]["a"][6] == 3 and not errors


def test_duplicates_and_the_representative_rule(df):
    case = df.stores.duplicates()
    store, hd, records, errors, read, levels = run(df, case)
    D = df.dref
    got = by_path(df, records)
    assert sorted((p, len(v)) for p, v in got.items()) == [("", 1), ("/d", 1), ("/d/dup", 4), ("/d/x", 2)]
    dups = got["/d/dup"]
    pair = [r for r in dups if r["change"] == D.MODIFIED]
    assert len(pair) == 1 and pair[0]["a"][0] == case[4]["y1"] and pair[0]["b"][0] == case[4]["z1"]   # the lowest positions
    assert sorted(r["change"] for r in dups) == [D.ADDED, D.REMOVED, D.REMOVED, D.MODIFIED]
    assert [r["change"] for r in got["/d/x"]] == [D.REMOVED, D.REMOVED]
    assert got["/d"][0]["n_new"] == 2 and (got["/d"][0]["a"][6], got["/d"][0]["b"][6]) == (7, 3)


def test_membership_names_and_cross_directory_hashes(df):
    case = df.stores.membership()
    store, hd, records, errors, read, levels = run(df, case)
    D = df.dref
    sets = D.path_sets(records)
    assert {"left/x", "right/old"} <= sets[D.REMOVED] and {"right/x", "left/fresh"} <= sets[D.ADDED]
    for n in df.stores.SIZES:
        assert sum(1 for p in sets[D.MODIFIED] if p.startswith("d%d/" % n)) == n // 2
        assert sum(1 for p in sets[D.ADDED] if p.startswith("d%d/" % n)) == n - n // 2
    check_listing(df, store, case[2], case[3], records)
    case = df.stores.names()
    store, hd, records, errors, read, levels = run(df, case)
    got = by_path(df, records)
    long_ = "x" * 255
    for n in ("", "a", "ab", "abc", long_, long_[:-1] + "y", long_[:-1]):
        assert [r["change"] for r in got["/names/" + n]] == [D.MODIFIED], n
    assert got["/names/abcd"][0]["change"] == D.REMOVED and got["/names/abce"][0]["change"] == D.ADDED
    assert len(records) == 2 + 7 + 3


def test_damage_never_stops_the_walk(df):
    case = df.stores.damaged()
    info = case[4]
    R, D = df.ref, df.dref
    store, hd, records, errors, read, levels = run(df, case)
    reasons = sorted(k[3] for k in errors.elements())
    assert reasons == sorted([R.ENOTFOUND, R.ENOTTREE, R.ETAG, R.EFORMAT, R.EFORMAT, R.ENOTFOUND, R.EFORMAT])
    got = by_path(df, records)
    unreadable = {r["b"][0] for r in records if r["flags"] & D.F_UNREADABLE}
    assert unreadable == {info["absent"], info["chunk"], info["flipped"], info["malformed"]}
    assert got["/trunc"][0]["flags"] == got["/lost"][0]["flags"] == D.F_TRUNCATED and got["/trunc"][0]["b"][6] == 1
    assert "/trunc/good1" in got and "/lost/good2" in got and "/good7" in got          # the siblings are all there
    inner_cyc = got["/cyc/inner/cyc"][0]
    assert inner_cyc["change"] == D.ADDED and inner_cyc["b"][6] == 0 and inner_cyc["flags"] == 0
    assert "/cyc/inner/cyc/inner" not in got and "/cyc/good4" in got and "/cyc/inner/good3" in got
    cyc_err = [k for k in errors if k[0] == info["cyc"]]
    assert cyc_err == [(info["cyc"], info["inner"], 1, R.EFORMAT)]
    # with the digest check the forged blob is refused before anything is believed
    store_v = R.Store(df.PRK, case[0], case[1], verify=True)
    records_v, errors_v, _, _ = D.diff(store_v, hd, case[2], case[3])
    assert any(k[0] == info["cyc"] and k[3] == R.EDIGEST for k in errors_v)
    assert {r["b"][0] for r in records_v if r["flags"] & D.F_UNREADABLE} == unreadable | {info["cyc"]}


def test_a_chain_that_names_itself_is_refused_after_as_many_pieces_as_the_store_has_entries(df):
    import diff_walk_stores
    case = diff_walk_stores.chain_names_itself()
    hl, n_e = case[4]["loop"], case[4]["n_entries"]
    R, D = df.ref, df.dref
    store, hd, records, errors, read, levels = run(df, case)
    assert n_e == 12 == len(df.pref.flat_entries(hd))
    got = by_path(df, records)
    assert sorted(got) == ["", "/after", "/before", "/loop"] and all(len(v) == 1 for v in got.values())
    loop = got["/loop"][0]
    assert loop["change"] == D.MODIFIED and loop["flags"] == D.F_TRUNCATED and loop["b"][0] == hl
    assert loop["a"][6] == 1 and loop["b"][6] == n_e + 1            # pieces 0 .. n_e were read, one row each
    assert (loop["common_prefix"], loop["n_new"]) == (1, 0)
    assert dict(errors) == {(hl, hl, D.NONE, R.EFORMAT): 1}
    for name in ("/before", "/after"):                              # the sound siblings are unaffected
        r = got[name][0]
        assert r["change"] == D.MODIFIED and r["flags"] == 0 and (r["a"][4], r["b"][4]) == (1000, 2000) and r["n_new"] == 0
    assert got[""][0]["flags"] == 0 and levels == 2
    # the other way round the looping side is A
    _, _, back, errors_back, read_back, _ = run(df, case, swap=True)
    loop = by_path(df, back)["/loop"][0]
    assert loop["flags"] == D.F_TRUNCATED and loop["a"][6] == n_e + 1 and loop["b"][6] == 1
    assert errors_back == errors and read_back == read


@pytest.mark.parametrize("seed", range(20))
def test_seeded_mutations_agree_with_two_listings(df, seed):
    case = df.stores.mutation(seed)
    store, hd, records, errors, read, levels = run(df, case)
    assert not errors and records, case[4]["ops"]
    check_listing(df, store, case[2], case[3], records)
    for k, r in enumerate(records):
        assert r["parent"] == df.dref.NONE or r["parent"] < k
