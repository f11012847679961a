"""tests/table_plant.py on the CPU: the inverted mix, the constants read from the sources, the planters
(every home recomputed here from the bytes), the shape of every case's tables as the model lays them
out, each case's answer by construction against the references and the model, and the mutants every
case is there to catch.

The shapes are conditions on the CASES, not measurements of the kernels: a case that stopped producing
a run across the table's end or a shared home (after a change of a hash or of a capacity rule) would let
tests/test_gpu_tables_planted.py pass without testing what it is for, and fails here instead.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import table_plant as P  # noqa: E402
import zstd_ref  # noqa: E402

needs_zstd = pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")
ALL = tuple(P.CASES)


@pytest.fixture(scope="module")
def built(oracle):
    """Every case and its model, built once."""
    return {name: (P.case(name),) + P.model(name) for name in ALL}


# ------------------------------------------------------------------ the hashes
def test_mix_inverse_and_key8():
    rng = np.random.default_rng(1)
    for h in [0, P.M64] + [int(x) for x in rng.integers(0, 1 << 64, 500, dtype=np.uint64)]:
        assert P.mix64(P.mix64_inv(h)) == h and P.mix64_inv(P.mix64(h)) == h
        home, hi, salt = h & P.M32, h >> 32, (h >> 7) & P.M32
        k = P.key8(home, salt, hi)
        assert len(k) == 8
        # recomputed from the bytes, little-endian, the salt above bit 32: rs_mix(rs_load8(key) ^ salt << 32)
        x = sum(b << (8 * i) for i, b in enumerate(k)) ^ (salt << 32)
        x ^= x >> 33
        x = x * 0xff51afd7ed558ccd & P.M64
        x ^= x >> 33
        assert x == h and x & P.M32 == home
        d = P.digest(h, bytes(range(24)))
        assert len(d) == 32 and d[8:] == bytes(range(24)) and P.mix64(int.from_bytes(d[:8], "little")) == h
    for bits in range(4, 21):          # all ones in the low bits: the last slot at every capacity
        assert P.key_home(P.key8(P.M32)) & ((1 << bits) - 1) == (1 << bits) - 1


def test_the_constants_are_the_public_ones():
    """A regular expression that picked up the wrong numbers would still invert itself: the mix is
    MurmurHash3's first finalizer round, the name hash FNV-1a, whose value of "a" is public."""
    assert (P.SHIFT, P.MUL, P.EMPTY) == (33, 0xff51afd7ed558ccd, 0xffffffff)
    assert P.fnv(0, b"") == 0xcbf29ce484222325 and P.fnv(0, b"a") == 0xaf63dc4c8601ec8c
    assert P.df_seed(0, 0) == 0 and P.df_seed(0, 1) == 1 and P.pm_seed(0) == 0
    assert P.df_seed(1, 0) == 0x9e3779b97f4a7c15 == P.pm_seed(1)
    assert [P.pow2_cap(n) for n in (0, 8, 9, 24, 300, 512, 513)] == [16, 16, 32, 64, 1024, 1024, 2048]
    assert [P.df_table_cap(n) for n in (0, 30, 32, 33, 300, 600)] == [64, 64, 64, 128, 1024, 2048]
    assert P.row_home(bytes(32), 0) == 0 and P.row_home(bytes(32), 3) == P.rs_mix(3 << 32 | 3)


EDITS = [("bw_restore.h", "x ^= x >> 33;\n    x *=", "x ^= x >> 31;\n    x *="),            # one shift of the mix
         ("bw_restore.h", "0xff51afd7ed558ccdull", "0xff51afd7ed558ccfull * 3"),
         ("bw_restore.h", "(uint64_t)p[i] << (8 * i)", "(uint64_t)p[i] << (8 * (7 - i))"),      # the byte order
         ("bw_restore.h", "^ ((uint64_t)salt << 32))", "^ salt)"),
         ("bw_restore.h", "RS_EMPTY = 0xffffffffu", "RS_EMPTY = 0u"),
         ("bw_restore.h", "(h + probe) & (cap - 1)", "(h + 2 * probe) & (cap - 1)"),
         ("bw_walk.h", "0xcbf29ce484222325ull ^ seed", "0xcbf29ce484222325ull + seed"),
         ("bw_walk.h", "(h ^ p[i]) * 0x100000001b3ull", "(h * 0x100000001b3ull) ^ p[i]"),
         ("bw_walk.h", "return rs_mix(h);", "return (uint32_t)h;"),
         ("bw_diff.hip", "(n.parent * 0x9e3779b97f4a7c15ull) ^ side", "(n.parent * 0x9e3779b97f4a7c15ull) + side"),
         ("bw_diff.hip", "^ ((uint64_t)node << 32) ^ node)", "^ ((uint64_t)node << 32))"),
         ("bw_parent.hip", "item * 0x9e3779b97f4a7c15ull", "(item + 1) * 0x9e3779b97f4a7c15ull"),
         ("bw_restore.hip", "while (c < 2 * n) c <<= 1;", "while (c < 4 * n) c <<= 1;"),
         ("bw_restore.hip", "uint64_t c = 16;", "uint64_t c = n;"),
         ("bw_diff_host.h", "while (cap < 2 * n &&", "while (cap < n &&"),
         ("bw_parent_host.h", "return df_table_cap(n);", "return df_table_cap(2 * n);")]


def test_the_constant_reader_reads_the_tree_and_raises_on_an_edited_copy():
    src = P.sources()
    assert P.read_constants(src) == P.C
    for name, old, new in EDITS:
        assert old in src[name], (name, old)
        edited = dict(src)
        edited[name] = src[name].replace(old, new, 1)
        with pytest.raises(RuntimeError, match="table_plant"):
            P.read_constants(edited)


def test_the_name_search_hits_its_homes_and_gives_up():
    sa, sb = P.df_seed(0, 0), P.df_seed(0, 1)
    names = P.names_with_home((sa, sb), 64, ({5, 6}, {63}), 3)
    assert len(set(names)) == 3
    for n in names:
        n.decode("ascii")
        h = 0xcbf29ce484222325          # FNV-1a by hand, then the mix
        for b in n:
            h = (h ^ b) * 0x100000001b3 & P.M64
        assert P.rs_mix(h) & 63 in {5, 6} and P.name_home(sb, n) & 63 == 63
    assert P.name_with_home(sa, 64, {5, 6}, taken=names[:1]) != names[0]
    with pytest.raises(RuntimeError, match="table_plant"):
        P.names_with_home(sa, 64, set(), 1)            # no home at all: the whole bounded search, then it raises


# ------------------------------------------------------------------ the planters hit what they aim at
def test_locator_homes(built):
    c = built["wrap"][0]
    assert {P.key_home(h) & 63 for h, _ in c["index"]} == {62, 63} and {P.key_home(h, p) & 63 for p, h in c["entries"]} == {62, 63}
    assert [P.key_home(q) & 63 for q in c["queries"][24:]] == [61, 63, 0]
    c = built["same_eight"][0]
    heads = [q[:8] for q in c["queries"]]
    assert heads.count(heads[3]) == 9 and len(set(c["queries"])) == len(c["queries"])
    c = built["salted"][0]
    h, g = c["queries"][:2]
    assert {P.key_home(x, p) & 15 for x in (h, g) for p in P.SALTED_POS} == {9}
    assert [e for e in c["entries"] if e[1] == h] == [(0, h), (6, h)] and [e for e in c["entries"] if e[1] == g] == [(0, g)]
    assert dict(c["index"])[h] == dict(c["index"])[g] == c["packs"][6][0]
    c = built["duplicates_behind_a_run"][0]
    d = c["queries"][0]
    assert [k for k, e in enumerate(c["entries"]) if e[1] == d] == list(range(P.DUP_FIRST, P.DUP_FIRST + P.DUP_N))
    assert sum(1 for p, x in set(c["entries"]) if P.key_home(x) & 255 == 200) == 11 and P.DUP_N > 64
    c = built["ids"][0]
    ids = [p[0] for p in c["packs"]]
    assert len({i[:8] for i in ids}) == 1 and len({i[8:] for i in ids}) == 6 and {P.key_home(i) & 15 for i in ids} == {15}
    c = built["crowd"][0]
    assert {P.key_home(q) & 1023 for q in c["queries"]} == {924} and len(set(c["queries"])) == 2 * P.CROWD


def test_walk_homes(built):
    sa, sb = P.df_seed(0, 0), P.df_seed(0, 1)
    for name, homes, cap in (("names_wrap", P.END3, 64), ("names_crowd", {1848}, 2048)):
        c = built[name][0]
        assert len(c["level1"]) == c["facts"]["n_level1"] and P.df_table_cap(len(c["level1"])) == cap
        assert {P.name_home((sa, sb)[s], n) & (cap - 1) for s, _, n, _, _ in c["level1"]} <= homes
        on_both = {n for s, _, n, _, _ in c["level1"] if s == 0} & {n for s, _, n, _, _ in c["level1"] if s == 1}
        assert all(P.name_home(sa, n) & (cap - 1) in homes and P.name_home(sb, n) & (cap - 1) in homes for n in on_both)
        assert len(on_both) == (8 if name == "names_wrap" else 4)
    assert sorted(k for _, k, _, _ in built["names_wrap"][0]["want"]) == [P.ADDED] * 7 + [P.REMOVED] * 7 + [P.MODIFIED] * 7 + [P.TYPE_CHANGED]
    c = built["dup_names"][0]
    n, first = c["facts"]["dup"]
    assert [pos for s, pos, x, _, _ in c["level1"] if s == 0 and x == n] == [3, 7, 9] and first == 3
    assert sum(1 for s, _, x, _, _ in c["level1"] if s == 0 and P.name_home(sa, x) & 63 == 40) == 10
    (e0, e1), (p0, p1), (y0, y1) = built["near_names"][0]["facts"]["pairs"]
    assert e0 == b"" and p1[:-1] == p0 and len(y0) == len(y1) and y0[:-1] == y1[:-1] and y0 != y1
    assert len({e0, e1, p0, p1, y0, y1}) == 6
    for a, b in ((e0, e1), (p0, p1), (y0, y1)):
        assert P.name_home(sa, a) & 63 == P.name_home(sa, b) & 63
    c = built["rows_same_eight"][0]
    (_, ra), (_, rb) = c["rows"]
    assert len({r[:8] for r in ra + rb}) == 1 and len(set(ra)) == 40 and len(set(rb)) == 40 and len(set(ra) & set(rb)) == 20
    c = built["root_rows_wrap"][0]
    (_, ra), (_, rb) = c["rows"]
    both = set(ra) & set(rb)
    assert len(both) == 6 and len(ra) == len(rb) == 12
    assert {P.row_home(r, 0) & 63 for r in ra} <= P.ROOT_END and {P.row_home(r, 1) & 63 for r in set(rb) - both} <= P.ROOT_END
    assert {P.row_home(r, 1) & 63 for r in both} <= P.ROOT_START
    s0 = P.pm_seed(0)
    for name, homes, cap in (("pm_wrap", {62, 63}, 64), ("pm_dup", {30}, 64), ("pm_crowd", {924}, 1024)):
        c = built[name][0]
        assert P.pm_table_cap(len(c["kids"])) == cap
        asked = [sn["name"] for sn in c["scan"][1:]]
        assert {P.name_home(s0, n) & (cap - 1) for n in asked + [k[0] for k in c["kids"]]} <= homes
    c = built["pm_dup"][0]
    assert [pos for pos, (n, _) in enumerate(c["kids"]) if n == c["facts"]["dup"][0]] == [2, 5, 7]
    assert built["pm_wrap"][0]["want"].count(None) == 6 and built["pm_crowd"][0]["want"].count(None) == 20


# per case and table: (capacity, the longest run of occupied slots, a run crosses the end, the longest probe)
SHAPES = {
    "wrap": dict(items=(64, 24, True, 24), entries=(64, 24, True, 23)),
    "same_eight": dict(items=(32, 13, False, 14), entries=(32, 13, False, 11)),
    "salted": dict(entries=(16, 5, False, 5)),
    "duplicates_behind_a_run": dict(entries=(256, 12, False, 12)),
    "ids": dict(ids=(16, 6, True, 7)),
    "crowd": dict(items=(1024, 300, True, 301), entries=(1024, 300, True, 300)),
    "names_wrap": dict(names=(64, 30, True, 29)),
    "names_crowd": dict(names=(2048, 600, True, 600)),
    "dup_names": dict(names=(64, 9, False, 9)),
    "near_names": dict(names=(64, None, False, 2)),
    "rows_same_eight": dict(rows=(256, 40, False, 41)),
    "root_rows_wrap": dict(rows=(64, 24, True, 22)),
    "pm_wrap": dict(names=(64, 12, True, 13)),
    "pm_dup": dict(names=(64, 6, False, 6)),
    "pm_crowd": dict(names=(1024, 300, True, 301)),
}


@pytest.mark.parametrize("name", ALL)
def test_the_model_shows_the_shape_the_case_is_for(built, name):
    c, _, tables = built[name]
    shape = P.shape(tables)
    for table, (cap, run, wraps, probe) in SHAPES[name].items():
        s = shape[table]
        assert (s["cap"], s["wraps"], s["longest_probe"]) == (cap, wraps, probe), (table, s)
        assert run is None or s["run"] == run, (table, s)
        assert tables[table].crossed == wraps and tables[table].lost == 0
    assert set(c["facts"].get("wraps", ())) == {t for t, v in SHAPES[name].items() if v[2]}
    # insertion order does not move the occupied set
    if c["kind"] == "locate":
        ids = [p[0] for p in c["packs"]]
        rec = [(P.key_home(h, p), (p, h, False), k) for k, (p, h) in enumerate(c["entries"])]
        fwd, rev = P.Table(P.pow2_cap(len(rec))).build(rec), P.Table(P.pow2_cap(len(rec)), reverse=True).build(rec)
        assert fwd.occupied() == rev.occupied() == tables["entries"].occupied() and len(ids) == len(tables["ids"].occupied())


# ------------------------------------------------------------------ construction, reference and model agree
@pytest.mark.parametrize("name", ALL)
def test_the_model_agrees_with_the_construction(built, name):
    assert built[name][1] == P.constructed(name)


@needs_zstd
@pytest.mark.parametrize("name", P.LOCATE)
def test_locator_cases_against_the_reference(built, name):
    import prune_ref
    c = built[name][0]
    assert P.reference_locate(c) == c["want"]
    assert [(e[0], e[1]) for e in prune_ref.flat_entries(prune_ref.headers_of(P.PRK, c["packs"]))] == c["entries"]
    assert {st for st, _ in c["want"]} >= {P.OK}


@needs_zstd
@pytest.mark.parametrize("name", P.DIFF)
def test_diff_cases_against_the_reference(built, name):
    c = built[name][0]
    records, errors, read, levels = P.reference_diff(c)
    assert not errors and levels == 2 and P.level1_records(records) == c["want"]
    assert records[0]["parent"] == P.NONE and all(r["parent"] == 0 for r in records[1:])
    assert len(records) == 1 + sum(c["want"].values())
    if "file_want" in c:
        f, w = records[1], c["file_want"]
        assert (f["n_new"], f["common_prefix"], f["common_suffix"], f["a"][6], f["b"][6]) == \
            (w["n_new"], w["common_prefix"], w["common_suffix"], w["n_a"], w["n_b"])


@needs_zstd
@pytest.mark.parametrize("name", P.PARENT)
def test_parent_cases_against_the_reference(built, name):
    c = built[name][0]
    res, errors, read, levels, n_unch, _ = P.reference_parent(c)
    assert not errors and levels == 1 and res[0] == (4, c["root"])          # the seed: Dir against Dir, the one item
    assert [None if h == P.ZERO else h for _, h in res[1:]] == c["want"]
    assert [st for st, _ in res[1:]] == c["status"] and n_unch == c["status"].count(P.PM_UNCHANGED)


# ------------------------------------------------------------------ discrimination
# which cases catch which mutant: the model with the flag set answers otherwise than the construction
CATCHES = {
    "no_wrap": ("wrap", "ids", "crowd", "names_wrap", "names_crowd", "root_rows_wrap", "pm_wrap", "pm_crowd"),
    "home_only": ALL,
    "eq8": ("same_eight", "ids", "rows_same_eight"),
    "len_only": ("names_wrap", "names_crowd", "dup_names", "near_names", "pm_wrap", "pm_dup", "pm_crowd"),
    "no_salt": ("salted", "names_wrap", "names_crowd", "dup_names", "root_rows_wrap"),
    "first_wins": ("duplicates_behind_a_run", "dup_names", "pm_dup"),
}


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_every_mutant_is_caught_by_the_cases_named_for_it(built, mutant):
    assert set(CATCHES) == set(P.MUTANTS) and CATCHES[mutant]
    for name in CATCHES[mutant]:
        assert P.model(name, mutant)[0] != P.constructed(name), (mutant, name)

