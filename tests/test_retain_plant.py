"""tests/retain_plant.py on the CPU: the constants read from the sources, the lane of every packfile's first
entry in every geometry, the shape of every mask pattern and drop-set family, the model of k_rt_drop and
its host loop against tests/retain_ref.py's drop on every case tests/test_gpu_retain_planted.py runs, and
the mutants the cases are there to catch; then the same for the mark (the expansion rule against
retain_ref.mark run directly, the staircase's sweeps, the model of seed, propagate and stats, its mutants).

The shapes are conditions on the CASES, not measurements of the kernels: a geometry that stopped putting
a packfile's first entry at lane 1 or lane 63, or a family that stopped filling one batch and beginning a
second, would let the GPU tests pass without testing what they are for, and fails here instead.

Built on the build machine (one core, the oracle's C library): the flat store bytes_bound (4,200 chunks,
14 packfiles) in 0.24 s, cycled_roots(4096) with its reference (ten prune marks, one walk, the expansion)
in 0.21 s, staircase(3) with its reference in 0.17 s; the whole file in 15 s, most of it retain_ref.drop in
Python over the 140 (geometry, pattern, roots) cases the GPU file runs.
"""
import os
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import retain_plant as P  # noqa: E402
import zstd_ref  # noqa: E402

needs_zstd = pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")


def same(a, b):
    return all(x is y or (x.shape == y.shape and (x == y).all()) for x, y in zip(a[:3], b[:3]))


# ------------------------------------------------------------------ the constants
def test_the_constants_are_the_headers():
    assert (P.BATCH_SETS, P.BATCH_BYTES, P.MAX_ROOTS, P.SUMS) == (65535, 1 << 28, 4096, 5)
    assert (P.WORKGROUP, P.WAVE, P.NONCE) == (256, 64, 12)
    from backuwup_amd import retain
    assert P.MAX_ROOTS == retain.MAX_ROOTS and [P.n_words(n) for n in (0, 1, 64, 65, 4096)] == [retain.words(n) for n in (0, 1, 64, 65, 4096)]
    assert [P.per_of(n, e) for n, e in ((13, 900), (65537, 48), (70000, 4200), (5, 0), (3, 1 << 29))] == [13, 65535, 63913, 5, 1]


EDITS = [("bw_retain.h", "RT_DROP_BATCH_SETS = 65535;", "RT_DROP_BATCH_SETS = 0xffff;"),
         ("bw_retain.h", "RT_DROP_BATCH_BYTES = 1ull << 28;", "RT_DROP_BATCH_BYTES = 256ull << 20;"),
         ("bw_retain_host.h", "RT_MAX_ROOTS = 4096;", "RT_MAX_ROOTS = 64 * 64;"),
         ("bw_retain.hip", "RT_DROP_BATCH_BYTES / std::max<uint64_t>(n_e, 1)})", "RT_DROP_BATCH_BYTES / std::max<uint64_t>(n_e * W, 1)})"),
         ("bw_retain.hip", "drop + q0 * W, 8 * m * W,", "drop + q0, 8 * m * W,"),
         ("bw_retain.hip", "hipMemsetAsync(d_stat, 0, freed_at + 32 * per, c->stream)", "hipMemsetAsync(d_stat, 0, freed_at, c->stream)"),
         ("bw_retain.hip", "__launch_bounds__(256) k_rt_drop(", "__launch_bounds__(512) k_rt_drop("),
         ("bw_retain.hip", "for (int d = 32; d; d >>= 1)", "for (int d = 16; d; d >>= 1)"),
         ("bw_retain.hip", "if (__all(!in || p == p0) && __shfl((int)in, 0)) {", "if (__all(!in || p == p0)) {"),
         ("bw_retain.hip", "live[q * n + e] = lv", "live[q * gridDim.x * 256 + e] = lv"),
         ("bw_retain.hip", "1ull << (i & 63)", "1ull << (i % 64)"),
         ("backuwup_gpu_pack.h", "#define BW_BLOB_NONCE_SIZE 12u", "#define BW_BLOB_NONCE_SIZE (4u + 8u)")]


def test_the_constant_reader_reads_the_tree_and_raises_on_an_edited_copy():
    src = P.sources()
    assert P.read_constants(src) == P.C
    for name, old, new in EDITS:
        assert old in src[name], (name, old)
        edited = dict(src)
        edited[name] = src[name].replace(old, new, 1)
        with pytest.raises(RuntimeError, match="retain_plant"):
            P.read_constants(edited)


# ------------------------------------------------------------------ the geometries
def test_every_packfile_begins_at_the_lane_it_is_planted_at():
    lanes = {g: [l for l, _ in P.first_lanes(P.GEOMETRIES[g])] for g in P.GEOMETRIES}
    groups = {g: [w for _, w in P.first_lanes(P.GEOMETRIES[g])] for g in P.GEOMETRIES}
    # lane1: a one-entry packfile in lane 0 and its neighbour from lane 1; a packfile that is exactly one wave, so
    # the next begins at lane 0 of the next wave; 65 entries, so the next begins at lane 1 again; two one-entry
    # packfiles in lanes 0 and 1 of a wave and a third packfile from lane 2; 256 entries that begin mid-workgroup
    # and cross into the next (entries 384 .. 639); 257 entries; 3 entries in a last wave that ends at lane 4
    assert P.first_entries(P.GEOMETRIES["lane1"]) == [0, 1, 64, 128, 193, 320, 321, 322, 384, 640, 897]
    assert lanes["lane1"] == [0, 1, 0, 0, 1, 0, 1, 2, 0, 0, 1] and groups["lane1"] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 3]
    assert P.wave_shapes(P.GEOMETRIES["lane1"]) == (Counter(uniform=11, by_lane=4, idle=1), 4)
    # lane63: boundaries at lane 63 twice, the second packfile one entry long; entry 256 begins a packfile and a workgroup
    assert P.first_entries(P.GEOMETRIES["lane63"]) == [0, 63, 127, 128, 130, 256, 449]
    assert lanes["lane63"] == [0, 63, 63, 0, 2, 0, 1] and groups["lane63"] == [0, 0, 0, 0, 0, 1, 1]
    assert P.wave_shapes(P.GEOMETRIES["lane63"]) == (Counter(uniform=4, by_lane=4), 12)
    # ones: every lane a packfile of its own, 130 of them: two full waves and two lanes of a third
    assert lanes["ones"] == [e % 64 for e in range(130)] and P.wave_shapes(P.GEOMETRIES["ones"]) == (Counter(by_lane=3, idle=1), 2)
    # one: nothing but uniform waves, the last of 44 entries
    assert lanes["one"] == [0] and P.wave_shapes(P.GEOMETRIES["one"]) == (Counter(uniform=5, idle=3), 44)
    # bytes_bound: 300 is no multiple of 64: 13 of its 66 waves hold a boundary
    assert sum(P.GEOMETRIES["bytes_bound"]) == 4200 > 4096 and P.wave_shapes(P.GEOMETRIES["bytes_bound"])[0]["by_lane"] == 13
    assert lanes["sets_bound"] == [0, 33] and sum(P.GEOMETRIES["sets_bound"]) == 48
    # the wave that lies partly past n, in every geometry
    assert all(sum(P.GEOMETRIES[g]) % P.WAVE for g in P.GEOMETRIES)


@needs_zstd
def test_flat_stores_hold_what_the_geometry_says(oracle):
    import prune_ref
    for g in P.GEOMETRIES:
        s = P.flat(g)
        assert [len(h[3]) for h in s["hd"]] == P.GEOMETRIES[g] and s["n_entries"] == sum(P.GEOMETRIES[g])
        ents = prune_ref.flat_entries(s["hd"])
        assert all(e[2] == 0 for e in ents)                       # file chunks: nothing refers to anything
        assert len(set(e[1] for e in ents)) == len(ents)
        assert len(set(s["pf_bytes"])) == len(s["groups"])        # a sum credited to the wrong packfile shows
        assert s["pf_bytes"] == [sum(12 + e[4] for e in ents if e[0] == p) for p in range(len(s["groups"]))]
    assert P.flat("lane1") is P.flat("lane1")


# ------------------------------------------------------------------ the patterns and the families
def test_every_pattern_has_the_shape_it_claims():
    for n in P.ROOT_COUNTS:
        lo, cnt = P.last_word_bits(n)
        assert (lo, cnt) == {1: (0, 1), 64: (0, 64), 65: (64, 1), 4095: (4032, 63), 4096: (4032, 64)}[n]
        f = P.full(n)
        for pat in P.PATTERNS:
            m = P.masks(pat, 900, n)
            assert len(m) == 900 and all(0 <= x <= f for x in m), (pat, n)       # no bit of a root that was not given
            w = P.to_words(m, n)
            assert w.shape == (900, P.n_words(n)) and P.to_ints(w) == m
        assert set(P.masks("empty", 900, n)) == {0} and set(P.masks("full", 900, n)) == {f}
        assert set(P.masks("lone_last", 900, n)) == {1 << (n - 1)}
        assert set(P.masks("last_word", 900, n)) == {f >> lo << lo} and bin(f >> lo).count("1") == cnt
        fl = P.masks("first_and_last_word", 900, n)
        for x in fl:
            assert x & P.M64 and x >> lo and bin(x).count("1") == (2 if n > 64 else bin(x).count("1")) <= 2
        assert len(set(fl)) > min(64, n) // 2                      # it moves with the entry
        r = P.masks("random", 900, n)
        assert 0.2 < sum(1 for x in r if not x) / 900 < 0.3
        if n > 64:                                                # masks with bits in the last word only, and in several
            assert any(x and not x & P.M64 for x in r) and any(x & P.M64 and x >> 64 for x in r)
        o = P.masks("orphan_lane0", 900, n)
        assert [e for e, x in enumerate(o) if not x] == list(range(0, 900, 64)) and all(bin(x).count("1") == 1 for x in o if x)


def test_every_family_has_the_shape_it_claims():
    assert P.BITS_SETS == (65534, 65535, 65536, 65537) and P.BITS_ROOTS == 17
    q = P.bits_of_q(65537)
    assert len(set(q)) == 65537 and max(q) < 1 << 17 and q[65536] == 1 << 16
    assert P.to_ints(P.bits_of_q_words(300)) == q[:300] and (P.bits_of_q_words(65537) == P.to_words(q, 17)).all()
    assert [P.per_of(n, 48) for n in P.BITS_SETS] == [65534, 65535, 65535, 65535]          # one batch, one, two, two
    n_e = sum(P.GEOMETRIES["bytes_bound"])
    n_sets = P.cycle_sets_for(n_e)
    per = P.per_of(n_sets, n_e)
    assert (per, n_sets) == (63913, 63915) == (P.BATCH_BYTES // n_e, P.BATCH_BYTES // n_e + 2) and per % 8 == 1 and per < P.BATCH_SETS
    c = P.cycle(n_sets)
    assert set(c[:8]) == set(range(8)) and c[:3] == [3, 0, 5] and c[per] != c[0] and c[per + 1] != c[1]
    with pytest.raises(RuntimeError, match="retain_plant"):
        P.cycle_sets_for(4096)                                    # the set bound binds there
    with pytest.raises(RuntimeError, match="retain_plant"):
        P.cycle_sets_for(1 << 13)                                 # per a multiple of 8
    w = P.wide(4096)
    ix = P.wide_index(4096)
    assert len(w) == 76 and w[ix["empty"]] == 0 and w[ix["full"]] == P.full(4096)
    assert [w[2 + k] for k in range(64)] == [P.M64 << (64 * k) for k in range(64)]
    assert (ix["word0"], ix["last_word"]) == (2, 65)
    assert w[66] == P.full(4096) ^ (1 << 5) and w[67] == P.full(4096) ^ (1 << 4095)
    assert all(0 < x < P.full(4096) for x in w[68:]) and len(set(w[68:])) == 8
    for n in (1, 64, 65, 193, 4095):
        w, ix = P.wide(n), P.wide_index(n)
        assert len(w) == 12 + P.n_words(n) and all(0 <= x <= P.full(n) for x in w) and w[ix["last_word"]] == P.full(n) >> P.last_word_bits(n)[0] << P.last_word_bits(n)[0]


# ------------------------------------------------------------------ the drop: model = reference, and the mutants
def drop_case(geometry, pattern, n_roots):
    return P.drop_case(geometry, pattern, n_roots)[:5]


@needs_zstd
@pytest.mark.parametrize("geometry", P.WAVE_GEOMETRIES)
def test_model_is_the_reference_on_every_wave_case(oracle, geometry):
    for n in P.ROOT_COUNTS:
        for pat in P.PATTERNS:
            s, m, mw, sets, sw, ref = P.drop_case(geometry, pat, n)
            got = P.model_drop(s, mw, sw)
            assert same(got, ref), (geometry, pat, n)
            assert got[3]["shapes"] == P.wave_shapes(P.GEOMETRIES[geometry])[0] and got[3]["n_batches"] == 1
            assert same(P.reference_drop_np(s, mw, sw), ref), (geometry, pat, n)
            no_live = P.model_drop(s, mw, sw, want_live=False)
            assert no_live[0] is None and same(no_live[1:], ref[1:])


@needs_zstd
def test_the_numpy_restatement_is_retain_ref_on_the_family_of_65537_sets(oracle):
    s, mw, sw, ref = P.sets_bound_case()
    m = P.to_ints(mw)
    assert any(x >> 16 for x in m) and any(not x for x in m) and sw.shape == (65537, 1)
    rows = sorted(set(list(range(40)) + list(range(65500, 65537)) + np.random.default_rng(3).integers(0, 65537, 150).tolist()))
    want = P.reference_drop(s, m, rows)
    assert same([x[rows] for x in ref], want)
    for n_sets in P.BITS_SETS:
        got = P.model_drop(s, mw, sw[:n_sets])
        assert same(got, [x[:n_sets] for x in ref]) and got[3]["n_batches"] == (1 if n_sets <= P.BATCH_SETS else 2)
        assert got[3]["shapes"] == Counter(by_lane=1, idle=3)


@needs_zstd
def test_model_is_the_reference_where_the_byte_bound_binds(oracle):
    s, mw, sw, ref, live16 = P.bytes_bound_case()
    assert sw.shape == (63915, 1) and ref[0] is None and live16.shape == (16, 4200)
    assert len(set(map(bytes, ref[2]))) == 8                      # the eight sets free eight different things
    got = P.model_drop(s, mw, sw, want_live=False)
    assert same(got, ref) and (got[3]["per"], got[3]["n_batches"]) == (63913, 2)
    got = P.model_drop(s, mw, sw[:16])
    assert same(got, (live16, ref[1][:16], ref[2][:16]))


# the case each mutant is shown on: (geometry, pattern, n_roots, sets) -> at least one differs from the reference
def _mutant_cases():
    cases = [(g, pat, n, None) for g in ("lane1", "lane63", "ones") for pat in ("last_word", "lone_last", "random", "orphan_lane0")
             for n in (65, 4096)]
    return cases


@needs_zstd
@pytest.mark.parametrize("mutant", [m for m in P.DROP_MUTANTS if m not in ("batch_set_q", "no_clear")])
def test_each_kernel_mutant_of_the_drop_is_caught(oracle, mutant):
    caught = []
    for g, pat, n, _ in _mutant_cases():
        s, m, mw, sets, sw = drop_case(g, pat, n)
        if mutant == "live_stride_per" and len(sets) == s["n_entries"]:
            continue
        if not same(P.model_drop(s, mw, sw, mutant=mutant), P.reference_drop_np(s, mw, sw)):
            caught.append((g, pat, n))
    assert caught, mutant
    print(mutant, "caught by", len(caught), "of", len(_mutant_cases()), caught[:4])
    # and by the case it is named for
    named = {"live_word0": ("one", "lone_last", 65), "any_word0": ("one", "last_word", 4096), "no_all_equal": ("lane1", "full", 1),
             "orphans_freed": ("one", "orphan_lane0", 64), "no_nonce": ("one", "full", 1), "live_stride_per": ("one", "random", 64)}[mutant]
    s, m, mw, sets, sw = drop_case(*named)
    assert not same(P.model_drop(s, mw, sw, mutant=mutant), P.reference_drop_np(s, mw, sw)), named


@needs_zstd
def test_no_all_equal_is_caught_by_every_geometry_with_a_boundary_and_by_no_other(oracle):
    for g in P.WAVE_GEOMETRIES:
        s, m, mw, sets, sw = drop_case(g, "random", 65)
        assert same(P.model_drop(s, mw, sw, mutant="no_all_equal"), P.reference_drop_np(s, mw, sw)) == (g == "one"), g


@needs_zstd
@pytest.mark.parametrize("mutant", ["batch_set_q", "no_clear", "live_stride_per"])
def test_each_batch_mutant_of_the_drop_is_caught_by_both_batch_cases(oracle, mutant):
    s, mw, sw, ref = P.sets_bound_case()
    if mutant != "live_stride_per":
        for n_sets in P.BITS_SETS:                                # one batch hides these two; a second shows them
            got = P.model_drop(s, mw, sw[:n_sets], mutant=mutant)
            assert same(got, [x[:n_sets] for x in ref]) == (n_sets <= P.BATCH_SETS), (mutant, n_sets)
        b, bw, bs, want, _ = P.bytes_bound_case()
        got = P.model_drop(b, bw, bs, want_live=False, mutant=mutant)
        assert not same(got[1:], want[1:])
        per = got[3]["per"]                                       # the first batch is right, the two sets behind it are not
        assert same([x[:per] for x in got[1:3]], [x[:per] for x in want[1:]])
        assert all((got[i][per:] != want[i][per:]).any() for i in (1, 2))
    else:                                                        # the live rows of 16 sets over 4,200 entries, and of 300 over 48
        b, bw, bs, want, live16 = P.bytes_bound_case()
        assert not same(P.model_drop(b, bw, bs[:16], mutant=mutant), (live16, want[1][:16], want[2][:16]))
        assert not same(P.model_drop(s, mw, sw[:300], mutant=mutant), [x[:300] for x in ref])


# ------------------------------------------------------------------ the mark
def figures(per_root):
    return [tuple(p[f] for f in ("reached_blobs", "reached_bytes", "unique_blobs", "unique_bytes", "n_damaged", "status")) for p in per_root]


@needs_zstd
def test_the_expansion_rule_is_retain_ref_run_on_all_130_roots(oracle):
    import retain_ref
    case, hd, masks, damaged, per_root, errors, info = P.cycled_reference(130)
    store, _ = P._store_of(case)
    m, d, pr, er, inf = retain_ref.mark(store, hd, case["roots"])
    assert masks == m and damaged == d and per_root == pr and errors == er
    assert info == {k: v for k, v in inf.items() if k not in ("walk", "n_sweeps")}
    assert sorted(k[2:] for k in errors) == [(65, 16), (128, 19)] and sum(errors.values()) == 2


@needs_zstd
@pytest.mark.parametrize("n", [130, 193, 4095, 4096])
def test_cycled_roots_lie_where_they_are_planted(oracle, n):
    case, hd, masks, damaged, per_root, errors, info = P.cycled_reference(n)
    which = case["which"]
    assert len(which) == n == len(case["roots"]) and len(set(case["distinct"])) == P.CYCLED_DISTINCT
    assert [(which.index(d), which.count(d)) for d in (0, 1, 2, 3, 4, 5)] == [(0, 1), (63, 1), (64, 1), (n - 1, 1), (65, 1), (n - 2, 1)]
    assert [i for i, d in enumerate(which) if d == 6] == [1, n - 3] and all(which.count(d) > n // 5 for d in (7, 8, 9))
    # unique_* is non-zero in the first and the last word, and nowhere else
    assert [i for i, p in enumerate(per_root) if p["unique_blobs"]] == [0, 63, 64, n - 1]
    assert all(per_root[i]["unique_bytes"] > 12 * per_root[i]["unique_blobs"] for i in (0, 63, 64, n - 1))
    assert (per_root[65]["status"], per_root[65]["reached_blobs"]) == (16, 0)
    assert (per_root[n - 2]["status"], per_root[n - 2]["reached_blobs"]) == (P.ENOTTREE, 1)
    assert {p["status"] for i, p in enumerate(per_root) if i not in (65, n - 2)} == {0}
    # root 6's own blobs: one bit in word 0, one in another word, no more
    own6 = [m for m in masks if m == (1 << 1 | 1 << (n - 3))]
    assert len(own6) == 3 and (n - 3) // 64 > 0 and per_root[1]["unique_blobs"] == 0
    assert all(0 <= m < 1 << n for m in masks) and info["orphan_blobs"] == 0 and not any(damaged)
    assert max(m.bit_length() for m in masks) == n                # the last root's bit is somebody's


@needs_zstd
def test_the_staircase_takes_k_plus_two_reference_sweeps(oracle):
    import retain_ref
    case, hd, masks, damaged, per_root, errors, info = P.staircase_reference(3)
    assert info["n_sweeps"] == 3 + 2 and info["n_levels"] == 5 and not errors
    assert retain_ref.fixed_point(info["walk"])[0] == masks
    # A reaches its own Dir and the staircase; B everything but A's Dir
    assert Counter(masks) == Counter({3: case["n_entries"] - 6, 2: 5, 1: 1})
    assert P.staircase_reference(2)[6]["n_sweeps"] == 4 and P.staircase_reference(4)[6]["n_sweeps"] == 6


def mark_cases():
    out = {}
    for n in (130, 193, 4095, 4096):
        case, hd, masks, _, per_root, _, info = P.cycled_reference(n)
        out["cycled-%d" % n] = (case, hd, masks, per_root, info)
    case, hd, masks, _, per_root, _, info = P.staircase_reference(3)
    out["staircase"] = (case, hd, masks, per_root, info)
    return out


@needs_zstd
def test_the_mark_model_is_the_reference_and_each_mutant_is_caught(oracle):
    cases = mark_cases()
    walks = {}
    for name, (case, hd, masks, per_root, info) in cases.items():
        w, _ = P.walk_of(case)
        walks[name] = w
        m, pr, totals, sweeps = P.model_mark(w, hd, len(case["roots"]))
        assert m == masks and pr == per_root, name
        assert totals == {k: info[k] for k in totals}, name
    assert P.model_mark(walks["staircase"], cases["staircase"][1], 2)[3] == 5
    caught = {}
    for mutant in P.MARK_MUTANTS:
        caught[mutant] = []
        for name, (case, hd, masks, per_root, info) in cases.items():
            m, pr, totals, _ = P.model_mark(walks[name], hd, len(case["roots"]), mutant=mutant, k=3)
            if m != masks or pr != per_root:
                caught[mutant].append(name)
    print(caught)
    assert set(caught["word0_only"]) == {"cycled-130", "cycled-193", "cycled-4095", "cycled-4096"}
    assert set(caught["seed_and_31"]) == {"cycled-130", "cycled-193", "cycled-4095", "cycled-4096"}
    assert set(caught["unique_own_word"]) == {"cycled-130", "cycled-193", "cycled-4095", "cycled-4096"}
    assert caught["k_sweeps"] == ["staircase"] and "staircase" in caught["leaf_first"]
    # unique from the root's own word: masks stay right, root 1's record is what goes wrong
    case, hd, masks, per_root, _ = cases["cycled-4096"]
    m, pr, _, _ = P.model_mark(walks["cycled-4096"], hd, 4096, mutant="unique_own_word")
    assert m == masks and pr[1]["unique_blobs"] == 3 and pr[4093]["unique_blobs"] == 3 and per_root[1]["unique_blobs"] == 0
