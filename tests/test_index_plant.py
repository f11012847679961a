"""tests/index_plant.py on the CPU: the inverted slot hash, the capacity rule, the model against the
plain duplicate rule (and the CPU oracle's BlobIndex) on every planted case, the census conditions
the GPU test rests on, and the mutants every case is there to catch.

The census figures are conditions on the CASES, not measurements of the kernel: a case that stopped
producing equal-tag probes, wraps or growths (after a change of the hash or of the growth rule) would
let tests/test_gpu_index_planted.py pass without testing what it is for, and fails here instead.
"""
import numpy as np
import pytest

import index_plant as P

CASE_NAMES = tuple(P.CASES)


@pytest.fixture(scope="module")
def models():
    """Every case through the model once, claims in canonical order."""
    return {name: P.run_model(P.case(name)) for name in CASE_NAMES}


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------ the hash

def test_fmix64_inverse():
    rng = np.random.default_rng(1)
    values = [0, P.M64] + [int(x) for x in rng.integers(0, 1 << 64, 1000, dtype=np.uint64)]
    for h in values:
        assert P.fmix64(P.fmix64_inv(h)) == h
        assert P.fmix64_inv(P.fmix64(h)) == h
    assert [int(x) for x in P.fmix64_np(np.array(values, dtype=np.uint64))] == [P.fmix64(h) for h in values]


def test_fmix64_is_murmur3_finalizer():
    """The constants read out of bw_dedup.hip are MurmurHash3's 64-bit finalizer's, whose value at 1
    is public (a regular expression that picked up the wrong numbers would still invert itself)."""
    assert (P.SHIFT, P.MUL1, P.MUL2) == (33, 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53)
    assert P.fmix64(0) == 0 and P.fmix64(1) == 0xb456bcfc34c2cb2c


def test_digest_round_trips_through_the_model_hash():
    rng = np.random.default_rng(2)
    tail = bytes(range(24))
    for h in [0, P.M64, P.slot_hash(P.LAST, 0), P.slot_hash(P.LAST, P.TAG_MAX, 0xFFFFF)] + \
            [int(x) for x in rng.integers(0, 1 << 64, 200, dtype=np.uint64)]:
        d = P.digest(h, tail)
        assert len(d) == 32 and d[8:] == tail
        assert P.hash_of(d) == h
        assert P.hashes(np.frombuffer(d, dtype=np.uint8)) == [h]
        assert int.from_bytes(d[:8], "little") == P.fmix64_inv(h)  # little-endian, as dig_hash reads it
    h = P.slot_hash(P.LAST, 0x123456, 0x54321)
    for bits in range(16, 21):  # the last slot at every capacity up to 2^20
        assert h & ((1 << bits) - 1) == (1 << bits) - 1
    assert h >> P.SEQ_BITS == 0x123456


def test_members_are_distinct_and_differ_in_one_byte():
    rows = [P.member(P.H_CT, P.T_CT, k) for k in range(-1, 24 * 255)]
    assert len(set(rows)) == len(rows)
    base = rows[0]
    for k in range(24):
        d = rows[1 + k]
        assert [i for i in range(32) if d[i] != base[i]] == [8 + k]
    assert len({x.tobytes() for x in P.decoys()}) == len(P.decoys())


# ------------------------------------------------------------------ the capacity rule

def test_capacity_rule():
    K = 1 << 10
    assert (P.TABLE_CAP0, P.LOG_CAP0) == (64 * K, 64 * K)
    # by hand: the table doubles when 2 x (log + incoming) passes it, the log when log + incoming does
    assert P.capacity_after([32768]) == [(64 * K, 64 * K)]          # 2 x 32768 == 65536: not yet
    assert P.capacity_after([32769]) == [(128 * K, 64 * K)]
    assert P.capacity_after([9000] * 8) == [(64 * K, 64 * K)] * 3 + [(128 * K, 64 * K)] * 4 + [(256 * K, 128 * K)]
    #                                       27000                  36000 .. 63000            72000
    assert P.capacity_after([65536, 1]) == [(128 * K, 64 * K), (256 * K, 128 * K)]
    assert P.capacity_after([1, 200000]) == [(64 * K, 64 * K), (512 * K, 256 * K)]  # doubled until it fits
    # a pre-sized index: bw_index_reset(200000) takes 2^18 log entries and 2^19 slots, and stays
    assert P.capacity_after([9000] * 20, reset_hint=200000) == [(512 * K, 256 * K)] * 20
    # bounds above the appended count (exchange buckets): with a read after every call the bound is
    # the length again, 3 x 9000 + 11400 passes 32768 ...
    assert P.capacity_after([(11400, 9000)] * 4) == [(64 * K, 64 * K)] * 3 + [(128 * K, 64 * K)]
    # ... and without reads the bounds add up (22800 + 11400 passes it a call earlier), but the
    # growth check reads the length first: 18000 + 11400 does not
    assert P.capacity_after([(11400, 9000)] * 4, read=False) == [(64 * K, 64 * K)] * 3 + [(128 * K, 64 * K)]
    assert P.capacity_after([(16000, 100)] * 5, read=False) == [(64 * K, 64 * K)] * 5
    c = P.Capacity()
    assert [c.gate(9000) for _ in range(8)] == [False] * 3 + [True] + [False] * 3 + [True]


def test_capacity_of_the_gpu_test_layouts():
    """Every layout tests/test_gpu_index_planted.py gives `grow` crosses exactly two growths, and the
    pre-sized run none."""
    _, batches = P.case("grow")
    sizes = [len(b) for b in batches]
    for bounds in [sizes] + [[(P.bucket_layout(n, n_src)[2], n) for n in sizes] for n_src in (1, 8)]:
        caps = [P.TABLE_CAP0] + [t for t, _ in P.capacity_after(bounds)]
        assert sorted(set(caps)) == [1 << 16, 1 << 17, 1 << 18], bounds[:3]
        assert P.capacity_after(bounds)[-1][1] == 1 << 17
        assert len(set(P.capacity_after(bounds, reset_hint=P.PRESIZE))) == 1


# ------------------------------------------------------------------ model against reference

@pytest.mark.parametrize("name", CASE_NAMES)
def test_model_matches_reference(models, oracle, name):
    seed, batches = P.case(name)
    want_v, want_n = P.expected(name)
    got_v, got_n, m = models[name]
    assert same(got_v, want_v)
    assert list(got_n) == list(want_n)
    assert not m.lost
    assert same(P.reference_oracle(oracle, batches, seed), want_v)
    assert all(0 < v.sum() < len(v) or name == "grow" for v in want_v)  # both verdicts in every batch
    assert sum(int(v.sum()) for v in want_v) > 0


@pytest.mark.parametrize("name", ["cluster_tail", "tags", "wrap", "contend", "seeded"])
def test_model_verdicts_do_not_depend_on_the_claim_order(name):
    """The kernel's claims run in any order; the minimum in the slot makes the first occurrence win."""
    got_v, got_n, m = P.run_model(P.case(name), order="reverse")
    want_v, want_n = P.expected(name)
    assert same(got_v, want_v) and list(got_n) == list(want_n) and not m.lost


# ------------------------------------------------------------------ census conditions

@pytest.mark.parametrize("name", [n for n in CASE_NAMES if n != "contend"])
def test_census_equal_tag_different_digest(models, name):
    assert P.total(models[name][2].census)["tag_eq_dig_ne"] >= 100


@pytest.mark.parametrize("name", ["wrap", "cluster_tail"])
def test_census_wraps(models, name):
    assert P.total(models[name][2].census)["wraps"] >= 10


def test_census_wrap_pushes_the_second_cluster(models):
    """The last-slot cluster spills over slot 3, the home of the second one."""
    m = models["wrap"][2]
    w1, w2, _ = P._wrap_rows()
    cap = len(m.table)
    assert set(m.homes(P.as_array(w1))) == {cap - 1} and set(m.homes(P.as_array(w2))) == {3}
    assert len(w1) == 40 and all(m.table[s] != P.EMPTY for s in [cap - 1] + list(range(0, 50)))
    assert m.census[0]["tag_ne"] > 0 and m.census[0]["longest_run"] > len(w1)


def test_census_tags(models):
    m = models["tags"][2]
    assert [c["zero_words"] for c in m.census] == [1, 1]       # tag 0 at log position 0, and only there
    assert all(c["tag_max_slots"] >= 1 for c in m.census)
    seed, batches = P.case("tags")
    assert seed is None and P.hash_of(batches[0][0].tobytes()) >> P.SEQ_BITS == 0
    assert {h >> P.SEQ_BITS for h in P.hashes(batches[0])} == set(P.TAGS) and len(set(P.TAGS)) == 8
    assert {0, P.TAG_MAX} <= set(P.TAGS)
    assert P.TAG_MAX << P.SEQ_BITS | P.SEQ_MASK == P.EMPTY     # one position away from the empty word
    for h in P.H_TAGS:  # each hash with siblings that differ in the tail only
        assert sum(1 for x in P.hashes(batches[0][:32]) if x == h) == 4


def test_census_cluster_tail(models):
    m = models["cluster_tail"][2]
    assert m.census[1]["from_batch"] >= 8 and m.census[1]["from_log"] >= 24
    seed, batches = P.case("cluster_tail")
    first = batches[0][:24]
    assert set(P.hashes(batches[0])) | set(P.hashes(batches[1])) == {P.H_CT}
    differ = {tuple(np.flatnonzero(first[j] != first[k])) for j in range(24) for k in range(j)}
    assert all(len(d) == 2 and min(d) >= 8 for d in differ)  # one byte each off the base tail
    assert any(min(d) >= 28 for d in differ) and any(max(d) == 31 for d in differ)


def test_census_ignored_bits(models):
    a, b, _ = P._ib_rows()
    ha, hb = P.hashes(P.as_array(a)), P.hashes(P.as_array(b))
    assert len(set(ha)) == 16 and len({h & ~(0xFFFFF << 20) for h in ha}) == 1   # bits 20..39 only
    assert len(set(hb)) == 16 and len({h & ~(0xF << 16) for h in hb}) == 1       # bits 16..19 only
    assert len({x[8:] for x in a + b}) == 1 and len({x[:8] for x in a + b}) == 32  # the prefixes differ, not the tails
    m = models["ignored_bits"][2]
    assert len(set(m.homes(P.as_array(a)))) == 1 and len(set(m.homes(P.as_array(b)))) == 1
    for bits in range(16, 21):
        assert len(set(m.homes(P.as_array(a), 1 << bits))) == 1
        assert len(set(m.homes(P.as_array(b), 1 << bits))) == 1 << (bits - 16)


def test_census_grow(models):
    """Two growths.  A growth comes with the call whose bound passes half the table, so the first
    re-claims what the log held below 32 768 entries and the second below 65 536; each re-claims
    more than that limit less one filler batch, i.e. the table was as full as the rule lets it get."""
    m = models["grow"][2]
    assert [g["table_cap"] for g in m.growths] == [1 << 17, 1 << 18]
    assert m.cap.log_cap == 1 << 17  # the log was reallocated and copied
    for g, limit in zip(m.growths, (32768, 65536)):
        assert limit - P.GROW_FILLER < g["entries"] <= limit
        assert g["tag_eq_dig_ne"] >= 100 and g["wraps"] >= 10  # the rebuild meets the planted clusters again
    assert len(m.log) > 65536 + P.GROW_FILLER // 2 and len(m.log) < 80000
    _, b, _ = P._ib_rows()
    assert [len(set(m.homes(P.as_array(b), c))) for c in (1 << 16, 1 << 17, 1 << 18, 1 << 20)] == [1, 2, 4, 16]
    assert len(m.table) == 1 << 18
    # a probe batch right behind each growth: every planted digest a duplicate, the new members new
    _, batches = P.case("grow")
    want_v, _ = P.expected("grow")
    probes = [i for i, x in enumerate(batches) if 6 <= i and len(x) != P.GROW_FILLER]
    assert len(probes) == 2 and [m.census[i - 1]["table_cap"] for i in probes] == [1 << 17, 1 << 18]
    for r, i in enumerate(probes):
        assert m.census[i - 2]["table_cap"] < m.census[i - 1]["table_cap"]
        new = set(P._grow_new(r))
        rows = [x.tobytes() for x in batches[i]]
        assert sum(1 for k, x in enumerate(rows) if not want_v[i][k]) == len(new) == 5
        assert {x for k, x in enumerate(rows) if not want_v[i][k]} == new
        assert len(rows) > 100 + P.GROW_TAIL * 3 * (r + 1)  # the tails of the three fillers before each growth


def test_census_contend(models):
    seed, (d,) = P.case("contend")
    assert len(d) == P.CONTEND_N
    keys, first, counts = np.unique(d, axis=0, return_index=True, return_counts=True)
    hot = counts >= 250
    assert hot.sum() >= 50
    assert (first[hot] < 256).sum() >= 20 and (first[hot] >= 10 * 256).sum() >= 20  # block 0, and late blocks
    shared = [k for k in np.flatnonzero(hot) if P.hash_of(keys[k].tobytes()) == P.H_HOT]
    assert len(shared) == P.CONTEND_SHARED
    assert min(first[shared]) < 256 and max(first[shared]) >= 10 * 256
    assert (counts == 1).sum() > 4000


def test_census_seeded(models):
    seed, batches = P.case("seeded")
    rows = [x.tobytes() for x in seed]
    assert rows == sorted(rows) and len(set(rows)) == len(rows) == 24 + 32
    m = models["seeded"][2]
    assert len(m.census) == 3 and m.census[0]["n"] == len(rows)
    assert all(c["from_log"] >= len(rows) for c in m.census[1:])


# ------------------------------------------------------------------ mutants

# mutant -> (claim order, the cases that must catch it).  from_log reads log entries that the
# running launch has not written: only claims out of canonical order see the difference (a repeat
# that claims before its first occurrence), so it is judged with the claims reversed.
CAUGHT_BY = {
    "eq28": ("forward", ("cluster_tail", "tags", "seeded")),
    "eq8": ("forward", ("cluster_tail", "tags", "wrap", "contend")),
    "tag_only": ("forward", ("ignored_bits",)),
    "from_log": ("reverse", ("contend", "cluster_tail")),
    "from_batch": ("forward", ("cluster_tail", "seeded")),
    "no_min": ("forward", ("contend", "tags")),
    "rehash_unique": ("forward", ("grow",)),
    "rehash_old_mask": ("forward", ("grow",)),
}


def test_every_mutant_is_listed():
    assert set(CAUGHT_BY) == set(P.MUTANTS)
    assert {c for _, cases in CAUGHT_BY.values() for c in cases} == set(CASE_NAMES)  # no idle case either


@pytest.mark.parametrize("mutant,name", [(mu, c) for mu, (_, cases) in CAUGHT_BY.items() for c in cases])
def test_mutant_is_caught(mutant, name):
    got_v, got_n, _ = P.run_model(P.case(name), mutant=mutant, order=CAUGHT_BY[mutant][0])
    want_v, want_n = P.expected(name)
    assert not same(got_v, want_v), "%s passes %s: the case no longer plants what it is for" % (mutant, name)
