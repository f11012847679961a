"""The planted-chain inputs of tests/cdc_chain_plant.py against the CPU oracle alone (no GPU).

For every case: after scrubbing, the candidates are exactly the planted ones; the model's true chain
from each file start is the oracle's chunk list (which validates Model.cut, the only part of the
model the predicted path depends on besides the rule itself); the oracle honours every planted cut
and non-cut; and the structural facts the case was built for hold in the model's view of it -- the
index at which the merge is found, chain lengths against CHAIN_CAP, segment counts.  The last test
applies one-line mistakes to the rule and shows that the cases tell each of them apart."""
import numpy as np
import pytest

import cdc_chain_plant as cc
import cdc_plant as cp


@pytest.fixture(scope="module")
def gear(oracle):
    return cp.Gear.of(oracle, cp.P1)


@pytest.fixture(scope="module")
def win():
    return cp.load_windows()


_BUILT = {}


def built(key, make):
    if key not in _BUILT:
        _BUILT[key] = make()
    return _BUILT[key]


def all_cases(oracle, gear, win):
    """(case, its gear) for every case family, built once per session."""
    def make():
        out = [(cc.ladder_a(gear, win, k, z), gear) for k, z in cc.A_CASES]
        out += [(cc.cap_b(gear, win, *a), gear) for a in cc.B_CASES]
        out += [(cc.beyond_c(gear, win, s), gear) for s in (1, 2, 3)]
        out += [(cc.forced_d(gear, win, *a), gear) for a in cc.D_CASES]
        out += [cc.resolve_f(oracle)]
        out += [(cc.units_g(gear, win, tiny=1500), gear)]
        out += [(cc.direct_h(gear, win), gear), (cc.shapes_e(gear, win), gear), (cc.remainder_e(gear, win), gear)]
        return out
    return built("all", make)


def modelled(case, g, **kw):
    key = (case.name, tuple(sorted(kw.items())))
    like = modelled(case, g) if kw else None
    return built(key, lambda: cc.Model(g, case.data, case.params, like=like, **kw))


def verify(oracle, case, g):
    """The conditions every case must meet; returns the model's resolution of it."""
    m = modelled(case, g)
    assert m.cand == case.planted, (case.name, sorted(set(m.cand) ^ set(case.planted))[:8])
    ref = oracle.process_files(case.data, case.offs, case.lens, *case.params, small_threshold=case.threshold)
    case.check_cuts(ref)
    for f, (o, ln) in enumerate(zip(case.offs.tolist(), case.lens.tolist())):
        if ln > case.threshold and ln > 0 and ln > case.params[0]:
            want = (ref["offset"][ref["file"] == f] + o).tolist()
            assert m.true_chain(o, o + ln) == want, (case.name, f)
    res = m.resolve(case.offs, case.lens, case.threshold)
    assert ("serial" if res["serial"] else "chain") == case.path, (case.name, res["serial"])
    # what k_extend compares with must not depend on whether the neighbour's wave already extended
    late = modelled(case, g, late_neighbour=True).resolve(case.offs, case.lens, case.threshold)
    assert cc.signature(late) == cc.signature(res), case.name
    # a file on the chain path: the contributions of its segments are the oracle's chunk starts
    for f in set(sd["file"] for sd in res["segs"]) - set(res["serial"]):
        got = [p for sd in res["segs"] if sd["file"] == f for p in sd["starts"]]
        assert got == (ref["offset"][ref["file"] == f] + int(case.offs[f])).tolist(), (case.name, f)
    return res


@pytest.mark.parametrize("k,tail_cut", cc.A_CASES)
def test_ladder_lengths(oracle, gear, win, k, tail_cut):
    case = cc.ladder_a(gear, win, k, tail_cut)
    res = verify(oracle, case, gear)
    s0, s1 = res["segs"]
    assert res["seg_bytes"] == cc.MIB and res["segments"] == 2
    # the merge is found at index k of chain 1's stored entries: 63 / 64 is k_extend's v0 / v1 seam
    assert (s0["merge"], s0["merge_idx"]) == (case.facts["meet"], k)
    assert (s0["n"], s1["n"]) == case.facts["chain_len"] and max(s0["n"], s1["n"]) <= cp.CHAIN_CAP
    if k >= 2:  # opposite rungs all the way: the chains share no cut before they meet
        assert not (set(s0["chain"]) & set(s1["chain"])) - {case.facts["meet"], int(case.lens[0])}
        assert s0["n"] > s0["n0"]  # and chain 0 got there by extension
    if k == 127:
        assert s0["n"] == s1["n"] == cp.CHAIN_CAP and s1["chain"][127] == case.facts["meet"]


@pytest.mark.parametrize("m,steps,on_end", cc.B_CASES)
def test_cap_boundaries(oracle, gear, win, m, steps, on_end):
    case = cc.cap_b(gear, win, m, steps, on_end)
    res = verify(oracle, case, gear)
    s0, s1, s2 = res["segs"]
    assert s0["ok"] and s1["ok"] == s2["ok"] == (case.path == "chain")  # the middle chain decides
    assert s1["n0"] == case.facts["n0"]
    if case.path == "chain":
        assert s1["n"] == m + 2 + steps <= cp.CHAIN_CAP and s1["merge"] != cc.NONE
    elif m <= cp.CHAIN_CAP - 2:  # serial by one entry: the merge would have been entry CHAIN_CAP + 1
        assert m + 2 + steps == cp.CHAIN_CAP + 1 and s1["n"] == cp.CHAIN_CAP and s1["merge"] == cc.NONE
    else:
        assert s1["n0"] == cp.CHAIN_CAP + 1
    if on_end:
        assert 2 * cc.MIB in s1["chain"] and s1["n"] == cp.CHAIN_CAP


@pytest.mark.parametrize("sub", [1, 2, 3])
def test_merge_beyond_next_start(oracle, gear, win, sub):
    case = cc.beyond_c(gear, win, sub)
    res = verify(oracle, case, gear)
    s0, s1, s2, s3 = res["segs"]
    b2 = 2 * cc.MIB
    past = [e for e in s1["chain0"] if e >= b2]
    assert len(past) == 2 and s1["n"] == s1["n0"]  # chain 1: two cuts past its end, never extended
    assert case.facts["past_rungs"] == sub - 1
    if sub < 3:
        assert s0["merge"] == past[sub - 1] > b2  # the merge lies beyond the next segment's start
        assert s1["M"] == s0["merge"] and s2["M"] == max(s0["merge"], s1["merge"]) == s1["merge"]
        assert s1["starts"] == [e for e in s1["chain"] if s1["M"] <= e < s2["M"]]
    else:
        last1 = s1["chain0"][-1]
        assert s0["merge"] == cc.NONE and s0["chain"][-1] > last1 and s0["chain"][-2] < last1
        assert s0["n"] < cp.CHAIN_CAP  # given up for coverage, not for the cap


@pytest.mark.parametrize("empty,tail", cc.D_CASES)
def test_off_phase_forced_cuts(oracle, gear, win, empty, tail):
    case = cc.forced_d(gear, win, empty, tail)
    res = verify(oracle, case, gear)
    assert res["segments"] == -(-int(case.lens[0]) // cc.MIB)
    first = 3 * cc.MIB + cc.MIB // 2 + 1
    true = modelled(case, gear).true_chain(0, int(case.lens[0]))
    i = true.index(first)
    assert true[i:i + empty + 1] == [first + k * cc.MIB for k in range(empty + 1)]  # forced cuts, off every segment start
    assert (res["serial"] == []) == (empty == 1 and tail)


def test_file_shapes(oracle, gear, win):
    case = cc.shapes_e(gear, win)
    assert np.array_equal(case.offs[1:], np.cumsum(case.lens)[:-1])  # ascending, back to back
    res = verify(oracle, case, gear)
    names = case.facts["names"]
    assert res["serial"] == [names.index("serial")] and res["cdc_files"] == 7
    nseg = {names[f]: sum(sd["file"] == f for sd in res["segs"]) for f in range(len(names)) if case.lens[f] > cc.E_THRESHOLD}
    assert nseg == dict(chainX=2, exact=1, plus1=2, minus1=1, serial=4, chainY=3, above=1)
    ref = oracle.process_files(case.data, case.offs, case.lens, *case.params, small_threshold=cc.E_THRESHOLD)
    last = {names[f]: int(ref["length"][ref["file"] == f][-1]) for f in range(len(names))}
    assert last["plus1"] == 30 <= case.params[0] and last["empty"] == 0 and last["atthr"] == cc.E_THRESHOLD
    assert [int((ref["file"] == f).sum()) for f in (1, 2, 6, 8)] == [1, 1, 1, 1]  # single blobs
    tails = [sd for sd in res["segs"] if sd["end"] - sd["start"] <= case.params[0]]
    assert sorted(sd["end"] - sd["start"] for sd in tails) == [1, 50]  # segments of <= min bytes: their chain is the file's end
    assert all(sd["chain"] == [sd["file_end"]] for sd in tails)
    # the serial file lies between chain-path CDC files: its fallback range starts after theirs
    cdc = [f for f in range(len(names)) if case.lens[f] > cc.E_THRESHOLD]
    assert 0 < cdc.index(7) < len(cdc) - 1


def test_remainder_below_avg(oracle, gear, win):
    case = cc.remainder_e(gear, win)
    res = verify(oracle, case, gear)
    assert res["seg_bytes"] == 3 * cc.MIB and res["segments"] == 4
    m = modelled(case, gear)
    kinds = dict(zip(m.cand, zip(m.cand_s, m.cand_l)))
    assert [kinds[p] for p in case.no_cuts] == [(False, True)] * 2  # L-only windows, in a mask_s region to the end


def test_resolve_beyond_its_block(oracle):
    case, g = cc.resolve_f(oracle)
    v = case.facts["byte"]
    run = bytes([v]) * 200
    assert all(g.classify_hash(g.hash_prefix(run[:k])) not in (cp.S, cp.L_ONLY) for k in range(1, 200))
    res = verify(oracle, case, g)
    assert res["seg_bytes"] == 2048 and res["segments"] == sum(cc.F_SEGMENTS) > 2 * cc.RESOLVE_THREADS
    assert res["segments"] == sum(-(-n // 2048) for n in case.lens.tolist())
    per = -(-res["segments"] // cc.RESOLVE_THREADS)
    heads = np.concatenate([[0], np.cumsum(cc.F_SEGMENTS)[:-1]])
    assert per == 3 and set((heads % per).tolist()) == {0, 1, 2}  # heads at the start, inside and at the end of a range
    big = modelled(case, g).resolve(case.offs, case.lens, small_batch=False)
    assert big["seg_bytes"] == 4096 and big["segments"] > cc.RESOLVE_THREADS and not big["serial"]
    ref = oracle.process_files(case.data, case.offs, case.lens, *case.params, small_threshold=0)
    assert int((ref["length"] == 1024).sum()) == sum(n // 1024 for n in case.lens.tolist())  # every chunk but a file's last is max
    assert ref["is_dup"].sum() > len(ref) // 2


def test_unit_scan_layout(oracle, gear, win):
    """The layout arithmetic at full size (no data built), the rest on a small instance."""
    tiny = 66000
    at = [cc.UNIT_BLOCK - 2, cc.UNIT_BLOCK ** 2 - 4, tiny + 2]
    units, start = 0, {}
    for f in range(tiny + 3):
        start[f] = units
        units += 3 if f in at else 1
    assert [start[f] for f in at[:2]] == [254, 65534] and units == tiny + 9 and -(-units // cc.UNIT_BLOCK) > cc.UNIT_BLOCK
    case = cc.units_g(gear, win, tiny=1500)
    assert case.facts["big"][0] == at[0]
    res = verify(oracle, case, gear)
    assert res["segments"] == 6 + int((case.lens > 0).sum()) - 2


def test_direct_scan_positions(oracle, gear, win):
    case = cc.direct_h(gear, win)
    verify(oracle, case, gear)


MISTAKES = [dict(no_beyond=True), dict(first64=True), dict(last_merge=True), dict(end_gt=True), dict(cap=cp.CHAIN_CAP - 1)]


@pytest.mark.parametrize("kw", MISTAKES, ids=lambda k: "-".join("%s=%s" % kv for kv in k.items()))
def test_cases_tell_mistakes_apart(oracle, gear, win, kw):
    """Each one-line mistake in the rule changes the predicted serial set or some segment's
    contribution on at least one case."""
    hit = []
    for case, g in all_cases(oracle, gear, win):
        good = modelled(case, g).resolve(case.offs, case.lens, case.threshold)
        bad = modelled(case, g, **kw).resolve(case.offs, case.lens, case.threshold)
        if cc.signature(good) != cc.signature(bad):
            hit.append(case.name)
    assert hit, kw


def test_coverage_test_equality_is_unreachable(oracle, gear, win):
    """k_extend gives up on e >= last1.  e == last1 never gets there: last1 is one of the stored
    entries the cut was compared with just before, so '>' in its place states the same rule, and no
    input can tell the two apart.  (The '>=' that does matter is k_chains' c >= segment end:
    end_gt above.)"""
    for case, g in all_cases(oracle, gear, win):
        good = modelled(case, g).resolve(case.offs, case.lens, case.threshold)
        same = modelled(case, g, cover_gt=True).resolve(case.offs, case.lens, case.threshold)
        assert cc.signature(good) == cc.signature(same), case.name
