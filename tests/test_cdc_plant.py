"""The planted-candidate inputs of tests/cdc_plant.py against the CPU oracle alone (no GPU).

Every window of tests/golden/cdc_windows.json is re-classified with the oracle's gear table and
masks, and every input builder that tests/test_gpu_cdc_planted.py runs on the GPU is run through
oracle.process_files here: the planted positions that are meant to cut start a chunk of the
reference, the ones that must not do not, and the per-tile candidate and flagged-block counts the
GPU test's counter assertions rest on are what the builder says.  These are conditions on the
reference and the inputs, with no exceptions: a seed for which one fails is a wrong seed."""
import numpy as np
import pytest

import cdc_plant as cp


@pytest.fixture(scope="module")
def gear(oracle):
    return cp.Gear.of(oracle, cp.P1)


@pytest.fixture(scope="module")
def win():
    return cp.load_windows()


def reference(oracle, case):
    blobs = oracle.process_files(case.data, case.offs, case.lens, *case.params, small_threshold=0)
    case.check_cuts(blobs)
    return blobs


def check_census(gear, case):
    """What the counter assertions of the GPU test assume about the scan's view of the input."""
    h = gear.hash_all(case.data)
    for tile in ([case.tile] if case.tile else cp.TILES):
        cand, flagged = gear.census(case.data, tile, h)
        if case.tiles is not None:
            assert {t: (int(cand[t]), int(flagged[t])) for t in range(len(cand))} == case.tiles, (case.name, tile)
        elif case.expect.get("ovf_tiles") == 0:
            assert cand.max() <= cp.SCAN_CAP and flagged.max() <= cp.SCAN_CAP, (case.name, tile)
        if "cand_found" in case.expect:
            assert int(cand.sum()) == case.expect["cand_found"], (case.name, tile)


def test_masks_shared(oracle):
    """P1, P3 and backuwup's parameters differ in min and max only: the same two masks."""
    assert oracle.masks(*cp.P1) == oracle.masks(*cp.P3) == oracle.masks(*cp.BK)
    s, l = oracle.masks(*cp.BK)
    assert s & l == l and bin(s).count("1") == 21 and bin(l).count("1") == 19 and s.bit_length() == cp.WINDOW


def test_fixture_windows_classify(oracle, gear, win):
    assert win["params"] == cp.P1
    assert len(win[cp.S]) >= 8 and len(win[cp.L_ONLY]) >= 8 and len(win[cp.PRE_ONLY]) >= 32
    for kind in (cp.S, cp.L_ONLY, cp.PRE_ONLY):
        assert len(set(win[kind])) == len(win[kind])
        for w in win[kind]:
            assert len(w) == cp.WINDOW and gear.classify(w) == kind, (kind, w.hex())
            # whatever precedes the window: 16 other bytes in front change no verdict
            assert gear.classify(bytes(range(100, 116)) + w) == kind
    assert sorted(win["TRUNC"]) == [0, 1, 2, 45, 46]
    for k, pre in win["TRUNC"].items():
        if pre is not None:
            assert len(pre) == k + 1 and gear.hash_prefix(pre) & gear.mask_s == 0, k


def test_fixture_nulls_are_exhaustive(gear, win):
    """A null truncated prefix says that NO prefix of that length passes mask_s: 256 one-byte and
    65,536 two-byte prefixes, all tried here."""
    g = gear.g
    h1 = g
    h2 = ((g[:, None] << np.uint64(1)) + g[None, :]).reshape(-1)
    for k, h in ((0, h1), (1, h2)):
        none = not ((h & np.uint64(gear.mask_s)) == 0).any()
        assert (win["TRUNC"][k] is None) == none, k
    for k in (2, 45, 46):
        assert win["TRUNC"][k] is not None, k


def test_hash_all_matches_serial(gear):
    buf = cp.filler(3, 3000)
    h = gear.hash_all(buf, block=1024)
    for p in (0, 1, 46, 47, 48, 1023, 1024, 1025, 2999):
        assert int(h[p]) == gear.hash_prefix(buf[max(p - 63, 0):p + 1].tobytes()) & ((1 << cp.WINDOW) - 1), p


def test_sweep(oracle, gear, win):
    case = cp.sweep(win)
    assert len(case.cuts) == 2052 and {p % 2048 for p in case.cuts} == set(range(2048))
    assert {p % 2 for p in case.cuts} == {0, 1}
    blobs = reference(oracle, case)
    check_census(gear, case)
    # chain length: the cuts of any 1 MiB stretch (a P1 segment) stay well under CHAIN_CAP
    starts = np.sort(blobs["offset"])
    per_seg = np.bincount((starts >> 20).astype(np.int64))
    assert per_seg.max() <= cp.CHAIN_CAP // 2 + 8, per_seg.max()


def test_edge_phases_cover_the_offsets():
    for tile in cp.TILES:
        got = sorted(o for ph in range(cp.EDGE_PHASES) for o in cp.edge_phase(tile, ph))
        assert got == sorted(cp.edge_offsets(tile))


@pytest.mark.parametrize("tile", cp.TILES)
@pytest.mark.parametrize("delta", [0, 1, -1])
def test_edges(oracle, gear, win, tile, delta):
    seen = set()
    for phase in range(cp.EDGE_PHASES):
        case = cp.edges(win, tile, phase, delta=delta)
        assert len(case.data) == 5 * tile + delta
        reference(oracle, case)
        check_census(gear, case)
        seen |= {(p // tile, p % tile) for p in case.cuts}
    n_t = (5 * tile + delta) // tile
    for t in ((n_t - 1) // 2, n_t - 1):  # a middle and the last full tile: every offset ...
        gone = {tile - 1} if t == n_t - 1 and delta == 0 else set()  # ... but the buffer's last byte
        assert {o for tt, o in seen if tt == t} == set(cp.edge_offsets(tile)) - gone, t
    assert {o for tt, o in seen if tt == 0} == {o for o in cp.edge_offsets(tile) if o >= 200}
    if delta == -1:  # the ragged tile holds tile - 1 bytes: every offset but its last
        assert {o for tt, o in seen if tt == n_t} == set(cp.edge_offsets(tile)) - {tile - 1}


CAPACITY = [dict(n_cand=16), dict(n_cand=17), dict(n_cand=4, n_pre=17), dict(n_cand=12, pair=True),
            dict(n_cand=15, pair=True)]


@pytest.mark.parametrize("tile", cp.TILES)
@pytest.mark.parametrize("kw", CAPACITY, ids=lambda k: "-".join("%s%s" % kv for kv in k.items()))
def test_capacity(oracle, gear, win, tile, kw):
    case = cp.capacity(gear, win, tile, **kw)
    reference(oracle, case)
    check_census(gear, case)
    want_ovf = {16: 0, 17: 1, 4: 1, 12: 0, 15: 1}[kw["n_cand"]]
    assert case.expect["ovf_tiles"] == want_ovf
    if kw.get("n_pre"):
        assert case.tiles[1][0] == 4 and case.tiles[1][1] > cp.SCAN_CAP
    if kw.get("pair"):
        # both sit in one 64-byte block, 48 bytes apart; the second lies inside the min of the
        # chunk the first one starts, so the scan must find both and the walker take only the first
        a, = [p for p in case.cuts if p // 64 == (tile + 2048) // 64]
        b, = [p for p in case.no_cuts if p // 64 == (tile + 2048) // 64]
        assert b - a == 48


def test_mask_switch(oracle, gear, win):
    case = cp.mask_switch(gear, win)
    assert case.cuts and case.no_cuts and 1 << 20 <= max(case.lens) <= 3 << 20
    blobs = reference(oracle, case)
    check_census(gear, case)
    # with the strays scrubbed each file is its planted cut or nothing: 1 or 2 chunks
    per_file = np.bincount(blobs["file"].astype(np.int64))
    assert set(per_file.tolist()) <= {1, 2} and int((per_file == 2).sum()) == len(case.cuts)


def test_head(oracle, gear, win):
    case = cp.head(gear, win)
    assert len(case.no_cuts) == len(cp.HEAD_K)
    reference(oracle, case)
    check_census(gear, case)


@pytest.mark.parametrize("empty", [False, True])
def test_segments(oracle, gear, win, empty):
    case = cp.segments(gear, win, empty=empty)
    blobs = reference(oracle, case)
    check_census(gear, case)
    cand, _ = gear.census(case.data, 1 << 20)
    assert (1 << 20) in case.cuts  # the cut ON segment 1's start
    if empty:
        assert cand.tolist() == [1, 1, 1, 0, 1, 0]  # none in segment 3
        assert len(blobs) == 7, blobs["offset"]  # the planted cuts plus forced cuts at max
    else:
        assert cand.tolist() == [1, 2, 1, 2, 1, 0]
        assert len(blobs) == len(case.cuts) + 1  # no forced cut


def test_backuwup_sweep(oracle, gear, win):
    case = cp.backuwup_sweep(gear, win)
    assert len(case.cuts) == 8 and case.params == cp.BK
    reference(oracle, case)
    check_census(gear, case)
