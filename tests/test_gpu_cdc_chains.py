"""The chunker's second stage -- speculative chains, their extension, k_resolve, the serial walker
and the unit scan -- pinned with planted chains (tests/cdc_chain_plant.py).

Random data makes neighbouring chains meet at the first cut after a segment start.  Here ladders of
windows and off-phase forced cuts hold them apart for a chosen number of cuts, so the merge is found
at a chosen index of the neighbour's chain, beyond the next segment's start, exactly at CHAIN_CAP,
or not at all.  Every case is compared exactly with the CPU oracle (file, offset, length, gear_hash,
digest, is_dup) and then asserts, from bw_batch_counters, the path a plain model of the resolution
rule computed on the CPU: serial_files, segments and seg_bytes.  A wrongly pessimistic k_resolve
costs only speed and shows in nothing but serial_files.  Every serial case also runs with
BW_F_SERIAL_RESOLVE.  tests/test_cdc_chain_plant.py holds, on the CPU, what the cases rest on."""
import numpy as np
import pytest

import cdc_chain_plant as cc
import cdc_plant as cp
from backuwup_amd import make_params
from backuwup_amd._lib import BW_BC_NONE, BW_F_SERIAL_RESOLVE
from test_gpu_cdc_planted import (blobs_equal, built, cand_cap, check, gear, reference, run, tile,  # noqa: F401
                                  win)

pytestmark = pytest.mark.gpu


def planned(case, g, tile):
    """The case's model resolution for the batch geometry of this tile size (forcing 128 KiB tiles
    makes the batch a large one for seg_len_for), computed once per case and geometry."""
    small = tile == 65536
    def make():
        m = built(("model", case.name), lambda: cc.Model(g, case.data, case.params))
        return m.resolve(case.offs, case.lens, case.threshold, small_batch=small)
    return built(("plan", case.name, small), make)


def check_path(ctx, oracle, case, g, tile, key, more=None):
    """Exact blobs, then the model's path from the counters; a serial case once more with the
    serial walker forced."""
    res = planned(case, g, tile)
    assert ("serial" if res["serial"] else "chain") == case.path
    expect = dict(serial_files=len(res["serial"]), segments=res["segments"], seg_bytes=res["seg_bytes"], trunc=BW_BC_NONE)
    expect.update(more or {})
    got, ctr = check(ctx, oracle, case, tile, key, expect=expect)
    if res["serial"]:
        serial, sctr = run(ctx, case, flags=BW_F_SERIAL_RESOLVE)
        assert sctr["serial_files"] == ctr["cdc_files"]
        blobs_equal(serial, reference(oracle, case, key), case.name + ", serial walker")
    return got, ctr


@pytest.mark.parametrize("k,tail_cut", cc.A_CASES, ids=lambda v: str(v))
def test_ladder_lengths(ctx, oracle, gear, win, tile, k, tail_cut):
    """A: two chains on opposite rungs of a ladder; the merge is found at index 0, 1, 63, 64 (the
    v0 / v1 seam of k_extend), 126 and 127 of the neighbour's stored entries.  Chain path."""
    case = built(("A", k), lambda: cc.ladder_a(gear, win, k, tail_cut))
    check_path(ctx, oracle, case, gear, tile, ("A", k))


@pytest.mark.parametrize("m,steps,on_end", cc.B_CASES, ids=lambda v: str(int(v)))
def test_cap_boundaries(ctx, oracle, gear, win, tile, m, steps, on_end):
    """B: a chain of exactly CHAIN_CAP entries stays on the chain path when it merges on a stored
    entry (or fills up with the merge itself), and the file goes serial when it needs one more."""
    case = built(("B", m, steps, on_end), lambda: cc.cap_b(gear, win, m, steps, on_end))
    check_path(ctx, oracle, case, gear, tile, ("B", m, steps, on_end))


@pytest.mark.parametrize("sub", [1, 2, 3])
def test_merge_beyond_next_start(ctx, oracle, gear, win, tile, sub):
    """C: the chains meet at the neighbour's first, then second cut past its own segment's end
    (chain path); one rung further its coverage ends first (serial)."""
    case = built(("C", sub), lambda: cc.beyond_c(gear, win, sub))
    check_path(ctx, oracle, case, gear, tile, ("C", sub))


@pytest.mark.parametrize("empty,tail", cc.D_CASES, ids=lambda v: str(int(v)))
def test_off_phase_forced_cuts(ctx, oracle, gear, win, tile, empty, tail):
    """D: 1, 2 and 3 candidate-free segments after an off-phase cut, and nothing up to the file's
    end: one is bridged by the cut beyond the segment's end, more send the file to the walker."""
    case = built(("D", empty, tail), lambda: cc.forced_d(gear, win, empty, tail))
    check_path(ctx, oracle, case, gear, tile, ("D", empty, tail))


def run_batch(ctx, case, flags=0):
    """run() with the case's own small_file_threshold."""
    ctx.index_reset()
    t = ctx.submit_host(case.data, case.offs, case.lens,
                        make_params(*case.params, small_file_threshold=case.threshold, flags=flags))
    got = ctx.wait(t)
    return got, ctx.batch_counters(t)


def check_batch(ctx, oracle, case, g, tile, key):
    """check_path for a batch with files below the threshold: exact blobs, the model's counters, and
    for a batch with a serial file the same blobs with every file on the serial walker."""
    res = planned(case, g, tile)
    ref = built(("ref", key), lambda: oracle.process_files(case.data, case.offs, case.lens, *case.params,
                                                           small_threshold=case.threshold))
    case.check_cuts(ref)
    got, ctr = run_batch(ctx, case)
    blobs_equal(got, ref, case.name)
    want = dict(serial_files=len(res["serial"]), segments=res["segments"], seg_bytes=res["seg_bytes"],
                cdc_files=res["cdc_files"], tile_bytes=tile, trunc=BW_BC_NONE)
    for name, v in want.items():
        assert ctr[name] == v, (case.name, name, ctr)
    if res["serial"]:
        serial, sctr = run_batch(ctx, case, flags=BW_F_SERIAL_RESOLVE)
        assert sctr["serial_files"] == res["cdc_files"]
        blobs_equal(serial, ref, case.name + ", serial walker")
    return got, ctr


def test_file_shapes_in_one_batch(ctx, oracle, gear, win, tile):
    """E: one-segment files, files ending on a segment boundary and one byte either side of it, a
    last chunk and last segments of at most min bytes, empty and below-threshold files, and one
    serial file between chain-path files: exactly that one goes to the walker, and its neighbours'
    blobs (and fallback offsets) are untouched."""
    case = built("E", lambda: cc.shapes_e(gear, win))
    got, ctr = check_batch(ctx, oracle, case, gear, tile, "E")
    assert ctr["serial_files"] == 1 and ctr["cdc_files"] == 7


def test_remainder_below_avg(ctx, oracle, gear, win, tile):
    """E at P3: a remainder between min and avg (center = rem): an L-only window is no cut, an S
    window is."""
    case = built("E3", lambda: cc.remainder_e(gear, win))
    check_batch(ctx, oracle, case, gear, tile, "E3")


def test_resolve_beyond_its_block(ctx, oracle, tile):
    """F: more segments than k_resolve has threads, file heads anywhere in the threads' ranges;
    every chain merges at once, no file is walked serially, most blobs are duplicates."""
    case, g = built("F", lambda: cc.resolve_f(oracle))
    got, ctr = check_path(ctx, oracle, case, g, tile, "F")
    assert ctr["segments"] > cc.RESOLVE_THREADS and ctr["seg_bytes"] == (2048 if tile == 65536 else 4096)
    assert ctr["cand_found"] == 0 and got["is_dup"].sum() > len(got) // 2


def test_unit_scan_beyond_one_level(ctx, oracle, gear, win, tile):
    """G: more than 256 blocks of 256 units; three CDC files of three segments straddle unit
    indices 255 / 256 and 65,535 / 65,536 and close the table.  Exact blobs, file indices and
    canonical order included."""
    case = built("G", lambda: cc.units_g(gear, win))
    res = planned(case, gear, tile)
    assert case.facts["nunits"] > cc.UNIT_BLOCK ** 2 and not res["serial"]
    ref = reference(oracle, case, "G")
    got, ctr = run(ctx, case)
    blobs_equal(got, ref, case.name)
    assert np.all(np.diff(got["file"].astype(np.int64)) >= 0)
    for name in ("cdc_files", "segments", "seg_bytes"):
        assert ctr[name] == res[name], (name, ctr)
    assert ctr["serial_files"] == 0 and ctr["tile_bytes"] == tile


def truncated_cases(oracle, gear, win):
    return [("A", lambda: built(("A", 63), lambda: cc.ladder_a(gear, win, 63))),
            ("C", lambda: built(("C", 1), lambda: cc.beyond_c(gear, win, 1))),
            ("D", lambda: built(("D", 2, True), lambda: cc.forced_d(gear, win, 2, True))),
            ("H", lambda: built("H", lambda: cc.direct_h(gear, win)))]


@pytest.mark.parametrize("which", ["A", "C", "D", "H"])
def test_truncated_candidate_array(ctx, oracle, gear, win, tile, which):
    """H: a candidate array of one entry: from the first tile that does not fit, every body test
    is direct_scan's.  walk_next is shared by the chains and the walker, so the blobs and the path
    are those of the whole array."""
    case = dict(truncated_cases(oracle, gear, win))[which]()
    trunc = cc.expected_trunc(gear, case.data, tile, 1)
    assert trunc != cc.NONE
    with cand_cap(ctx, 1):
        check_path(ctx, oracle, case, gear, tile, ("H", which), more=dict(trunc=trunc, cand_stored=1))


@pytest.mark.parametrize("which", ["mask_switch", "head"])
def test_truncated_mask_switch_and_head(ctx, oracle, gear, win, tile, which):
    """The planted scan cases whose verdict depends on the mask region and on the head region,
    through direct_scan (mask_s below center, mask_l from there; the first position it may test)."""
    case = built(which, lambda: cp.mask_switch(gear, win) if which == "mask_switch" else cp.head(gear, win))
    trunc = cc.expected_trunc(gear, case.data, tile, 1)
    with cand_cap(ctx, 1):
        check(ctx, oracle, case, tile, which, expect={"serial_files": 0, "trunc": trunc, "cand_stored": 1})
