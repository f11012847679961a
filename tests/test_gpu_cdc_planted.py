"""The gear scan's fast path, pinned with planted cut candidates (tests/cdc_plant.py).

The other CDC tests compare finished chunk lists on random or periodic bytes.  At small parameters
nearly every scan tile overflows its 16 slots and the exact rescan replaces whatever k_scan's fast
path (v_perm gear fetch, prefilter, staged 64-byte steps, refine_block) found; at backuwup's masks a
random input has a few dozen cuts, and the chance that one of them sits on a given strip offset is
about 1 in 2048.  Here every deciding cut is planted: a known 48-byte window whose gear hash passes
a mask, written so that its last byte is the position under test.  min = 64 lets cuts sit 111 bytes
apart while the masks stay those of backuwup's avg = 1 MiB.

Every case runs at both scan tile sizes, compares the whole result with the CPU oracle exactly
(offset, length, gear_hash, digest, is_dup), and then asserts from bw_batch_counters that the path it
was built for produced that result: no overflowed tile, no truncated candidate array, no file
handed to the serial walker -- or exactly the overflow the case plants.  tests/test_cdc_plant.py
holds, on the CPU, every condition on the inputs these assertions rest on."""
import contextlib

import numpy as np
import pytest

import cdc_plant as cp
from backuwup_amd import make_params
from backuwup_amd._lib import (BW_BC_NONE, BW_ESTATE, BW_F_SERIAL_RESOLVE, BW_OPT_CAND_CAP, BW_OPT_DEPTH,
                               BW_OPT_SCAN_SMALL_BYTES, BwError)

pytestmark = pytest.mark.gpu

SMALL_BYTES_DEFAULT = 1 << 32  # bw_capi.hip: batches below 4 GiB scan half-size tiles
TILE_OPTION = {131072: 0, 65536: (1 << 64) - 1}  # BW_OPT_SCAN_SMALL_BYTES that forces each tile size


@pytest.fixture(scope="module")
def gear(oracle):
    return cp.Gear.of(oracle, cp.P1)


@pytest.fixture(scope="module")
def win():
    return cp.load_windows()


@pytest.fixture(params=cp.TILES, ids=lambda t: "tile%dk" % (t >> 10))
def tile(request, ctx):
    """Force one scan tile size on the shared context for the test, then put the default back."""
    ctx.set_option(BW_OPT_SCAN_SMALL_BYTES, TILE_OPTION[request.param])
    yield request.param
    ctx.set_option(BW_OPT_SCAN_SMALL_BYTES, SMALL_BYTES_DEFAULT)


@contextlib.contextmanager
def cand_cap(ctx, cap):
    ctx.set_option(BW_OPT_CAND_CAP, cap)
    try:
        yield
    finally:
        ctx.set_option(BW_OPT_CAND_CAP, 0)


_REF = {}


def reference(oracle, case, key):
    """The oracle's blobs of a case, computed once per input (both tile sizes share it)."""
    if key not in _REF:
        ref = oracle.process_files(case.data, case.offs, case.lens, *case.params, small_threshold=0)
        case.check_cuts(ref)
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def run(ctx, case, flags=0):
    ctx.index_reset()
    t = ctx.submit_host(case.data, case.offs, case.lens, make_params(*case.params, small_file_threshold=0, flags=flags))
    got = ctx.wait(t)
    return got, ctx.batch_counters(t)


def blobs_equal(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for f in ("file", "offset", "length", "gear_hash", "is_dup"):
        bad = np.nonzero(got[f] != ref[f])[0]
        assert not len(bad), (what, f, "first mismatch at blob", int(bad[0]), got[bad[0]], ref[bad[0]])
    assert np.array_equal(got["digest"], ref["digest"]), (what, "digest")


def check(ctx, oracle, case, tile, key, expect=None):
    """Run the case, compare with the oracle, then assert the path from the counters."""
    ref = reference(oracle, case, key)
    got, ctr = run(ctx, case)
    blobs_equal(got, ref, case.name)
    assert ctr["tile_bytes"] == tile and ctr["scan_tiles"] == -(-len(case.data) // tile), ctr
    assert ctr["cdc_files"] == len(case.offs), ctr
    for name, want in (case.expect if expect is None else expect).items():
        assert ctr[name] == want, (case.name, name, ctr)
    return got, ctr


_CASES = {}


def built(name, make):
    """The expensive inputs (tens of MB, scrubbed) are built once and shared by both tile sizes."""
    if name not in _CASES:
        _CASES[name] = make()
    return _CASES[name]


# ------------------------------------------------------------------ A: strip-offset sweep

def test_sweep_every_strip_offset(ctx, oracle, win, tile):
    """2052 S windows at stride 16385 = 1 (mod 2048): a planted cut on every offset of a strip, every
    lane of a refined block, every staging row and both parities (k_cut_hash's << 1), all delivered
    by the fast path; then the same blobs from the serial walker."""
    case = built("sweep", lambda: cp.sweep(win))
    got, ctr = check(ctx, oracle, case, tile, "sweep")
    assert ctr["segments"] == -(-len(case.data) // ctr["seg_bytes"]) and ctr["segments"] > 30
    assert ctr["cand_found"] == ctr["cand_stored"] >= len(case.cuts)
    serial, sctr = run(ctx, case, flags=BW_F_SERIAL_RESOLVE)
    assert sctr["serial_files"] == 1
    blobs_equal(serial, _REF["sweep"], "sweep, serial walker")


# ------------------------------------------------------------------ B: tile and buffer edges

@pytest.mark.parametrize("delta", [0, 1, -1])
def test_tile_and_buffer_edges(ctx, oracle, win, tile, delta):
    """One planted cut per file at the first / last bytes of tiles, strips and 64-byte steps, in the
    first, a middle and the last full tile and in the ragged tail tile, in buffers of exactly
    k * tile, k * tile + 1 and k * tile - 1 bytes; files start 200 bytes before their cut."""
    for phase in range(cp.EDGE_PHASES):
        case = cp.edges(win, tile, phase, delta=delta)
        check(ctx, oracle, case, tile, ("edges", tile, phase, delta))


# ------------------------------------------------------------------ C: slot capacity

@pytest.mark.parametrize("kw", [dict(n_cand=16), dict(n_cand=17), dict(n_cand=4, n_pre=17),
                                dict(n_cand=12, pair=True), dict(n_cand=15, pair=True)],
                         ids=lambda k: "-".join("%s%s" % kv for kv in k.items()))
def test_slot_capacity(ctx, oracle, gear, win, tile, kw):
    """A tile with exactly SCAN_CAP candidates stays on the fast path, one more (or more than
    SCAN_CAP flagged blocks around 4 candidates) puts exactly that tile on the overflow list; two
    candidates of one 64-byte block are both found.  The neighbouring tiles hold one candidate
    each: the candidate total and the exact result show them unaffected."""
    case = cp.capacity(gear, win, tile, **kw)
    check(ctx, oracle, case, tile, ("capacity", tile) + tuple(sorted(kw.items())))


def test_candidate_array_too_small(ctx, oracle, gear, win, tile):
    """BW_OPT_CAND_CAP below the 18 planted candidates: C_TRUNC names the tile that did not fit (the
    planted one), the walkers test the bytes from there on themselves, the blobs stay exact."""
    case = cp.capacity(gear, win, tile, n_cand=16)
    with cand_cap(ctx, 8):
        got, ctr = check(ctx, oracle, case, tile, ("capacity", tile, ("n_cand", 16)),
                         expect={"ovf_tiles": 0, "serial_files": 0, "cand_found": 18, "cand_stored": 8, "trunc": tile})
    assert min(case.cuts) <= ctr["trunc"] <= max(case.cuts)
    got, ctr = check(ctx, oracle, case, tile, ("capacity", tile, ("n_cand", 16)))  # and whole again without the cap
    assert ctr["trunc"] == BW_BC_NONE and ctr["cand_stored"] == 18


# ------------------------------------------------------------------ D: mask switch at center

def test_mask_switch_at_center(ctx, oracle, gear, win, tile):
    """P3, files of 1 to 3 MiB: an L-only window cuts at center but not at center - 1, an S window
    cuts at center - 1; r2 - 1 is the last tested position and r2 never cuts; in a file shorter
    than avg, center = rem and L-only windows never cut."""
    case = built("mask_switch", lambda: cp.mask_switch(gear, win))
    check(ctx, oracle, case, tile, "mask_switch")



# ------------------------------------------------------------------ E: head region

def test_head_region(ctx, oracle, gear, win, tile):
    """The 47 positions after s + s0 are judged by the truncated hash: a windowed candidate there is
    no cut, the fixture's truncated prefixes are, and k = 47 is the candidate array's first."""
    case = cp.head(gear, win)
    assert any(len(w) < cp.WINDOW for w in win["TRUNC"].values() if w)
    check(ctx, oracle, case, tile, "head")


# ------------------------------------------------------------------ F: segments

def p1_segment_bytes(ctx):
    """The segment length of P1 batches, read from the counters of a probe batch."""
    _, ctr = run(ctx, cp.Case("probe", cp.filler(1, 4096), [0], [4096], cp.P1))
    return ctr["seg_bytes"]


def test_cut_on_segment_start(ctx, oracle, gear, win, tile):
    """A cut exactly on a segment start (and one inside every segment): the chains merge."""
    seg = p1_segment_bytes(ctx)
    case = built(("segments", seg, False), lambda: cp.segments(gear, win, seg, empty=False))
    got, ctr = check(ctx, oracle, case, tile, ("segments", seg, False))
    assert ctr["seg_bytes"] == seg and ctr["segments"] == 6 and seg in case.cuts


def test_segment_without_candidates(ctx, oracle, gear, win, tile):
    """A segment with no candidate at all, crossed by one forced cut that is not a multiple of max
    from the segment's start.  The empty segment's speculative chain is a forced cut at 4 MiB that
    the true chain (3.5 MiB + 1, then 4 MiB + 12345) never makes; the two meet at the planted cut
    after it, which k_chains reaches by walking one cut beyond the segment's end.  Before that
    change this input gave exact blobs but serial_files = 1: the whole file went to k_fallback."""
    seg = p1_segment_bytes(ctx)
    case = built(("segments", seg, True), lambda: cp.segments(gear, win, seg, empty=True))
    got, ctr = check(ctx, oracle, case, tile, ("segments", seg, True))
    assert ctr["seg_bytes"] == seg and ctr["segments"] == 6


def test_backuwup_parameters(ctx, oracle, gear, win, tile):
    """True backuwup parameters, one 24 MiB file, 8 planted cuts (and no other candidate)."""
    case = built("bk", lambda: cp.backuwup_sweep(gear, win))
    got, ctr = check(ctx, oracle, case, tile, "bk")
    # 8 planted cuts, and one forced cut in the 3.3 MB after the last of them
    assert len(got) == 10 and ctr["segments"] == -(-len(case.data) // ctr["seg_bytes"]) >= 2



# ------------------------------------------------------------------ the counters call itself

def test_batch_counters_tickets(ctx):
    """Ticket 0 names the most recent batch; a ticket the ring dropped gives BW_ESTATE, like
    bw_wait; a batch without CDC files reports no tiles and nothing truncated.  (A context of its
    own: BW_OPT_DEPTH drops every held ticket.)"""
    from backuwup_amd import Context
    with Context(0) as c:
        c.set_option(BW_OPT_DEPTH, 2)
        data = cp.filler(4, 300000)
        p = make_params(*cp.P1, small_file_threshold=0)
        t1 = c.submit_host(data, [0], [len(data)], p)
        c.wait(t1)
        assert c.batch_counters(t1) == c.batch_counters(0)
        assert c.batch_counters(t1)["cdc_files"] == 1
        t2 = c.submit_host(data, [0, 1000], [1000, 2000], make_params(*cp.P1))  # both files below the threshold
        c.wait(t2)
        ctr = c.batch_counters(t2)
        assert (ctr["scan_tiles"], ctr["cdc_files"], ctr["segments"], ctr["trunc"]) == (0, 0, 0, BW_BC_NONE)
        t3 = c.submit_host(data, [0], [len(data)], p)
        c.wait(t3)
        with pytest.raises(BwError) as e:
            c.batch_counters(t1)  # depth 2: t3 took t1's slot
        assert e.value.rc == BW_ESTATE
        with pytest.raises(BwError):
            c.batch_counters(t3 + 1)
