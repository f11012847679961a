"""The planted cases of tests/retain_plant.py on the device.  Every comparison is exact: all sums are integers.

The drop (bw_retain_drop) over flat stores, with masks that come from nowhere but the plant: live, stats and
freed equal tests/retain_ref.py's drop, with and without the live vector, for every pattern x {1, 64, 65,
4095, 4096} roots over the geometries lane1, lane63, ones and one (where a packfile begins inside a wave),
against the wide family of drop sets; then the two batch cases, 65,534 .. 65,537 distinct sets over 48
entries (RT_DROP_BATCH_SETS binds) and 63,915 sets over 4,200 entries (RT_DROP_BATCH_BYTES binds), every row.
The mark (bw_retain_mark) over staircase(3), which needs four productive sweeps, and over ten distinct roots
cycled to 193, 4095 and 4096: masks, damaged, every per-root record, the totals, the counts and the errors
equal retain_ref.mark's, expanded by the rule that every given root has its own bit; the device's masks then
go through the drop, against prune.mark over the kept roots.  That a case reaches the path it is planted
for is tests/test_retain_plant.py's to show, on the CPU.  Outputs are filled with 0xa5 before every call, so
a row the library did not write differs from a row of zeros.

On an MI355X the file's 29 tests take 4.4 s of wall time, 1.6 s of it the context's set-up; the figure of
each test is in its docstring."""
import ctypes
import os
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import retain_plant as P  # noqa: E402
import zstd_ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]

FILL = 0xa5


def session(ctx, case):
    import restore_store
    from backuwup_amd import restore
    files, ids = [b for _, b in case["packs"]], [i for i, _ in case["packs"]]
    return restore.Session(ctx, restore_store.PRK, files, ids, ctx.unpack_headers(restore_store.PRK, files, ids),
                           restore_store.items_array(case["index"]), slots=case["slots"])


def device_drop(s, mask_words, n_roots, set_words, want_live=True):
    """bw_retain_drop with the sets given as words -> (live (n_sets, n_e) u8 or None, stats (n_sets, n_pf, 4) u64,
    freed (n_sets, 4) u64)."""
    from backuwup_amd import _lib
    m = np.ascontiguousarray(mask_words, dtype=np.uint64)
    d = np.ascontiguousarray(set_words, dtype=np.uint64)
    n_sets, n_e, n_pf = d.shape[0], s.n_entries, s.n_packfiles
    assert m.shape == (n_e, P.n_words(n_roots)) and d.shape[1] == m.shape[1]
    live = np.full((n_sets, n_e), FILL, dtype=np.uint8) if want_live else None
    stats = np.full((n_sets, n_pf, 4 * 8), FILL, dtype=np.uint8).view(np.uint64)
    freed = np.full((n_sets, 4 * 8), FILL, dtype=np.uint8).view(np.uint64)
    _lib.check(s._L.bw_retain_drop(s.h, m.ctypes.data_as(_lib.u64p), int(n_roots), d.ctypes.data_as(_lib.u64p), n_sets,
                                   None if live is None else live.ctypes.data_as(_lib.u8p),
                                   stats.ctypes.data_as(ctypes.POINTER(_lib.BwPrunePackfileStat)),
                                   freed.ctypes.data_as(ctypes.POINTER(_lib.BwRetainFreed))), s._ctx.h)
    return live, stats, freed


def assert_rows(got, want, what):
    """Row by row, so that a failure names the first set that is wrong."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not (got == want).all():
        q = int(np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0])
        raise AssertionError("%s: set %d is the first of %d wrong rows: got %r, want %r"
                             % (what, q, int((got != want).reshape(got.shape[0], -1).any(axis=1).sum()),
                                got[q].reshape(-1)[:16].tolist(), want[q].reshape(-1)[:16].tolist()))


# ------------------------------------------------------------------ the drop: where a packfile begins inside a wave
@pytest.mark.parametrize("n_roots", P.ROOT_COUNTS)
@pytest.mark.parametrize("geometry", P.WAVE_GEOMETRIES)
def test_drop_over_planted_masks_with_and_without_live(ctx, oracle, geometry, n_roots):
    """Seven patterns x the wide family (13 + W sets) on one session, each once with the live vector and once
    without.  MI355X: 0.01 - 0.07 s a case up to 65 roots, 0.14 - 0.28 s at 4095 and 4096 (most of it the
    reference's 7 x 76 drops in Python, once per process)."""
    store = P.flat(geometry)
    with session(ctx, store) as s:
        assert (s.n_entries, s.n_packfiles) == (store["n_entries"], len(store["groups"]))
        for pattern in P.PATTERNS:
            _, _, mw, sets, sw, (live, stats, freed) = P.drop_case(geometry, pattern, n_roots)
            got = device_drop(s, mw, n_roots, sw)
            what = "%s %s %d" % (geometry, pattern, n_roots)
            assert_rows(got[0], live, what + " live")
            assert_rows(got[1], stats, what + " stats")
            assert_rows(got[2], freed, what + " freed")
            got = device_drop(s, mw, n_roots, sw, want_live=False)
            assert got[0] is None
            assert_rows(got[1], stats, what + " stats without live")
            assert_rows(got[2], freed, what + " freed without live")


# ------------------------------------------------------------------ the drop: the batch loop
@pytest.mark.parametrize("n_sets", P.BITS_SETS)
def test_batches_by_sets_every_row(ctx, oracle, n_sets):
    """Set q is the binary expansion of q over 17 roots, 48 entries in packfiles of 33 and 15: one batch of
    65,534, one of 65,535, then 65,535 + 1 and 65,535 + 2.  Host arrays: live 3.1 MB, stats 4.2 MB, freed 2.1 MB.
    MI355X: 0.03 s for the first case, which builds the reference, under 0.005 s for each of the others."""
    store, mw, sw, (live, stats, freed) = P.sets_bound_case()
    assert P.per_of(n_sets, store["n_entries"]) == min(n_sets, P.BATCH_SETS)
    with session(ctx, store) as s:
        got = device_drop(s, mw, P.BITS_ROOTS, sw[:n_sets])
    assert max(x.nbytes for x in got) < 5 << 20
    assert_rows(got[0], live[:n_sets], "live")
    assert_rows(got[1], stats[:n_sets], "stats")
    assert_rows(got[2], freed[:n_sets], "freed")


def test_batches_by_bytes_every_row(ctx, oracle):
    """4,200 entries in 14 packfiles, 3 roots, set q = (5 q + 3) mod 8: per = 2^28 // 4200 = 63,913 sets a
    batch, 63,915 sets, no live vector (it would be 268 MB); then 16 sets with it.  MI355X: 0.18 s, store and
    reference included, so n_e stays at 4,200."""
    store, mw, sw, (_, stats, freed), live16 = P.bytes_bound_case()
    n_e = store["n_entries"]
    assert n_e > 4096 and P.per_of(sw.shape[0], n_e) == P.BATCH_BYTES // n_e == sw.shape[0] - 2 < P.BATCH_SETS
    with session(ctx, store) as s:
        got = device_drop(s, mw, P.CYCLE_ROOTS, sw, want_live=False)
        got16 = device_drop(s, mw, P.CYCLE_ROOTS, sw[:16])
    assert_rows(got[1], stats, "stats")
    assert_rows(got[2], freed, "freed")
    assert_rows(got16[0], live16, "live of 16 sets")
    assert_rows(got16[1], stats[:16], "stats of 16 sets")
    assert_rows(got16[2], freed[:16], "freed of 16 sets")


# ------------------------------------------------------------------ the mark
def as_errors(errors):
    return Counter((bytes(e["hash"]), bytes(e["parent"]), int(e["child_pos"]), int(e["reason"])) for e in errors)


def assert_mark(got, want, n_roots):
    from backuwup_amd import retain
    m, dmg, pr, counts, errs = got
    case, _, masks, damaged, per_root, errors, info = want
    assert m.shape == (case["n_entries"], retain.words(n_roots)) and P.to_ints(m) == masks
    assert dmg.tolist() == damaged
    records = [{f: int(x[f]) for f in retain.ROOT_DTYPE.names} for x in pr]
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(records, per_root)) if g != w]
    assert len(records) == n_roots and not bad, bad[:3]
    for f in ("n_trees_expanded", "n_levels", "n_edges", "reached_blobs", "reached_bytes", "orphan_blobs", "orphan_bytes"):
        assert counts[f] == info[f], f
    assert as_errors(errs) == errors and counts["n_errors"] == sum(errors.values())


def test_staircase_takes_four_productive_sweeps(ctx, oracle):
    """MI355X: 5 sweeps (four that change something and the one that does not), 0.01 s."""
    from backuwup_amd import retain
    want = P.staircase_reference(3)
    case = want[0]
    assert want[6]["n_sweeps"] == 5
    with session(ctx, case) as s:
        got = retain.mark(s, case["roots"])
    print("staircase(3): device sweeps", got[3]["n_sweeps"], "reference", want[6]["n_sweeps"])
    assert_mark(got, want, 2)
    assert got[3]["n_sweeps"] >= 4


@pytest.mark.parametrize("n", [193, 4095, 4096])
def test_cycled_roots_mark_then_drop(ctx, oracle, n):
    """Ten distinct roots at n places.  The mark against the expanded reference; then the device's own masks
    through the drop with the wide family: every set against retain_ref.drop, and the empty, the full, the
    first-word and the last-word set byte for byte against prune.mark over the kept roots (four prune marks).
    MI355X: 0.01 s at 193 roots, 0.04 s at 4095 and 4096."""
    from backuwup_amd import prune, retain
    want = P.cycled_reference(n)
    case, hd, masks = want[0], want[1], want[2]
    roots, sets, ix = case["roots"], P.wide(n), P.wide_index(n)
    four = [ix["empty"], ix["full"], ix["word0"], ix["last_word"]]
    with session(ctx, case) as s:
        got = retain.mark(s, roots)
        live, stats, freed = device_drop(s, got[0], n, P.to_words(sets, n))
        kept = [prune.mark(s, [r for k, r in enumerate(roots) if not sets[q] >> k & 1]) for q in four]
    assert_mark(got, want, n)
    store = dict(hd=hd, n_entries=case["n_entries"], groups=[len(h[3]) for h in hd])
    rlive, rstats, rfreed = P.reference_drop(store, masks, sets)
    assert_rows(live, rlive, "live")
    assert_rows(stats, rstats, "stats")
    assert_rows(freed, rfreed, "freed")
    for q, (plive, pstats, _, _) in zip(four, kept):
        assert live[q].tobytes() == plive.tobytes(), q
        assert stats[q].tobytes() == pstats.tobytes(), q
    # the four are different questions: nothing, everything, and two that keep something
    assert live[four[0]].all() and not live[four[1]].any() and 0 < live[four[2]].sum() < case["n_entries"] > live[four[3]].sum() > 0
