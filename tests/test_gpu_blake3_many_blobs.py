"""k_b3_upper's many-blob path against upstream BLAKE3 (tests/golden/blake3_upstream.json alone, as
in tests/test_gpu_blake3_upstream.py).

From a bound of 8193 blobs on, launch_blake3 no longer gives every blob a workgroup: blobs of
5..64 leaves get a lane each (b3_small_blob<false>: the in-place stack, its ROOT conditions and
the fold of the spine) and larger ones a wave each (b3_upper_wave<false, 64>: rounds of 63 parents
through global memory, then the register levels), on a grid whose cap makes a wave take several
blobs in turn from 16,385 blobs on.  Every other quick test stays at or below 8192 blobs, or has no
blob above one leaf.  The batches come from tests/blake3_many_cases.py, which
tests/test_blake3_many_cases.py checks on the CPU; a CDC batch whose bound is far above its blob
count (the `blob >= ctr[C_NBLOBS]` guard, slots nobody fills) is compared with the oracle."""
import json
import os

import numpy as np
import pytest

import blake3_many_cases as many
from backuwup_amd import Context, _lib, make_params
from backuwup_amd._lib import BW_OPT_B3_GROUP, BW_OPT_B3_UPPER
from backuwup_amd.synth import splitmix_bytes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "blake3_upstream.json")))

# flip: the two batches that differ only in the path, one after the other on one context (the
# longer run leaves its cv_buf / cv_tmp contents to the shorter one), then the other way round
RUNS = {"flip": (many.FLIP_HI, many.FLIP_LO, many.FLIP_HI), "small-only": ("small-only",),
        "mixed-shuffled": ("mixed-shuffled",), "mixed-runs": ("mixed-runs",), "strided": ("strided",)}


@pytest.fixture(scope="module", params=list(RUNS))
def batches(request):
    """[(layout name, its batch)] of one test case; a module-scoped parameter, so that one case's
    buffers are dropped before the next case's are built."""
    built = {name: many.layout(name, FIX) for name in set(RUNS[request.param])}
    return [(name, built[name]) for name in RUNS[request.param]]


def _check(name, batch, got):
    """Every digest equals the fixture's.  A mismatch reports how many differ, the first of them as
    (index, index % 256, leaves, length % 1024), and which half of k_b3_upper they belong to."""
    _, _, lens, labels, want = batch
    assert len(got) == len(want)
    bad = [i for i, w in enumerate(want) if bytes(got[i]) != w]
    if not bad:
        return
    lv = [many.leaves(int(lens[i])) for i in bad]
    lane, wave = sum(k <= many.SMALL_LEAVES for k in lv), sum(k > many.SMALL_LEAVES for k in lv)
    side = "all <= 64 leaves (lane per blob)" if not wave else "all > 64 leaves (wave per blob)" if not lane else \
        "both: %d of <= 64 leaves, %d of > 64" % (lane, wave)
    first = [(i, i % 256, k, int(lens[i]) % 1024) for i, k in zip(bad[:12], lv)]
    pytest.fail("%s: %d of %d digests differ, %s; first (index, index %% 256, leaves, length %% 1024): %s; cases %s"
                % (name, len(bad), len(want), side, first, [labels[i] for i in bad[:12]]), pytrace=False)


@pytest.mark.parametrize("group", [0, 4, 2, 1], ids=["lines", "lines-g4", "lines-g2", "lines-g1"])
def test_many_blob_upper_matches_upstream(ctx, batches, group):
    ctx.set_option(BW_OPT_B3_GROUP, group)
    try:
        for name, batch in batches:
            buf, offs, lens = batch[:3]
            _check(name, batch, ctx.blake3_many(buf, offs, lens))
    finally:
        ctx.set_option(BW_OPT_B3_GROUP, 0)  # the context default


# ------------------------------------------------------------------ a bound far above the blob count

CDC = (4096, 16384, 65536)
CDC_BYTES = 34 << 20  # chunks of 4..64 leaves, about two thousand of them
WHOLE_LEAVES = (65, 66, 259, 260, 261, 512, 1000)  # whole files of these leaf counts, -1 and +1 byte
THRESHOLD = 1000 * 1024 + 1  # the small-file threshold: the longest whole file


def _chunk_bound(n):
    """chunk_bound (bw_plan.h): every chunk but the last is at least min(s0, max) bytes, plus two."""
    mn, _, mx = CDC
    return n // min(2 * (mn // 2), mx) + 2


def test_bound_above_count_cdc_batch(oracle):
    """One process_files call, dedup on, fresh index: seven whole files, a 34 MiB CDC file, seven
    more whole files and copies of two earlier ones.  The batch's blob bound, the CDC file's
    chunk_bound plus one per whole file, is above 8192, so k_b3_upper runs its many-blob path over
    arrays of which only the first fifth is filled: the chunks are lane-per-blob, the whole files
    wave-per-blob.  Every record equals the oracle's."""
    assert 64 <= CDC[0] <= 1 << 20 and 256 <= CDC[1] <= 4 << 20 and 1024 <= CDC[2] <= 16 << 20  # make_masks
    assert CDC[0] <= CDC[2] and CDC[1] <= CDC[2] and CDC[2] <= many.SMALL_LEAVES * 1024
    whole = [k * 1024 + d for k in WHOLE_LEAVES for d in (-1, 1)]
    assert max(whole) <= THRESHOLD < CDC_BYTES and min(whole) > many.SMALL_LEAVES * 1024
    half = len(whole) // 2
    lens = whole[:half] + [CDC_BYTES] + whole[half:] + [whole[1], whole[half]]  # the last two: copies
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    data = splitmix_bytes(8193, int(sum(lens)))
    for dst, src in ((len(lens) - 2, 1), (len(lens) - 1, half + 1)):
        assert lens[dst] == lens[src]
        data[int(offs[dst]):int(offs[dst]) + lens[dst]] = data[int(offs[src]):int(offs[src]) + lens[src]]
    bound = sum(_chunk_bound(n) if n > THRESHOLD else 1 for n in lens)
    assert bound > many.UPPER_BLOCK_BLOBS
    want = oracle.process_files(data, offs, lens, *CDC, small_threshold=THRESHOLD, threads=8)
    chunks = want[want["file"] == half]
    assert len(want) == len(chunks) + len(lens) - 1 and 4 * len(want) < bound
    assert len(chunks) > 1500 and int(chunks["length"].max()) <= CDC[2]
    assert int((chunks["length"] > 4 * 1024).sum()) > 1000  # above one group: lane-per-blob stacks
    assert int(want["is_dup"].sum()) >= 2 and not want["is_dup"][:len(want) - 2].all()
    with Context(0) as c:
        c.index_reset()
        got = c.process_files(data, offs, lens, make_params(*CDC, small_file_threshold=THRESHOLD))
    assert got.shape == want.shape
    for field in ("file", "offset", "length", "gear_hash", "is_dup"):
        assert np.array_equal(got[field], want[field]), field
    bad = np.nonzero((got["digest"] != want["digest"]).any(axis=1))[0]
    assert bad.size == 0, (bad.size, [(int(i), int(got["file"][i]), int(got["length"][i])) for i in bad[:12]])


# ------------------------------------------------------------------ the fused instantiations

def _diag_lib():
    """True when the loaded library is the diagnostic build (BW_DIAG variants compiled in)."""
    return _lib.LIB_PATH.endswith("_debug.so")


@pytest.mark.parametrize("name", ["mixed-shuffled", "small-only"])
def test_fused_upper_same_cases(ctx, name):
    """BW_OPT_B3_UPPER 1 (diagnostic build, BW_LIB): b3_small_blob<true> and b3_upper_wave<true>,
    called from the leaf pass by the wave that completes a blob, over the same batches."""
    if not _diag_lib():
        pytest.skip("BW_OPT_B3_UPPER needs the diagnostic library (BW_LIB)")
    batch = many.layout(name, FIX)
    ctx.set_option(BW_OPT_B3_UPPER, 1)
    try:
        got = ctx.blake3_many(*batch[:3])
    finally:
        ctx.set_option(BW_OPT_B3_UPPER, 0)
    _check(name + " fused", batch, got)
