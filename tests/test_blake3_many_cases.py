"""The batches of tests/blake3_many_cases.py, checked on the CPU: the thresholds they are built
around are the ones in bw_blake3.hip, every layout has the geometry its description promises, and
the bytes in each buffer hash (the oracle's CPU BLAKE3) to the fixture digest filed beside them.
tests/test_gpu_blake3_many_blobs.py then runs them through k_b3_upper's many-blob path."""
import json
import os
import re

import numpy as np
import pytest

import blake3_cases as cases
import blake3_many_cases as many

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "blake3_upstream.json")))
SRC = open(os.path.join(os.path.dirname(HERE), "backuwup_amd", "csrc", "bw_blake3.hip")).read()


def _one(pattern):
    found = re.findall(pattern, SRC)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_thresholds_are_the_kernels():
    """Whoever retunes one of these gets a failing test here, not a suite that has quietly left the
    many-blob path (or the strided wave loop)."""
    assert int(_one(r"#define\s+B3_UPPER_BLOCK_BLOBS\s+(\d+)")) == many.UPPER_BLOCK_BLOBS
    assert _one(r"per_block\s*=\s*max_blobs\s*(<=?)\s*B3_UPPER_BLOCK_BLOBS\b") == "<="
    assert int(_one(r"constexpr\s+uint64_t\s+B3_SMALL_LEAVES\s*=\s*(\d+)\s*;")) == many.SMALL_LEAVES
    cap = _one(r"if\s*\(\s*big\s*>\s*(\d+)\s*\)\s*big\s*=\s*(\d+)\s*;")
    assert int(cap[0]) == int(cap[1]) == many.WAVE_GRID_BLOCKS
    # four waves a block, one blob a wave: (max_blobs + 3) / 4 blocks of 256 threads
    _one(r"\(max_blobs\s*\+\s*3\)\s*/\s*4")
    _one(r"hipLaunchKernelGGL\(k_b3_upper,\s*dim3\(\(unsigned\)\(small \+ big\)\),\s*dim3\(256\)")
    assert many.WAVES_AT_CAP == 4 * many.WAVE_GRID_BLOCKS


@pytest.fixture(scope="module", params=many.LAYOUTS)
def lay(request):
    return (request.param, many.order(request.param)) + many.layout(request.param, FIX)


def test_layout_invariants(lay):
    name, msgs, buf, offs, lens, labels, want = lay
    n = len(msgs)
    assert len(offs) == len(lens) == len(labels) == len(want) == n
    # which side of the two thresholds
    if name == many.FLIP_LO:
        assert n == many.UPPER_BLOCK_BLOBS
    elif name == many.FLIP_HI:
        assert n == many.UPPER_BLOCK_BLOBS + 1
    elif name == "strided":
        assert n >= many.WAVES_AT_CAP + 2048
        assert -(-n // 4) > many.WAVE_GRID_BLOCKS  # the grid is at its cap
    else:
        assert many.UPPER_BLOCK_BLOBS < n <= many.WAVES_AT_CAP  # one blob a wave
        assert n % 256  # lane-per-blob: the last block has lanes past the last blob
    # placement
    assert buf.ctypes.data % 128 == 0 and buf.dtype == np.uint8
    o, ln = offs.astype(np.int64), lens.astype(np.int64)
    assert [int(x) for x in ln] == [m.n for m in msgs]
    assert np.all(o[1:] >= o[:-1] + ln[:-1])  # in order, no two overlap
    edge = np.array([m.edge for m in msgs])
    idx = np.arange(n)
    assert np.array_equal(o[edge] % 128, (37 * idx[edge]) % 128)
    assert o[0] == 0 and np.all(o[1:] - (o + ln)[:-1] < 128)
    fill = np.nonzero(~edge)[0]
    fill = fill[fill > 0]
    assert np.array_equal(o[fill], (o + ln)[fill - 1])  # a filler starts where its predecessor ends
    assert ln[-1] > 0 and int(o[-1] + ln[-1]) == buf.size
    used = np.zeros(buf.size, dtype=bool)
    for a, k in zip(o.tolist(), ln.tolist()):
        used[a:a + k] = True
    assert np.all(buf[~used] == 0xFF) and (~used).sum() > 0  # the gaps
    starts = len({int(x) % 128 for x in o[edge]})  # of the 128 start offsets of a 128-byte line
    assert starts == 128 if name in (many.FLIP_LO, many.FLIP_HI) else starts > 100
    # fillers are rooted in the leaf pass and come with fixture digests
    assert all(m.n <= many.FILL_MAX and m.group == "small" and m.off == 0 for m in msgs if not m.edge)
    assert (~edge).sum() > n - 600


def _leaves(msgs):
    return np.array([many.leaves(m.n) for m in msgs])


def test_flip_layouts_differ_by_one_filler():
    lo, hi = many.order(many.FLIP_LO), many.order(many.FLIP_HI)
    assert hi[:len(lo)] == lo and len(hi) == len(lo) + 1 and not hi[-1].edge and hi[-1].n > 0
    assert many.place(hi)[0][:len(lo)] == many.place(lo)[0]
    assert {m for m in lo if m.edge} == set(many.edge_cases())  # every edge case inside the first 8192
    assert many.leaves(lo[-1].n) > many.SMALL_LEAVES  # the shorter batch ends in a large blob


def test_flip_coverage():
    for name in (many.FLIP_LO, many.FLIP_HI):
        have = {m.n for m in many.order(name) if m.edge}
        for k in list(range(5, many.SMALL_LEAVES + 1)) + list(cases.TREE_LEAVES):
            for d in (-1, 0, 1):
                assert k * 1024 + d in have, (name, k, d)
        assert set(range(131)) <= have and set(cases.tree_lens()) <= have


def test_small_only_geometry():
    msgs = many.order("small-only")
    lv = _leaves(msgs)
    assert lv.max() == many.SMALL_LEAVES  # big == 0: no wave-per-blob block is launched
    run = many.lane_run()
    assert list(msgs[:len(run)]) == run and len(run) > 2 * 64  # contiguous: whole waves of live stacks
    want = {k * 1024 + d for k in range(5, many.SMALL_LEAVES + 1) for d in (-1, 0, 1)} - {many.SMALL_LEAVES * 1024 + 1}
    assert {m.n for m in run} == want | {4 * 1024 + 1}
    assert {many.leaves(m.n) for m in run} == set(range(5, many.SMALL_LEAVES + 1))
    rest = msgs[len(run):]
    assert {m.n for m in rest if m.edge} >= {m.n for m in run}  # the same set again, among the fillers
    at = [i for i, m in enumerate(rest) if m.edge and m in run]
    assert at != sorted(at, key=lambda i: rest[i].n) and max(at) - min(at) > len(rest) // 2  # shuffled, spread out


def test_mixed_shuffled_geometry():
    msgs = many.order("mixed-shuffled")
    assert sorted(m for m in msgs if m.edge) == sorted(many.edge_cases())
    at = np.array([i for i, m in enumerate(msgs) if m.edge])
    assert len({int(i) % 64 for i in at}) == 64 and len({int(i) // 256 for i in at}) > 30
    big = np.nonzero(_leaves(msgs) > many.SMALL_LEAVES)[0]
    assert len({int(i) % 4 for i in big}) == 4  # every wave of a block


def test_mixed_runs_geometry():
    msgs = many.order("mixed-runs")
    assert sorted(m for m in msgs if m.edge) == sorted(many.edge_cases())
    lv = _leaves(msgs)
    big = np.nonzero(lv > many.SMALL_LEAVES)[0]
    head = big[big < len(msgs) - many.RUNS_TAIL]
    assert np.array_equal(head, np.arange(len(head))) and len(head) >= 8  # whole blocks of four large blobs
    assert np.array_equal(big[len(head):], np.arange(len(msgs) - many.RUNS_TAIL, len(msgs)))
    assert big[0] == 0 and big[-1] == len(msgs) - 1
    mid = np.nonzero((lv > 4) & (lv <= many.SMALL_LEAVES))[0]
    assert np.array_equal(mid, np.arange(mid[0], mid[0] + len(mid))) and len(mid) > 3 * 64 and mid[0] % 64


def test_strided_geometry():
    msgs = many.order("strided")
    lv = _leaves(msgs)
    pairs = many.strided_pairs()
    big = set(np.nonzero(lv > many.SMALL_LEAVES)[0].tolist())
    assert big == {i for p in pairs for i in p}
    assert all(b - a == many.WAVES_AT_CAP for a, b in pairs) and len(pairs) >= 8
    assert pairs[0][0] == 0 and pairs[-1][1] == len(msgs) - 1  # the first wave, and the last index with a partner
    assert [a for a, _ in pairs[:4]] == [0, 1, 2, 3]  # one block's four waves, each with two trees
    # both orders: a tree with global rounds (more than 64 group nodes at 4 leaves a group) after a
    # short one in the same wave's cv_tmp slots, and the other way round
    deep = [(lv[a] >= 260, lv[b] >= 260) for a, b in pairs]
    assert (False, True) in deep and (True, False) in deep and (True, True) in deep
    have = {m.n for m in msgs if m.edge}
    assert {k * 1024 for k in cases.TREE_LEAVES} <= have
    assert {k * 1024 + d for k in many.STRIDED_TREE_PM for d in (-1, 1)} <= have
    assert {k * 1024 + d for k in range(5, many.SMALL_LEAVES + 1) for d in (-1, 0, 1)} - {64 * 1024 + 1} <= have


def test_buffers_hash_to_their_digests(oracle, lay):
    """The builder's self-check: every message of every layout, through the oracle's CPU BLAKE3."""
    name, msgs, buf, offs, lens, labels, want = lay
    bad = [(i, labels[i]) for i, (o, n) in enumerate(zip(offs.tolist(), lens.tolist()))
           if oracle.blake3(buf[o:o + n]) != want[i]]
    assert not bad, (name, len(bad), bad[:8])
