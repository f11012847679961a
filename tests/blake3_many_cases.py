"""Batches of whole messages for the many-blob half of k_b3_upper (bw_blake3.hip): a pure function
of constants, like blake3_cases.py, whose cases and fixture digests it reuses.

launch_blake3 builds the tree levels above the leaf groups in one of two ways.  Up to
UPPER_BLOCK_BLOBS blobs (the batch's bound) every blob above one group gets a 4-wave workgroup.
Above it, blobs of up to SMALL_LEAVES leaves get a lane each (b3_small_blob, blocks of 256 blobs)
and larger ones a wave each (b3_upper_wave<.., 64>, four to a block), on a grid of at most
WAVE_GRID_BLOCKS blocks, so that from WAVES_AT_CAP + 1 blobs on a wave takes blob w, then blob
w + WAVES_AT_CAP.  tests/test_blake3_many_cases.py pins the three constants to the source.

Edge cases: the SMALL offset-0 cases and the TREE cases of blake3_cases.py.  Fillers: the SMALL
offset-0 cases of 0..FILL_MAX bytes (rooted in the leaf pass), message i of a layout taking
i % (FILL_MAX + 1) bytes.  Placement follows test_gpu_blake3_upstream.py::packed: the buffer sits
on a 128-byte boundary and is 0xFF wherever no message lies, an edge case that is message i of its
layout starts where the address is (37 * i) % 128 mod 128, a filler starts right where message
i - 1 ends (so the leaf pass's waves straddle blobs), and the last message ends at the buffer's end.

Layouts (LAYOUTS):
  flip-8192, flip-8193  one list, cut after 8192 and after 8193 messages: every edge case lies in
                  the first 8192, an odd stride apart, the longest as message 8191.  The two
                  batches differ in the k_b3_upper path alone.
  small-only      nothing above SMALL_LEAVES leaves, so only lane-per-blob blocks are launched:
                  every leaf count 5..64 at -1/0/+1 byte as messages 0..179 (whole waves of stacks
                  of different depth), then every SMALL case of up to 64 leaves (those 180 again
                  among them) at shuffled places among the fillers.
  mixed-shuffled  every edge case at shuffled places among the fillers.
  mixed-runs      the blobs above 64 leaves in two runs, one at each end of the batch (four in a
                  row share a block's four waves; the first and the last message are large), the
                  blobs of 5..64 leaves in one run, then the remaining edge cases.
  strided         more than WAVES_AT_CAP + 2048 messages: large blobs at i and i + WAVES_AT_CAP for
                  18 values of i, 0..3 and the last four that have a partner among them, the
                  longer tree first in every other pair; a large blob is the last message.  A
                  subset of the TREE cases: TREE_LEAVES at +0, and 65, 259..261, 3072 at -1 and +1.
"""
import functools
from collections import namedtuple

import numpy as np

import blake3_cases as cases

UPPER_BLOCK_BLOBS = 8192                # B3_UPPER_BLOCK_BLOBS: the last bound with a workgroup per blob
SMALL_LEAVES = 64                       # B3_SMALL_LEAVES: the last leaf count with a lane per blob
WAVE_GRID_BLOCKS = 4096                 # launch_blake3's cap on the wave-per-blob blocks
WAVES_AT_CAP = 4 * WAVE_GRID_BLOCKS     # blockDim 256: four waves a block
FILL_MAX = 130
LEAF = 1024

FLIP_LO, FLIP_HI = "flip-%d" % UPPER_BLOCK_BLOBS, "flip-%d" % (UPPER_BLOCK_BLOBS + 1)
LAYOUTS = (FLIP_LO, FLIP_HI, "small-only", "mixed-shuffled", "mixed-runs", "strided")

MANY = UPPER_BLOCK_BLOBS + 512 + 3      # small-only and the mixed layouts: the last block of 256 lanes is partial
STRIDED = WAVES_AT_CAP + 2048 + 5
RUNS_TAIL, RUNS_MID_AT = 6, 1027        # mixed-runs: large blobs in the tail run; where the 5..64-leaf run starts
STRIDED_TREE_PM = (65, 259, 260, 261, 3072)

# group, k: the case's place in blake3_cases.digests(fixture, group); edge: placed by the 37 * i rule
Msg = namedtuple("Msg", "edge group k off n")


def leaves(n):
    return max(1, -(-n // LEAF))


def label(m):
    return ("fill" if not m.edge else m.group, m.n)


@functools.lru_cache(maxsize=None)
def edge_cases():
    """The SMALL offset-0 cases, then the TREE cases, in fixture order."""
    small = [Msg(True, "small", k, off, n) for k, (off, n) in enumerate(cases.small_cases()) if off == 0]
    tree = [Msg(True, "tree", k, off, n) for k, (off, n) in enumerate(cases.tree_cases())]
    assert [m.k for m in small] == list(range(len(cases.SMALL_LENS)))  # the offset-0 cases lead the fixture
    return tuple(small + tree)


def filler(i):
    n = i % (FILL_MAX + 1)
    assert cases.SMALL_LENS[n] == n  # lengths 0..130 are the first SMALL cases
    return Msg(False, "small", n, 0, n)


def _fill_in(n_msgs, at):
    """The layout's message list: at[i] where given, a filler everywhere else."""
    assert all(0 <= i < n_msgs for i in at)
    return [at[i] if i in at else filler(i) for i in range(n_msgs)]


def _scatter(rng, free, msgs, at):
    free = np.asarray(free)
    for i, m in zip(rng.permutation(len(free))[:len(msgs)], msgs):
        at[int(free[i])] = m
    assert len(msgs) <= len(free)


def _flip():
    e = edge_cases()
    stride = (UPPER_BLOCK_BLOBS - 1) // (len(e) - 1)
    stride -= 1 - stride % 2  # odd: 37 * stride * k then runs through all 128 start offsets
    at = {k * stride: m for k, m in enumerate(e[:-1])}
    assert max(at) < UPPER_BLOCK_BLOBS - 1
    at[UPPER_BLOCK_BLOBS - 1] = e[-1]  # 3 MiB + 1: the last message of the shorter batch
    return _fill_in(UPPER_BLOCK_BLOBS + 1, at)


def lane_run():
    """Every leaf count 5..SMALL_LEAVES at -1/0/+1 byte (SMALL cases), ascending."""
    run = [m for m in edge_cases() if m.group == "small" and 4 < leaves(m.n) <= SMALL_LEAVES
           and (m.n + 1) % LEAF <= 2]
    assert len(run) == 3 * (SMALL_LEAVES - 4)  # 4 KiB + 1 .. 64 KiB
    return run


def _small_only():
    run = lane_run()
    at = dict(enumerate(run))
    again = [m for m in edge_cases() if m.group == "small" and leaves(m.n) <= SMALL_LEAVES]
    _scatter(np.random.default_rng(6401), range(len(run), MANY), again, at)
    return _fill_in(MANY, at)


def _mixed_shuffled():
    at = {}
    _scatter(np.random.default_rng(6402), range(MANY), edge_cases(), at)
    return _fill_in(MANY, at)


def _mixed_runs():
    e = edge_cases()
    large = [m for m in e if leaves(m.n) > SMALL_LEAVES]
    mid = [m for m in e if 4 < leaves(m.n) <= SMALL_LEAVES]
    rest = [m for m in e if leaves(m.n) <= 4]
    head, tail = large[:-RUNS_TAIL], large[-RUNS_TAIL:]
    assert len(head) < RUNS_MID_AT and RUNS_MID_AT + len(mid) + len(rest) < MANY - RUNS_TAIL
    at = dict(enumerate(head))
    at.update((RUNS_MID_AT + j, m) for j, m in enumerate(mid + rest))
    at.update((MANY - RUNS_TAIL + j, m) for j, m in enumerate(tail))
    return _fill_in(MANY, at)


def strided_pairs():
    """[(i, i + WAVES_AT_CAP)]: the indices of the strided layout's large blobs."""
    partners = STRIDED - WAVES_AT_CAP  # indices 0 .. partners - 1 have one
    firsts = [0, 1, 2, 3] + [5 + 113 * j for j in range(10)] + [partners - 4 + j for j in range(4)]
    assert firsts == sorted(set(firsts)) and firsts[-1] + WAVES_AT_CAP == STRIDED - 1
    return [(i, i + WAVES_AT_CAP) for i in firsts]


def _strided():
    e = edge_cases()
    keep = {k * LEAF for k in cases.TREE_LEAVES} | {k * LEAF + d for k in STRIDED_TREE_PM for d in (-1, 1)}
    large = sorted((m for m in e if leaves(m.n) > SMALL_LEAVES and (m.group == "small" or m.n in keep)),
                   key=lambda m: (m.n, m.group))
    pairs = strided_pairs()
    assert len(large) == 2 * len(pairs), len(large)
    at = {}
    for j, (a, b) in enumerate(pairs):  # the shortest with the longest, and so on inwards
        two = (large[j], large[-1 - j])
        at[a], at[b] = two if j % 2 == 0 else two[::-1]
    free = [i for i in range(STRIDED) if i not in at]
    _scatter(np.random.default_rng(6403), free, [m for m in e if leaves(m.n) <= SMALL_LEAVES], at)
    return _fill_in(STRIDED, at)


@functools.lru_cache(maxsize=None)
def order(name):
    """The layout's messages, in batch order."""
    if name in (FLIP_LO, FLIP_HI):
        return tuple(_flip()[:UPPER_BLOCK_BLOBS + (name == FLIP_HI)])
    return tuple({"small-only": _small_only, "mixed-shuffled": _mixed_shuffled, "mixed-runs": _mixed_runs,
                  "strided": _strided}[name]())


def place(msgs):
    """([start offset of each message], buffer size) by the placement rule above."""
    offs, pos = [], 0
    for i, m in enumerate(msgs):
        if m.edge:
            pos += (37 * i - pos) % 128
        offs.append(pos)
        pos += m.n
    assert msgs[-1].n > 0  # so that "ends at the buffer's end" says something
    return offs, pos


def aligned(a, align=128):
    """A copy of uint8 array `a` whose first byte sits on an `align`-byte boundary."""
    raw = np.empty(a.size + align, dtype=np.uint8)
    s = (-raw.ctypes.data) % align
    out = raw[s:s + a.size]
    out[:] = a
    assert out.ctypes.data % align == 0
    return out


def layout(name, fixture):
    """(buffer, offs, lens, case labels, expected digests) of one layout; `fixture` is the loaded
    tests/golden/blake3_upstream.json."""
    msgs = order(name)
    offs, size = place(msgs)
    src = {"small": cases.small_source(), "tree": cases.tree_source()}
    dig = {g: cases.digests(fixture, g) for g in src}
    buf = aligned(np.full(size, 0xFF, dtype=np.uint8))
    for o, m in zip(offs, msgs):
        buf[o:o + m.n] = src[m.group][m.off:m.off + m.n]
    assert offs[-1] + msgs[-1].n == buf.size
    buf.setflags(write=False)
    return buf, np.array(offs, dtype=np.uint64), np.array([m.n for m in msgs], dtype=np.uint64), \
        [label(m) for m in msgs], [dig[m.group][m.k] for m in msgs]
