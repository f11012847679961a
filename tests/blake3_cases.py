"""The BLAKE3 cases of tests/golden/blake3_upstream.json: a pure function of constants, shared by the
generator (tests/golden/make_blake3_upstream.py) and by the tests that read the fixture.

SMALL: the small-message path (b3q_message in bw_b3_small.hip; messages up to 64 KiB, and the first
lengths past it, which fall through to the batch path).  Every leaf count 1..65 at -1/0/+1 byte,
every length 0..130 (each byte position of the first two blocks), and every position of the last
16-byte word of a leaf (t = 1009..1023) at the leaf counts where the tree merge changes shape
(1, 2, 32, 33, 34 and 64 leaves), each at four source alignments mod 16.

TREE: the batch path alone (k_b3_lines / k_b3_upper): the official test-vector lengths and the leaf
counts around 64 leaves and around the upper tree's passes, up to 3 MiB + 1.  In a batch of these
cases alone (a few hundred blobs) k_b3_upper gives every blob a 4-wave workgroup; its other path,
a lane per blob of up to 64 leaves and a wave per larger one from a bound of 8193 blobs on, sees
them in the batches of tests/blake3_many_cases.py.
"""
from backuwup_amd.synth import splitmix_bytes

SMALL_SEED, SMALL_BYTES = 4242, (70 << 10) + 64
SMALL_OFFS = (0, 1, 5, 15)
SMALL_LENS = sorted({k * 1024 + d for k in range(1, 66) for d in (-1, 0, 1)}
                    | set(range(0, 131))
                    | {k * 1024 + t for k in (0, 1, 31, 32, 33, 63) for t in range(1009, 1024)})

TREE_SEED, TREE_BYTES, TREE_OFF = 4243, 4 << 20, 3
TREE_LEAVES = (65, 66, 127, 128, 129, 255, 256, 257, 259, 260, 261, 511, 512, 513, 1023, 1024, 1025, 2047, 2048,
               2049, 3071, 3072)


def tree_lens():
    from test_gpu_parity import TV_LENS  # the official test-vector lengths plus the tree-shape edges
    return sorted(set(TV_LENS) | {k * 1024 + d for k in TREE_LEAVES for d in (-1, 0, 1)})


def small_cases():
    """[(off, n)] in fixture order: every length at offset 0, then at 1, 5 and 15."""
    return [(off, n) for off in SMALL_OFFS for n in SMALL_LENS]


def tree_cases():
    """[(off, n)] in fixture order."""
    return [(TREE_OFF, n) for n in tree_lens()]


def small_source():
    return splitmix_bytes(SMALL_SEED, SMALL_BYTES)


def tree_source():
    return splitmix_bytes(TREE_SEED, TREE_BYTES)


assert len(SMALL_LENS) == 410 and len(small_cases()) == 1640
assert SMALL_LENS[-1] + max(SMALL_OFFS) <= SMALL_BYTES


def digests(fixture, group):
    """The 32-byte digests of one group ('small' or 'tree') of the loaded fixture, in case order."""
    raw = bytes.fromhex(fixture[group])
    n = len(small_cases() if group == "small" else tree_cases())
    assert len(raw) == 32 * n, (group, len(raw), n)
    return [raw[32 * i:32 * i + 32] for i in range(n)]
