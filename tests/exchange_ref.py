"""Plain numpy / Python reference of the digest exchange's partition, gate and scatter steps
(backuwup_amd/sharded.py, steps 2, 4 and 5), and the digest sets the kernel tests feed them.

Written from the definition, not from the kernels: a digest belongs to the owner named by the
top log2(n_owners) bits of its first byte, each owner receives its digests in canonical (input)
order, and a gate decides a digest a duplicate iff the index has seen it before.  Everything is
whole-array numpy (boolean masks and flatnonzero), so there are no blocks, chunks or scans here
for a kernel's geometry to hide in.
"""
import numpy as np

OWNER_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
UNTOUCHED = -1  # perm value of a bucket slot that the partition must leave alone


def _bits(n_owners):
    n = int(n_owners)
    if n < 1 or n > 256 or n & (n - 1):
        raise ValueError("n_owners must be a power of two in [1, 256], got %r" % (n_owners,))
    return n.bit_length() - 1


def _rows(digests, n=None):
    d = np.asarray(digests, dtype=np.uint8).reshape(-1, 32)
    return d if n is None else d[:int(n)]


def owner_of(digests, n_owners):
    """Owner of every digest: d[0] >> (8 - log2 n_owners), and 0 for one owner."""
    bits = _bits(n_owners)
    first = _rows(digests)[:, 0].astype(np.int64)
    return first >> (8 - bits) if bits else np.zeros(len(first), dtype=np.int64)


def partition(digests, n, n_owners):
    """The stable partition of the first n digests -> (per-owner index arrays in canonical
    order, counts)."""
    own = owner_of(_rows(digests, n), n_owners)
    lists = [np.flatnonzero(own == o).astype(np.int64) for o in range(n_owners)]
    return lists, np.array([len(x) for x in lists], dtype=np.int64)


def buckets(digests, n, n_owners, cap):
    """Fixed-capacity owner buckets -> (bytes [n_owners][cap][32], perm [n_owners][cap], counts,
    overflowed).  The first `cap` digests of each owner are placed and the counts clamped to cap;
    perm is UNTOUCHED (and the bytes zero) in every slot that receives nothing."""
    d = _rows(digests, n)
    lists, counts = partition(d, n, n_owners)
    out = np.zeros((n_owners, cap, 32), dtype=np.uint8)
    perm = np.full((n_owners, cap), UNTOUCHED, dtype=np.int64)
    for o, idx in enumerate(lists):
        kept = idx[:cap]
        out[o, :len(kept)] = d[kept]
        perm[o, :len(kept)] = kept
    return out, perm, np.minimum(counts, cap), bool((counts > cap).any())


def sections(digests, n, n_owners):
    """The owner sections back to back, as bw_exchange_dedup lays them out -> (bytes [n][32],
    perm [n], msg [2 * n_owners]) with msg[2o] = owner o's count and msg[2o + 1] = the largest
    count."""
    d = _rows(digests, n)
    lists, counts = partition(d, n, n_owners)
    perm = np.concatenate(lists) if len(d) else np.zeros(0, dtype=np.int64)
    msg = np.zeros(2 * n_owners, dtype=np.int64)
    msg[0::2] = counts
    msg[1::2] = counts.max()
    return d[perm], perm, msg


def gate(bucket_bytes, counts, index, fill=7):
    """Source-major verdicts of received buckets over `index` (an oracle.Index: anything with
    is_blob_duplicate and insert) -> uint8 [n_src][cap]; slots beyond counts[s] hold `fill`."""
    b = np.asarray(bucket_bytes, dtype=np.uint8)
    n_src = len(counts)
    b = b.reshape(n_src, -1, 32)
    v = np.full(b.shape[:2], fill, dtype=np.uint8)
    for s in range(n_src):
        for k in range(int(counts[s])):
            key = b[s, k].tobytes()
            v[s, k] = 1 if index.is_blob_duplicate(key) else 0
            index.insert(key)
    return v


# ------------------------------------------------------------------ digest sets (n x 32 bytes)

KINDS = ("uniform", "one-owner", "edges", "striped", "blocky")


def _with_repeats(d, rng, by_first_byte):
    """About a third of the rows become whole-row repeats of an earlier row; with by_first_byte,
    of an earlier row with the same first byte, so a patterned set keeps its owner pattern."""
    first = d[:, 0]
    groups = [np.flatnonzero(first == v) for v in np.unique(first)] if by_first_byte else [np.arange(len(d))]
    for idx in groups:
        take = rng.random(len(idx)) < 1 / 3
        src = (rng.random(len(idx)) * np.arange(len(idx))).astype(np.int64)
        for j in np.flatnonzero(take):  # increasing: a repeat of a repeat repeats the original
            if j:
                d[idx[j]] = d[idx[src[j]]]
    return d


def digest_set(kind, n, n_owners, seed=0, first=0x00, run=4096, skew=0):
    """n digests of one of the five patterns, about a third of them repeats of earlier rows.
      uniform    random bytes
      one-owner  first byte constant (`first`)
      edges      first bytes only from {k * 2^shift - 1, k * 2^shift} for the owner count
      striped    the owner changes with every item
      blocky     runs of `run` items for one owner, the first run shortened by `skew`"""
    rng = np.random.default_rng([seed, n, n_owners, KINDS.index(kind)])
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if n == 0:
        return d
    bits = _bits(n_owners)
    shift = 8 - bits
    i = np.arange(n, dtype=np.int64)
    if kind == "uniform":
        pass
    elif kind == "one-owner":
        d[:, 0] = first
    elif kind == "edges":
        k = np.arange(0, n_owners + 1, dtype=np.int64) << shift
        vals = np.unique(np.concatenate([k - 1, k]))
        vals = vals[(vals >= 0) & (vals <= 255)]
        d[:, 0] = vals[rng.integers(0, len(vals), n)]
    elif kind == "striped":
        owner = (i * 37 + 11) % n_owners  # 37 is odd: a permutation of the owners, one per item
        low = (i // n_owners) % min(3, 1 << shift)  # below the owner bits
        d[:, 0] = (owner << shift) | low if n_owners > 1 else i % 5
    elif kind == "blocky":
        owner = (((i + skew) // run) * 5 + 3) % n_owners
        d[:, 0] = (owner << shift) | (i % 2 if shift else 0)
    else:
        raise ValueError(kind)
    return _with_repeats(d, rng, by_first_byte=kind != "uniform")
