"""tests/exchange_ref.py (the reference the exchange kernels are pinned to, test_gpu_exchange_kernels.py)
against the project's other CPU statements of the same steps: backuwup_amd.sharded.owner_of and the
CpuShardOps stand-in of test_sharded.py, on the same inputs at every owner count.  No GPU."""
import numpy as np
import pytest
import torch

import exchange_ref as R
from backuwup_amd.sharded import owner_of
from test_sharded import CpuShardOps


def test_owner_of_agrees_on_every_first_byte():
    d = np.zeros((256, 32), dtype=np.uint8)
    d[:, 0] = np.arange(256)
    for w in R.OWNER_COUNTS:
        want = [owner_of(b, w) for b in range(256)]
        got = R.owner_of(d, w)
        assert got.tolist() == want, w
        assert got.min() == 0 and got.max() == w - 1 and (np.diff(got) >= 0).all()
        assert (np.bincount(got, minlength=w) == 256 // w).all()  # equal prefix ranges
    for bad in (0, 3, 512):
        with pytest.raises(ValueError):
            R.owner_of(d, bad)


@pytest.mark.parametrize("kind", R.KINDS)
def test_digest_sets_are_what_they_say(kind):
    for w in (1, 8, 256):
        d = R.digest_set(kind, 9000, w, first=0x80, skew=1)
        assert d.shape == (9000, 32) and d.dtype == np.uint8
        uniq = len(np.unique(d, axis=0))
        assert 0.55 * 9000 < uniq < 0.8 * 9000, (w, uniq)  # about a third are repeats
        own = R.owner_of(d, w)
        shift = 8 - (w.bit_length() - 1)
        if kind == "one-owner":
            assert (d[:, 0] == 0x80).all()
        if kind == "edges":
            lo = d[:, 0].astype(int) % (1 << shift)
            assert np.isin(lo, [0, (1 << shift) - 1]).all()
        if kind == "striped" and w > 1:
            assert (np.diff(own) != 0).all()
        if kind == "blocky":
            cuts = np.flatnonzero(np.diff(own)) + 1
            assert w == 1 or cuts.tolist() == [4095, 8191]  # misaligned by one to the 4096 block


@pytest.mark.parametrize("w", R.OWNER_COUNTS)
def test_partition_buckets_and_scatter_agree_with_the_cpu_ops(w):
    for kind in R.KINDS:
        n = 777
        d = R.digest_set(kind, n, w, seed=w, first=0xff, run=100, skew=1)
        lists, counts = R.partition(d, n, w)
        assert sorted(np.concatenate(lists).tolist()) == list(range(n)) and counts.sum() == n
        assert all((np.diff(x) > 0).all() for x in lists)  # canonical order inside each section
        cap = int(counts.max())
        ops = CpuShardOps()
        batch = (n, torch.from_numpy(d.reshape(-1).copy()), torch.zeros(n, dtype=torch.uint8), n)
        b2, p2, c2 = (t.numpy() for t in ops.partition(batch, cap, w))
        b1, p1, c1, ovf = R.buckets(d, n, w, cap)
        assert not ovf and np.array_equal(c1, c2) and np.array_equal(c1, counts)
        placed = p1 != R.UNTOUCHED
        assert np.array_equal(placed, np.arange(cap)[None, :] < counts[:, None])
        assert np.array_equal(b1[placed], b2.reshape(w, cap, 32)[placed])
        assert np.array_equal(p1[placed], p2.reshape(w, cap)[placed])
        assert (b1[~placed] == 0).all()
        # sections: the same lists back to back
        sec, sperm, msg = R.sections(d, n, w)
        assert np.array_equal(sperm, p1[placed]) and np.array_equal(sec, b1[placed])
        assert np.array_equal(msg[0::2], counts) and (msg[1::2] == counts.max()).all()
        # a prefix only: the digests past n do not count
        assert R.partition(d, 100, w)[1].sum() == 100
        # overflow: clamped, the first cap - 1 of every owner, flagged
        if cap > 1:
            b3, p3, c3, ovf3 = R.buckets(d, n, w, cap - 1)
            assert ovf3 and np.array_equal(c3, np.minimum(counts, cap - 1))
            assert np.array_equal(p3, p1[:, :cap - 1]) and np.array_equal(b3, b1[:, :cap - 1])


@pytest.mark.parametrize("w", R.OWNER_COUNTS)
def test_gate_agrees_with_the_cpu_ops(w, oracle):
    """One rank's owner role: buckets from w sources, two calls on one shard; the verdicts are
    those of CpuShardOps.decide (a Python set), and scattered back they are one index's."""
    ix, ops = oracle.Index(), CpuShardOps()
    for call in range(2):
        cap = 40
        rng = np.random.default_rng([w, call])
        counts = rng.integers(0, cap + 1, w)
        counts[0], counts[-1] = (cap, 0) if w > 1 else (cap, cap)
        pool = np.random.default_rng(5).integers(0, 256, (60, 32), dtype=np.uint8)  # shared: repeats
        recv = pool[rng.integers(0, 60, (w, cap))]
        want = ops.decide(torch.from_numpy(recv.reshape(-1).copy()), torch.from_numpy(counts), w, cap).numpy()
        got = R.gate(recv, counts, ix, fill=7)
        live = np.arange(cap)[None, :] < counts[:, None]
        assert np.array_equal(got[live], want.reshape(w, cap)[live]) and (got[~live] == 7).all()
        assert got[live].sum() > 0
