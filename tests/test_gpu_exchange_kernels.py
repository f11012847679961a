"""The digest exchange's partition, gate and scatter kernels (backuwup_amd/csrc/bw_dedup.hip:
k_partition, k_bucket_pass<false/true>, k_bucket_top, k_owner_top, k_bucket_gather in both modes,
k_bucket_scatter, k_scatter, k_owner_scatter) against the plain reference of tests/exchange_ref.py.

Every other exchange test reaches these kernels through verdicts only, with one 4096-digest scan
block per rank and at most eight owners.  Here the outputs themselves are read (bucket bytes, perm,
counts, verdict slots), at sizes on both sides of every block boundary, at every owner count the ABI
promises, with digest sets built to make a wrong partition visible (empty owners, one owner, owner
boundaries, an owner change with every item, whole blocks of one owner), and every output buffer is
filled with a canary first so that a byte written where none belongs shows.  All comparisons are
exact.
"""
import numpy as np
import pytest

import exchange_ref as R
from backuwup_amd._lib import BW_EINVAL, BW_ENOSPC, BwError

pytestmark = pytest.mark.gpu

BLK = 4096            # digests per block of the bucket passes
CANARY = 0xA5         # every byte of an output buffer before the call
CANARY64 = np.frombuffer(bytes([CANARY]) * 8, dtype=np.int64)[0]
V_CANARY = 7          # verdict / is_dup bytes before the call
GUARD = 64            # slots behind every output that must stay untouched
ONE_OWNER_FIRST = (0x00, 0x7f, 0x80, 0xff)

N_BUCKETS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 5, 20000)
BUCKET_CASES = sorted({(n, w) for n in N_BUCKETS for w in (1, 8, 256)} |
                      {(n, w) for n in (4097, 20000) for w in R.OWNER_COUNTS})


@pytest.fixture
def dev(ctx):
    """The shared context on a torch stream of this test, so that uploads, the library's kernels
    and the read-backs are ordered; its own stream again afterwards."""
    import torch
    st = torch.cuda.Stream()
    ctx.set_stream(st.cuda_stream)
    try:
        with torch.cuda.stream(st):
            ctx.index_reset()
            yield torch
            st.synchronize()
    finally:
        ctx.set_stream(0)


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filled(torch, nbytes, value=CANARY):
    return torch.full((int(nbytes),), value, dtype=torch.uint8, device="cuda")


def host(t, dtype=np.uint8):
    return t.cpu().numpy().view(dtype)


def digest_sets(n, w, seed=0):
    """(label, digests) for the five kinds; one-owner at each of its four first bytes, blocky
    aligned and misaligned by one to the block size."""
    for kind in R.KINDS:
        if kind == "one-owner":
            for f in ONE_OWNER_FIRST:
                yield "%s-%02x" % (kind, f), R.digest_set(kind, n, w, seed=seed, first=f)
        elif kind == "blocky":
            for skew in (0, 1):
                yield "%s-%d" % (kind, skew), R.digest_set(kind, n, w, seed=seed, run=BLK, skew=skew)
        else:
            yield kind, R.digest_set(kind, n, w, seed=seed)


def padded(d, max_n, seed=99):
    """The digest array of a batch bounded by max_n: n real rows, then rows that are NOT part of
    the batch (random, so reading one changes a count)."""
    tail = np.random.default_rng(seed).integers(0, 256, (max_n - len(d), 32), dtype=np.uint8)
    return np.concatenate([d, tail])


def run_buckets(ctx, torch, d_all, n, max_n, w, cap):
    """bw_partition_buckets over canary-filled outputs -> device (bytes, perm, counts), guards included."""
    d_dev = up(torch, d_all) if max_n else filled(torch, 32)
    d_n = up(torch, np.array([n], dtype=np.int64))
    b = filled(torch, (w * cap + GUARD) * 32)
    p = filled(torch, (w * cap + GUARD) * 8)
    c = filled(torch, (w + GUARD) * 8)
    ctx.partition_buckets(d_dev.data_ptr(), d_n.data_ptr(), max_n, cap, w, b.data_ptr(), p.data_ptr(), c.data_ptr())
    return b.view(-1, 32), p.view(torch.int64), c.view(torch.int64)


def check_buckets(torch, got, d, n, w, cap, what):
    """The whole output buffers against the reference: counts, the placed slots' bytes and perm,
    and the canary in every other slot and in the guards.  The buffers are compared on the device
    (256 owners x 20 000 slots are 164 MB of mostly canaries); only a mismatch is read back.
    -> whether the reference overflowed."""
    wb, wp, wc, ovf = R.buckets(d, n, w, cap)
    idx = np.flatnonzero(wp.reshape(-1) != R.UNTOUCHED)
    assert idx.size == wc.sum()
    eb = filled(torch, (w * cap + GUARD) * 32).view(-1, 32)
    ep = filled(torch, (w * cap + GUARD) * 8).view(torch.int64)
    if idx.size:
        at = up(torch, idx)
        eb[at] = up(torch, wb.reshape(-1, 32)[idx])
        ep[at] = up(torch, wp.reshape(-1)[idx])
    ec = np.full(w + GUARD, CANARY64, dtype=np.int64)
    ec[:w] = wc
    gc = host(got[2], np.int64)
    assert np.array_equal(gc, ec), (what, "counts", gc[:w][gc[:w] != wc][:8], wc[gc[:w] != wc][:8])
    for name, g, e in (("perm", got[1], ep), ("bytes", got[0], eb)):
        if not torch.equal(g, e):
            g, e = g.cpu().numpy(), e.cpu().numpy()
            bad = np.flatnonzero((g != e).reshape(len(g), -1).any(axis=1))
            raise AssertionError("%s: %s differ in %d slots of %d x %d (+%d guard), first at %d: got %s want %s"
                                 % (what, name, len(bad), w, cap, GUARD, bad[0], g[bad[0]], e[bad[0]]))
    return ovf


def n_modes(n):
    """(label, max_n) for *d_n equal to max_n, below it inside the same block (when n is a multiple
    of the block size, the smallest bound above it), and below it by more than two whole blocks."""
    room = (-n) % BLK
    return (("equal", n), ("same-block", n + (min(7, room) if room else 7)), ("two-blocks", n + 2 * BLK + 17))


def stale_blk(ctx, torch, d_all, max_n, w):
    """A larger call on the context first: every block's totals of all max_n rows, scanned, stay in
    the context's scratch; the smaller call that follows must not read the blocks past its *d_n.
    (cap 0: nothing is placed; the overflow this reports is cleared by the reset.)"""
    c = filled(torch, w * 8)
    d_dev, d_n = up(torch, d_all), up(torch, np.array([max_n], dtype=np.int64))
    ctx.partition_buckets(d_dev.data_ptr(), d_n.data_ptr(), max_n, 0, w, 0, 0, c.data_ptr())
    assert (host(c, np.int64) == 0).all()  # clamped to cap
    ctx.index_reset()


# ------------------------------------------------------------------ bw_partition_buckets

@pytest.mark.parametrize("n,w", BUCKET_CASES)
def test_partition_buckets_matches_reference(ctx, dev, n, w):
    for label, d in digest_sets(n, w):
        cap = int(R.partition(d, n, w)[1].max())  # the largest count: no overflow
        for mode, max_n in n_modes(n):
            d_all = padded(d, max_n)
            if mode == "two-blocks":
                stale_blk(ctx, dev, d_all, max_n, w)
            got = run_buckets(ctx, dev, d_all, n, max_n, w, cap)
            assert not check_buckets(dev, got, d, n, w, cap, (label, mode, cap))
            ctx.index_check()  # no overflow reported
        if cap >= 1:  # one below the largest count: clamped, bounded, reported
            got = run_buckets(ctx, dev, d, n, n, w, cap - 1)
            assert check_buckets(dev, got, d, n, w, cap - 1, (label, "overflow", cap - 1))
            with pytest.raises(BwError) as e:
                ctx.index_check()
            assert e.value.rc == BW_ENOSPC
            ctx.index_reset()


@pytest.mark.parametrize("n,w,kind", [(4097, 4, "uniform"), (3 * BLK + 5, 2, "striped"), (20000, 8, "blocky"),
                                      (8193, 1, "uniform"), (4097, 256, "one-owner")])
def test_bucket_overflow_is_reported_bounded_and_sticky(ctx, dev, n, w, kind):
    d = R.digest_set(kind, n, w, seed=3, first=0x80, skew=1)
    counts = R.partition(d, n, w)[1]
    big = int(counts.max())
    for cap in sorted({big - 1, big // 2, 1, 0}):
        # clamped counts, exactly the first cap digests of each owner in order, nothing past any bucket
        assert (R.buckets(d, n, w, cap)[2] == np.minimum(counts, cap)).all()
        assert check_buckets(dev, run_buckets(ctx, dev, d, n, n, w, cap), d, n, w, cap, ("overflow", cap))
        with pytest.raises(BwError) as e:
            ctx.index_check()
        assert e.value.rc == BW_ENOSPC
        # sticky: a clean call does not clear it
        assert not check_buckets(dev, run_buckets(ctx, dev, d, n, n, w, big), d, n, w, big, ("clean", big))
        with pytest.raises(BwError) as e:
            ctx.index_check()
        assert e.value.rc == BW_ENOSPC
        # after a reset the same call with enough room is clean again
        ctx.index_reset()
        assert not check_buckets(dev, run_buckets(ctx, dev, d, n, n, w, big), d, n, w, big, ("reset", big))
        ctx.index_check()


# ------------------------------------------------------------------ bw_partition_by_owner

@pytest.mark.parametrize("w", [1, 2, 16, 256])
def test_partition_by_owner_matches_reference(ctx, dev, w):
    for n in (0, 1, 1023, 1024, 1025, 2047, 5000):
        for label, d in digest_sets(n, w, seed=1):
            sec, perm, msg = R.sections(d, n, w)
            d_dev = up(dev, padded(d, n + 3))  # rows past n are not part of the call
            out = filled(dev, (n + GUARD) * 32)
            p = filled(dev, (n + GUARD) * 8)
            counts = ctx.partition_by_owner(d_dev.data_ptr(), n, w, out.data_ptr(), p.data_ptr())
            assert counts.astype(np.int64).tolist() == msg[0::2].tolist(), (n, label)
            eo = np.full((n + GUARD, 32), CANARY, dtype=np.uint8)
            ep = np.full(n + GUARD, CANARY64, dtype=np.int64)
            eo[:n], ep[:n] = sec, perm
            assert np.array_equal(host(p, np.int64), ep), (n, label)
            assert np.array_equal(host(out).reshape(-1, 32), eo), (n, label)


@pytest.mark.parametrize("bad", [0, 3, 512])
def test_partition_by_owner_rejects_invalid_owner_counts(ctx, dev, bad):
    d = up(dev, R.digest_set("uniform", 64, 1))
    out, p = filled(dev, 64 * 32), filled(dev, 64 * 8)
    with pytest.raises(BwError) as e:
        ctx.partition_by_owner(d.data_ptr(), 64, bad, out.data_ptr(), p.data_ptr())
    assert e.value.rc == BW_EINVAL
    assert (host(out) == CANARY).all() and (host(p) == CANARY).all()


# ------------------------------------------------------------------ the two scatters

def test_scatter_verdicts_counted_slots_only(ctx, dev):
    n, w = 5000, 16
    rng = np.random.default_rng(41)
    for label, d in digest_sets(n, w, seed=2):
        perm = R.sections(d, n, w)[1]
        verdict = rng.integers(0, 256, n, dtype=np.uint8)
        v_dev, p_dev = up(dev, verdict), up(dev, perm)
        for m in (0, 1, 255, 256, 257, n):
            dst = filled(dev, n + GUARD, V_CANARY)
            ctx.scatter_verdicts(v_dev.data_ptr(), p_dev.data_ptr(), m, dst.data_ptr())
            want = np.full(n + GUARD, V_CANARY, dtype=np.uint8)
            want[perm[:m]] = verdict[:m]  # the entries no counted slot names keep the canary
            assert np.array_equal(host(dst), want), (label, m)


@pytest.mark.parametrize("n,w", [(1, 1), (4097, 1), (4097, 8), (5000, 256), (777, 64)])
def test_scatter_buckets_counted_slots_only(ctx, dev, n, w):
    rng = np.random.default_rng([43, n, w])
    for label, d in digest_sets(n, w, seed=3):
        big = int(R.partition(d, n, w)[1].max())
        for cap in sorted({big, big + 3, max(big - 1, 0), big // 2}):  # exact, slack, clamped
            _, perm, counts, _ = R.buckets(d, n, w, cap)
            live = perm != R.UNTOUCHED
            # a slot beyond its bucket's count names the trap entry n: in bounds, and checked below
            perm_dev = np.where(live, perm, n)
            verdict = rng.integers(0, 256, (w, cap), dtype=np.uint8)
            dst = filled(dev, n + GUARD, V_CANARY)
            v_dev, p_dev, c_dev = up(dev, verdict), up(dev, perm_dev), up(dev, counts)
            ctx.scatter_buckets(v_dev.data_ptr() if cap else 0, p_dev.data_ptr() if cap else 0, c_dev.data_ptr(), w,
                                cap, dst.data_ptr())
            want = np.full(n + GUARD, V_CANARY, dtype=np.uint8)
            want[perm[live]] = verdict[live]  # blobs of a clamped bucket's tail keep the canary
            assert np.array_equal(host(dst), want), (label, cap)


# ------------------------------------------------------------------ bw_index_check_insert_buckets

def gate_counts(rng, n_src, cap, call):
    """Counts with 0 and cap among them; a few full buckets and small ones, so the reference's
    Python loop stays short at 64 x 4097 slots."""
    c = np.minimum(rng.integers(0, 301, n_src), cap)
    c[rng.integers(0, n_src, max(n_src // 8, 1))] = cap
    if n_src > 1:
        c[call % n_src] = cap
        c[(call + 1) % n_src] = 0
    else:
        c[0] = (cap, 0, cap // 2 + 1)[call]
    return c.astype(np.int64)


@pytest.mark.parametrize("n_src", [1, 2, 8, 64])
@pytest.mark.parametrize("cap", [1, 300, 4097])
def test_gate_buckets_matches_reference(ctx, dev, oracle, n_src, cap):
    ctx.index_reset(16)  # the table grows and rehashes under counts only the device knows
    ix, seen = oracle.Index(), set()
    rng = np.random.default_rng([47, n_src, cap])
    pool = rng.integers(0, 256, (max(n_src * min(cap, 600), 8), 32), dtype=np.uint8)
    for call in range(3):
        counts = gate_counts(rng, n_src, cap, call)
        # every slot, counted or not, draws from the pool: the same digest in several sources and
        # calls, and a slot beyond its count that is gated by mistake changes a later verdict
        recv = pool[rng.integers(0, len(pool), (n_src, cap))]
        v = filled(dev, n_src * cap + GUARD, V_CANARY)
        r_dev, c_dev = up(dev, recv), up(dev, counts)
        ctx.index_check_insert_buckets(r_dev.data_ptr(), c_dev.data_ptr(), n_src, cap, v.data_ptr())
        want = np.full(n_src * cap + GUARD, V_CANARY, dtype=np.uint8)
        want[:n_src * cap] = R.gate(recv, counts, ix, fill=V_CANARY).reshape(-1)
        got = host(v)
        assert np.array_equal(got, want), (call, np.flatnonzero(got != want)[:8], counts[:8])
        live = np.arange(cap)[None, :] < counts[:, None]
        seen.update(x.tobytes() for x in recv[live])
        assert ctx.index_size() == len(seen), call
        ctx.index_check()
        assert cap < 300 or call or counts.sum() > 256  # more than one block of the verdict pass


# ------------------------------------------------------------------ the whole chain in one process

@pytest.mark.parametrize("world", [2, 4])
def test_exchange_chain_matches_one_index(oracle, world):
    """partition_buckets -> transpose (the all-to-all) -> index_check_insert_buckets -> transpose
    back -> scatter_buckets, with `world` contexts on device 0 as the ranks, each gating its own
    index; every verdict equals one index over the canonical order (batch, rank, position)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from backuwup_amd import Context
    sizes = (9000, 4097)
    cap = max(sizes)
    pool = np.random.default_rng(53).integers(0, 256, (6000, 32), dtype=np.uint8)  # cross-rank repeats

    def batch_digests(b, r):
        rng = np.random.default_rng([59, b, r])
        own = rng.integers(0, 256, (sizes[b], 32), dtype=np.uint8)
        pick = rng.random(sizes[b])
        d = np.where((pick < 0.4)[:, None], pool[rng.integers(0, len(pool), sizes[b])], own)
        rep = np.flatnonzero(pick > 0.8)
        rep = rep[rep > 0]
        d[rep] = d[(rng.random(len(rep)) * rep).astype(np.int64)]  # in-batch repeats
        return d

    st = torch.cuda.Stream()
    ctxs = [Context(0) for _ in range(world)]
    try:
        with torch.cuda.stream(st):
            for c in ctxs:
                c.set_stream(st.cuda_stream)
                c.index_reset(16)
            ix = oracle.Index()
            for b, n in enumerate(sizes):
                max_n = n + (2 * BLK + 17) * (b == 1)  # the second batch ends two blocks below its bound
                ds = [batch_digests(b, r) for r in range(world)]
                bk, pm, ct = [], [], []
                for r, c in enumerate(ctxs):
                    bk.append(filled(torch, world * cap * 32))
                    pm.append(filled(torch, world * cap * 8))
                    ct.append(filled(torch, world * 8))
                    d_dev, d_n = up(torch, padded(ds[r], max_n)), up(torch, np.array([n], dtype=np.int64))
                    c.partition_buckets(d_dev.data_ptr(), d_n.data_ptr(), max_n, cap, world, bk[r].data_ptr(),
                                        pm[r].data_ptr(), ct[r].data_ptr())
                sent = np.stack([host(x).reshape(world, cap, 32) for x in bk])  # [source][owner]
                cnt = np.stack([host(x, np.int64) for x in ct])
                assert (cnt.sum(axis=1) == n).all()
                for r in range(world):  # before any kernel scatters through it: perm names blobs of the batch
                    live = np.arange(cap)[None, :] < cnt[r][:, None]
                    p = host(pm[r], np.int64).reshape(world, cap)
                    assert np.array_equal(p[live], R.buckets(ds[r], n, world, cap)[1][live]), (b, r)
                recv, rcnt = sent.transpose(1, 0, 2, 3), cnt.T  # [owner][source]
                vd = []
                for r, c in enumerate(ctxs):
                    vd.append(filled(torch, world * cap, V_CANARY))
                    r_dev, c_dev = up(torch, recv[r]), up(torch, rcnt[r])
                    c.index_check_insert_buckets(r_dev.data_ptr(), c_dev.data_ptr(), world, cap, vd[r].data_ptr())
                back = np.stack([host(x).reshape(world, cap) for x in vd]).transpose(1, 0, 2)  # [source][owner]
                for r, c in enumerate(ctxs):
                    dup = filled(torch, max_n + GUARD, V_CANARY)
                    b_dev = up(torch, back[r])
                    c.scatter_buckets(b_dev.data_ptr(), pm[r].data_ptr(), ct[r].data_ptr(), world, cap, dup.data_ptr())
                    got = host(dup)
                    want = []
                    for x in ds[r]:
                        k = x.tobytes()
                        want.append(int(ix.is_blob_duplicate(k)))
                        ix.insert(k)
                    assert np.array_equal(got[:n], np.array(want, dtype=np.uint8)), (b, r)
                    assert (got[n:] == V_CANARY).all(), (b, r)
                    assert 0 < sum(want) < n
            for c in ctxs:
                c.index_check()
            st.synchronize()
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------ bw_exchange_dedup past one block

@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def tiny_files(n_files, seed, ids=None):
    """n_files files of 8 bytes, a third of them copies of an earlier file: one blob each, so a
    batch's blob count is its file count.  ids: the distinct contents to draw from."""
    rng = np.random.default_rng(seed)
    src = np.arange(n_files)
    rep = np.flatnonzero(rng.random(n_files) < 1 / 3)
    rep = rep[rep > 0]
    for j in rep:
        src[j] = src[int(rng.random() * j)]
    content = (np.arange(n_files, dtype="<u8") + (np.uint64(seed) << np.uint64(32))) if ids is None else ids[:n_files]
    data = np.ascontiguousarray(content[src]).view(np.uint8)
    offs = np.arange(n_files, dtype=np.uint64) * np.uint64(8)
    return data, offs, np.full(n_files, 8, dtype=np.uint64)


def assert_session_batches(oracle, session, data, offs, lens, batches):
    ix = oracle.Index()
    for lo, hi in batches:
        got = session.process_files(data, offs[lo:hi], lens[lo:hi])
        want = oracle.process_files(data, offs[lo:hi], lens[lo:hi], index=ix, threads=8)
        for f in ("file", "offset", "length", "gear_hash", "is_dup"):
            assert np.array_equal(got[f], want[f]), (lo, hi, f)
        assert np.array_equal(got["digest"], want["digest"]), (lo, hi)
    return want


@pytest.mark.parametrize("world", [2, 4, 8, 16])
def test_node_session_past_one_block(gpu, oracle, world):
    """bw_exchange_dedup (k_bucket_pass with sections back to back, k_owner_top, k_owner_scatter)
    with more than two 4096-blob blocks per rank, then a batch of 3 files (ranks without any: the
    contexts' block scratch keeps the large batch's totals), then sizes in between.

    World 16 fits one device: a context allocates only what its batches need (every buffer of
    bw_ctx.h is sized by `ensure` from the batch's bounds, none at creation).  With ~9000 one-blob
    files of 8 bytes per rank that is 13 per-blob arrays and the records, digests and sections
    (under 250 bytes per blob: ~2.3 MB), the index (2^16 log entries of 32 B and 2^17 table words:
    3 MiB) and a few dozen buffers of a few KiB; even at one 2 MiB allocation granule for each of a
    context's ~70 device buffers it is under 150 MiB per rank, 2.4 GiB for sixteen of the 288 GB.
    The staging ring is pinned host memory (one 80 MiB chunk per rank)."""
    from backuwup_amd.session import NodeSession
    per = 9001
    n = world * per + 5
    data, offs, lens = tiny_files(n, seed=61 + world)
    batches = [(0, n), (7, 10), (n // 3, n // 3 + world * 5000), (0, world * 4097), (n - 2, n)]
    with NodeSession([0] * world, transport="local") as s:
        want = assert_session_batches(oracle, s, data, offs, lens, batches)
    assert want["is_dup"].all()


def test_node_session_rccl_world1_past_one_block(gpu, oracle):
    from backuwup_amd.session import NodeSession
    data, offs, lens = tiny_files(12289, seed=67)
    with NodeSession([0], transport="rccl") as s:
        want = assert_session_batches(oracle, s, data, offs, lens, [(0, 4097), (0, 12289), (4000, 4003)])
    assert want["is_dup"].all()


def test_node_session_every_blob_for_the_last_owner(gpu, oracle):
    """World 4, every digest's first byte >= 0xC0: three ranks send three empty sections and
    receive nothing, and the last owner gates every blob of every rank."""
    from backuwup_amd.session import NodeSession
    n = 4 * 4200
    ids, k = [], 0
    while len(ids) < n:
        c = np.array([k + (71 << 32)], dtype="<u8")
        if oracle.blake3(c.tobytes())[0] >= 0xC0:
            ids.append(c[0])
        k += 1
    data, offs, lens = tiny_files(n, seed=73, ids=np.array(ids, dtype="<u8"))
    with NodeSession([0] * 4, transport="local") as s:
        ix = oracle.Index()
        got = s.process_files(data, offs, lens)
        want = oracle.process_files(data, offs, lens, index=ix, threads=8)
        assert (want["digest"][:, 0] >= 0xC0).all() and len(want) == n
        assert np.array_equal(got["digest"], want["digest"]) and np.array_equal(got["is_dup"], want["is_dup"])
        assert 0 < want["is_dup"].sum() < n
        # the other owners' shards stayed empty
        assert [c.index_size() for c in s.ctxs] == [0, 0, 0, int((want["is_dup"] == 0).sum())]
        # and a mixed batch behind it on the same session
        d2, o2, l2 = tiny_files(9000, seed=79)
        got = s.process_files(d2, o2, l2)
        want = oracle.process_files(d2, o2, l2, index=ix, threads=8)
        assert np.array_equal(got["digest"], want["digest"]) and np.array_equal(got["is_dup"], want["is_dup"])
