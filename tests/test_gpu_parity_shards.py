"""Parity shards on the GPU (backuwup_amd.parity over bw_parity_build(_device), bw_parity_repair(_device),
k_gf_matmul) against tests/parity_ref.py: every parity shard and digest of stores with unequal packfiles,
every erasure pattern of a (4, 2) group with exact statuses, damaged survivors with and without digests,
the whole protect -> damage -> check -> repair_store -> check loop over a real store, and a fuzz.
(tests/test_gpu_parity.py is about agreement with the oracle, not about this.)"""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import parity_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

W = 2048  # bw_internal.h GF_WAVE_BYTES
CANARY = 0xC3
OK, DAMAGED, REBUILT, REBUILT_BAD, LOST = 0, 1, 2, 3, 4


def _packs(seed, sizes):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, 256, n, dtype=np.uint8).tobytes() for n in sizes]  # no zero byte: a tail shows


def _hash(ctx, packs):
    from backuwup_amd import blake3
    return [bytes(blake3.hash(p, ctx)) for p in packs]


# ---------------------------------------------------------------- build
@pytest.mark.parametrize("sizes,k,m", [([1, 17, W - 1, W, W + 1, 5000, 16, 3 * W + 5, 900, 33, 2 * W], 4, 2),
                                       ([700, 1, 64], 8, 3), ([W + 9] * 5, 1, 1), ([40, 50, 60, 70], 2, 9)])
def test_build_equals_the_reference(ctx, sizes, k, m):
    """Groups of unequal members, several groups in one launch, the short last group; both forms."""
    import torch
    from backuwup_amd import parity
    packs = _packs(600 + k, sizes)
    want, wgroups = pr.encode(packs, k, m)
    groups, total = parity.plan(sizes, k, m)
    tab = parity._table(sizes)
    data = np.frombuffer(b"".join(packs), dtype=np.uint8)
    out, dig = parity.build(ctx, data, tab, groups, total)
    d_pf = torch.from_numpy(data.copy()).cuda()
    d_out = torch.full((total + 32,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch's stream is not the context's
    dig_d = parity.build_device(ctx, d_pf.data_ptr(), tab, groups, d_out.data_ptr(), total)
    torch.cuda.synchronize()
    assert np.array_equal(d_pf.cpu().numpy(), data), "bw_parity_build_device wrote the packfiles"
    dev = d_out.cpu().numpy()
    assert (dev[total:] == CANARY).all()
    assert np.array_equal(dev[:total], out)
    got, want_dig, at = [], [], 0
    for (first, kk, mm, length, off), g in zip(wgroups, groups):
        assert (first, kk, mm, length, off) == tuple(int(g[f]) for f in ("first_packfile", "k", "m", "shard_len", "out_offset"))
        got += [out[off + i * length:off + (i + 1) * length].tobytes() for i in range(mm)]
        want_dig += packs[first:first + kk] + want[at:at + mm]
        at += mm
    assert got == want
    assert [bytes(d) for d in dig] == _hash(ctx, want_dig) and np.array_equal(dig, dig_d)


def test_build_refusals(ctx):
    from backuwup_amd import _lib, parity
    sizes = [100, 200, 300]
    data = np.zeros(600, np.uint8)
    groups, total = parity.plan(sizes, 2, 1)
    for field, value in [("shard_len", 192), ("shard_len", 200), ("out_offset", 8), ("first_packfile", 2), ("k", 0), ("m", 0)]:
        bad = groups.copy()
        bad[field][0] = value
        with pytest.raises(_lib.BwError) as x:
            parity.build(ctx, data, parity._table(sizes), bad, total)
        assert x.value.rc == _lib.BW_EINVAL, field
    with pytest.raises(_lib.BwError) as x:
        parity.build(ctx, data, parity._table(sizes), groups, total - 16)
    assert x.value.rc == _lib.BW_EINVAL


# ---------------------------------------------------------------- repair
SIZES42 = [3 * W + 100, 50, W + 7, 3 * W + 90]  # shard_len 3 W + 112: every data shard has a tail


@pytest.fixture(scope="module")
def group42(ctx):
    from backuwup_amd import parity
    packs = _packs(610, SIZES42)
    shards, groups = pr.encode(packs, 4, 2)
    length = groups[0][3]
    assert length == 3 * W + 112
    full = packs + shards
    size = SIZES42 + [length] * 2
    return dict(full=full, size=size, length=length, digests=np.frombuffer(b"".join(_hash(ctx, full)), np.uint8),
                group=np.array([(0, 4, 2, length, 0)], dtype=parity.GROUP_DTYPE))


def _repair(ctx, g, present, shards=None, digests=True, device=False):
    """The group's shards (or `shards`, a damaged copy) with `present` through one form: (status list,
    {shard: rebuilt bytes at shard_len}, the whole output buffer)."""
    import torch
    from backuwup_amd import parity
    shards = g["full"] if shards is None else shards
    n, length = len(shards), g["length"]
    off, at, parts = [], 5, [bytes([CANARY]) * 5]  # an odd base: every source alignment differs
    for s in range(n):
        off.append(at)
        if present[s]:
            parts.append(shards[s] + bytes([CANARY]) * 3)
            at += len(shards[s]) + 3
    buf = np.frombuffer(b"".join(parts), dtype=np.uint8)
    out_off = [16 + s * (length + 16) for s in range(n)]
    total = 16 + n * (length + 16)
    dg = g["digests"] if digests else None
    if device:
        d_sh = torch.from_numpy(buf.copy()).cuda()
        d_out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # torch's stream is not the context's
        st = parity.repair_device(ctx, g["group"], present, d_sh.data_ptr(), off, g["size"], d_out.data_ptr(), out_off, digests=dg)
        torch.cuda.synchronize()
        assert np.array_equal(d_sh.cpu().numpy(), buf), "bw_parity_repair_device wrote the shards"
        out = d_out.cpu().numpy()
    else:
        out = np.full(total, CANARY, dtype=np.uint8)
        _, st = parity.repair(ctx, g["group"], present, buf, off, g["size"], out_off, total, digests=dg, out=out)
    st = [int(x) for x in st]
    written = np.zeros(total, dtype=bool)
    rebuilt = {}
    for s in range(n):
        if st[s] in (DAMAGED, REBUILT, REBUILT_BAD):
            written[out_off[s]:out_off[s] + length] = True
            rebuilt[s] = out[out_off[s]:out_off[s] + length].tobytes()
    assert (out[~written] == CANARY).all(), "bytes outside the rebuilt shards were written"
    return st, rebuilt, out


@pytest.mark.parametrize("device", [False, True])
def test_every_erasure_pattern_up_to_two(ctx, group42, device):
    g = group42
    padded = [s + bytes(g["length"] - len(s)) for s in g["full"]]
    for gone in [()] + [c for r in (1, 2) for c in itertools.combinations(range(6), r)]:
        present = [s not in gone for s in range(6)]
        st, rebuilt, _ = _repair(ctx, g, present, device=device)
        assert st == [REBUILT if s in gone else OK for s in range(6)], gone
        assert rebuilt == {s: padded[s] for s in gone}, gone


def test_three_missing_is_lost_and_nothing_is_written(ctx, group42):
    for device in (False, True):
        for gone in [(0, 1, 2), (1, 4, 5), (0, 1, 2, 3, 4, 5)]:
            present = [s not in gone for s in range(6)]
            st, rebuilt, out = _repair(ctx, group42, present, device=device)
            assert st == [LOST if s in gone else OK for s in range(6)] and not rebuilt
            assert (out == CANARY).all()


def _flip(shard, at, bit=0x10):
    b = bytearray(shard)
    b[at] ^= bit
    return bytes(b)


def test_a_damaged_survivor_is_demoted_and_rebuilt(ctx, group42):
    g = group42
    padded = [s + bytes(g["length"] - len(s)) for s in g["full"]]
    for device in (False, True):
        for bad, at in [(0, 0), (3, g["size"][3] - 1), (1, 17), (4, W), (5, g["length"] - 1)]:
            shards = list(g["full"])
            shards[bad] = _flip(shards[bad], at)
            st, rebuilt, _ = _repair(ctx, g, [True] * 6, shards=shards, device=device)
            assert st == [DAMAGED if s == bad else OK for s in range(6)], (bad, at)
            assert rebuilt == {bad: padded[bad]}
            # and with another shard missing beside it: both come back
            gone = (bad + 2) % 6
            st, rebuilt, _ = _repair(ctx, g, [s != gone for s in range(6)], shards=shards, device=device)
            assert st == [DAMAGED if s == bad else REBUILT if s == gone else OK for s in range(6)]
            assert rebuilt == {bad: padded[bad], gone: padded[gone]}
    # a damaged shard and two missing ones: three gone, nothing written
    shards = list(g["full"])
    shards[2] = _flip(shards[2], 3)
    st, rebuilt, out = _repair(ctx, g, [False, True, True, True, False, True], shards=shards)
    assert st == [LOST, OK, LOST, OK, LOST, OK] and (out == CANARY).all()


def test_without_digests_a_damaged_survivor_poisons_the_result(ctx, group42):
    g = group42
    padded = [s + bytes(g["length"] - len(s)) for s in g["full"]]
    for device in (False, True):
        # shard 1 (50 bytes, a long tail) is missing; shard 0 carries a flipped bit at byte 1000, beyond shard
        # 1's size: the rebuilt shard 1 differs there, in what must be its zero tail
        shards = list(g["full"])
        shards[0] = _flip(shards[0], 1000)
        st, rebuilt, _ = _repair(ctx, g, [True, False, True, True, True, True], shards=shards, digests=False, device=device)
        assert st == [OK, REBUILT_BAD, OK, OK, OK, OK]
        diff = np.flatnonzero(np.frombuffer(rebuilt[1], np.uint8) != np.frombuffer(padded[1], np.uint8))
        assert diff.tolist() == [1000]
        # a missing parity shard has no tail: the damage goes through unseen, the bytes differ
        st, rebuilt, _ = _repair(ctx, g, [True, True, True, True, False, True], shards=shards, digests=False, device=device)
        assert st == [OK, OK, OK, OK, REBUILT, OK]
        assert rebuilt[4] != padded[4] and rebuilt[4][:1000] == padded[4][:1000]
        # with digests the same input is caught
        st, rebuilt, _ = _repair(ctx, g, [True, False, True, True, True, True], shards=shards, device=device)
        assert st == [DAMAGED, REBUILT, OK, OK, OK, OK] and rebuilt == {0: padded[0], 1: padded[1]}


def test_repair_refusals(ctx, group42):
    from backuwup_amd import _lib, parity
    g = group42
    buf = np.zeros(64, np.uint8)
    off, out_off = [0] * 6, [s * g["length"] for s in range(6)]
    for size in [g["size"][:3] + [g["length"] + 1] + g["size"][4:], g["size"][:4] + [g["length"] - 16, g["length"]],
                 [0] + g["size"][1:]]:
        with pytest.raises(_lib.BwError) as x:
            parity.repair(ctx, g["group"], [False] * 6, buf, off, size, out_off, 6 * g["length"])
        assert x.value.rc == _lib.BW_EINVAL


# ---------------------------------------------------------------- the wrappers, end to end
@pytest.fixture(scope="module")
def store(oracle):
    import prune_ref
    import restore_store
    rng = np.random.default_rng(620)
    b = restore_store.Builder(seed=620)
    for k in range(14):
        b.add(rng.integers(0, 256, 40 + 23 * k, dtype=np.uint8).tobytes())
    packs, index = b.finish(target=3)
    assert len(packs) == 5
    hd = prune_ref.headers_of(restore_store.PRK, packs)
    return dict(files=[bytes(p) for _, p in packs], ids=[bytes(i) for i, _ in packs], entries=prune_ref.entries_array(hd),
                items=restore_store.items_array(index), prk=restore_store.PRK)


def test_protect_damage_check_repair_check(ctx, store):
    from backuwup_amd import check, parity
    s = store
    shards, manifest = parity.protect(ctx, s["files"], s["ids"], s["prk"], k=3, m=2, nonce=bytes(range(12)))
    want, groups = pr.encode(s["files"], 3, 2)
    assert shards == want and [g[1] for g in groups] == [3, 2]
    # the manifest is the reference codec's bytes, sealed as one item
    man = parity.open_manifest(ctx, s["prk"], manifest)
    assert manifest[:12] == bytes(range(12)) and len(manifest) == 12 + len(pr.manifest_encode(man)) + 16
    assert [g["ids"] for g in man] == [s["ids"][:3], s["ids"][3:]] and [g["sizes"] for g in man] == [[len(f) for f in s["files"][:3]],
                                                                                                    [len(f) for f in s["files"][3:]]]
    digests = _hash(ctx, s["files"][:3] + want[:2] + s["files"][3:] + want[2:])
    assert [d for g in man for d in g["data_digests"] + g["parity_digests"]] == digests
    assert manifest == parity.protect(ctx, s["files"], s["ids"], s["prk"], k=3, m=2, nonce=bytes(range(12)))[1]
    assert manifest[12:] != parity.protect(ctx, s["files"], s["ids"], s["prk"], k=3, m=2)[1][12:]  # a random nonce
    # packfile 0 is gone, packfile 2 of the same group has a flipped byte in its last blob
    damaged = list(s["files"])
    damaged[2] = _flip(damaged[2], len(damaged[2]) - 20, 1)
    rep = check.check(ctx, damaged, s["ids"], s["entries"], s["items"], s["prk"])
    assert not rep["ok"] and rep["bad_packfiles"] == [2]
    held = [None if p == 0 else f for p, f in enumerate(damaged)]
    files, par, report = parity.repair_store(ctx, held, shards, manifest, s["prk"])
    assert files == s["files"] and par == shards
    assert report["status"] == [["rebuilt", "ok", "damaged", "ok", "ok"], ["ok", "ok", "ok", "ok"]]
    assert report["lost_groups"] == [] and report["rebuilt_packfiles"] == [0, 2] and report["rebuilt_parity"] == [] and report["ok"]
    rep = check.check(ctx, files, s["ids"], s["entries"], s["items"], s["prk"])
    assert rep["ok"] and rep["bad_packfiles"] == []
    # a lost parity shard comes back too; three gone in one group is lost, the other group is still repaired
    files, par, report = parity.repair_store(ctx, s["files"], [None, shards[1], shards[2], None], manifest, s["prk"])
    assert par == shards and report["rebuilt_parity"] == [0, 3] and report["ok"]
    held = [None, None, s["files"][2], None, s["files"][4]]
    files, par, report = parity.repair_store(ctx, held, [None] + shards[1:], manifest, s["prk"])
    assert report["lost_groups"] == [0] and not report["ok"] and files[:3] == held[:3] and files[3:] == s["files"][3:]
    assert report["status"][0] == ["lost", "lost", "ok", "lost", "ok"]
    # a manifest with a flipped byte raises, wherever the byte is, and so does another PRK
    for at in (0, 11, 12, 40, len(manifest) - 1):
        with pytest.raises(ValueError):
            parity.repair_store(ctx, s["files"], shards, _flip(manifest, at, 1), s["prk"])
    with pytest.raises(ValueError):
        parity.repair_store(ctx, s["files"], shards, manifest, bytes(32))


# ---------------------------------------------------------------- fuzz
@pytest.mark.parametrize("seed", range(40))
def test_fuzz(ctx, seed):
    from backuwup_amd import parity
    rng = np.random.default_rng(7000 + seed)
    try:
        k, m = int(rng.integers(1, 12)), int(rng.integers(1, 6))
        hi = int(rng.choice([40, 3000, 3 * W]))
        sizes = [int(x) for x in rng.integers(1, hi, k)]
        packs = _packs(8000 + seed, sizes)
        shards, groups = pr.encode(packs, k, m)
        length = groups[0][3]
        full, size = packs + shards, sizes + [length] * m
        g = dict(full=full, size=size, length=length, digests=np.frombuffer(b"".join(_hash(ctx, full)), np.uint8),
                 group=np.array([(0, k, m, length, 0)], dtype=parity.GROUP_DTYPE))
        gone = set(int(x) for x in rng.choice(k + m, size=int(rng.integers(0, m + 1)), replace=False))
        shards_in, bad = list(full), None
        if len(gone) < m and rng.integers(0, 2):
            bad = int(rng.choice([s for s in range(k + m) if s not in gone]))
            shards_in[bad] = _flip(full[bad], int(rng.integers(0, size[bad])), 1 << int(rng.integers(0, 8)))
        st, rebuilt, _ = _repair(ctx, g, [s not in gone for s in range(k + m)], shards=shards_in, device=bool(seed & 1))
        assert st == [REBUILT if s in gone else DAMAGED if s == bad else OK for s in range(k + m)]
        assert rebuilt == {s: full[s] + bytes(length - len(full[s])) for s in gone | ({bad} if bad is not None else set())}
    except BaseException:
        print("fuzz seed", seed)
        raise
