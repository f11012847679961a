"""Prune on the CPU: tests/prune_ref.py's own invariants, and bw_prune_plan (host only) against it and
oracle/pack_oracle.plan_packfiles."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402

pytestmark = pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")


@pytest.fixture(scope="module")
def pr(oracle):
    import prune_ref
    import restore_ref
    import restore_store
    from backuwup_amd import _lib, prune

    class NS:
        pass
    ns = NS()
    ns.pref, ns.ref, ns.store, ns.lib, ns.prune, ns.po = prune_ref, restore_ref, restore_store, _lib, prune, restore_store.po
    ns.PRK = restore_store.PRK
    return ns


def _tree(oracle, kind=0, name=b"n", children=b"", sib=None):
    return oracle.tree_serialize(kind, name, None, None, None, children, sib)


@pytest.fixture(scope="module")
def snapshots(pr):
    """Two roots that share most subtrees."""
    rng = np.random.default_rng(21)
    blob = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    shared = {"docs": {"a.txt": blob(3000), "b.txt": blob(700), "empty": b""}, "src": {"m.c": blob(5000), "deep": {"x": blob(100)}}}
    b = pr.store.Builder(seed=21)
    root_a = b.add_dir("", dict(shared, only_a=blob(2500)))
    root_b = b.add_dir("", dict(shared, only_b={"y": blob(1800)}))
    packs, index = b.finish(target=7)
    return packs, index, root_a, root_b


def test_ref_mark_invariants(pr, snapshots):
    packs, index, root_a, root_b = snapshots
    store = pr.ref.Store(pr.PRK, packs, index)
    hd = pr.pref.headers_of(pr.PRK, packs)
    n = len(pr.pref.flat_entries(hd))
    none, e0, i0 = pr.pref.mark(store, hd, [])
    assert not none and not e0 and i0["n_levels"] == 0 and i0["n_trees_expanded"] == 0
    la, ea, ia = pr.pref.mark(store, hd, [root_a])
    lb, eb, ib = pr.pref.mark(store, hd, [root_b])
    lab, eab, iab = pr.pref.mark(store, hd, [root_a, root_b])
    assert not ea and not eb and not eab
    assert lab == la | lb == set(range(n)) and la - lb and lb - la and len(la & lb) > n // 2
    # every distinct tree blob is expanded once
    ents = pr.pref.flat_entries(hd)
    assert iab["n_trees_expanded"] == sum(1 for e in lab if ents[e][2] == pr.po.KIND_TREE)
    assert [s[2] for s in iab["stats"]] == [len(h[3]) for h in hd]
    assert sum(s[0] for s in ia["stats"]) == len(la)
    # what the kept root's restore reads is live
    _, files, errors = pr.ref.unpack(store, root_a)
    assert not errors and "only_a" in files


def test_ref_two_bits(pr, oracle):
    """A tree blob first named as a File's chunk is marked but not expanded; a Dir on a later level
    that names it as a child must still expand it."""
    b = pr.store.Builder(seed=22)
    leaf = b.add(b"leaf chunk of the hidden subtree")
    hidden_file = b.add_tree(0, "hf", None, None, None, [leaf])
    hidden = b.add_tree(1, "hidden", None, None, None, [hidden_file])
    trap = b.add_tree(0, "trap", None, None, None, [hidden])        # level 1: a File whose chunk is the tree blob
    late = b.add_tree(1, "late", None, None, None, [hidden])        # level 2: a Dir that names it
    mid = b.add_tree(1, "mid", None, None, None, [late])
    root = b.add_tree(1, "", None, None, None, [trap, mid])
    packs, index = b.finish(target=3)
    store = pr.ref.Store(pr.PRK, packs, index)
    hd = pr.pref.headers_of(pr.PRK, packs)
    live, errs, info = pr.pref.mark(store, hd, [root])
    assert not errs and len(live) == 7 and info["n_trees_expanded"] == 6
    live, errs, info = pr.pref.mark(store, hd, [trap])               # alone, the trap does not open it
    assert len(live) == 2 and info["n_trees_expanded"] == 1


def _plan_case(pr, packs, live, rewrite):
    hd = pr.pref.headers_of(pr.PRK, packs)
    en = pr.pref.entries_array(hd)
    lv = np.array([1 if e in live else 0 for e in range(en.size)], dtype=np.uint8)
    tab = pr.prune.packfile_table([p for _, p in packs])
    order, plan, total = pr.prune.plan(en, tab, lv, np.asarray(rewrite, dtype=np.uint8))
    want_order = pr.pref.order_of(hd, live, rewrite)
    assert list(order) == want_order
    groups = pr.po.plan_packfiles([int(en[e]["length"]) for e in want_order])
    assert [(int(p["first_blob"]), int(p["n_blobs"])) for p in plan] == groups
    ids = [bytes([g + 1]) * 12 for g in range(len(groups))]
    new, _, _, _ = pr.pref.repack(pr.PRK, packs, hd, live, rewrite, ids)
    assert [int(p["size"]) for p in plan] == [len(b) for _, b in new]
    assert [int(p["header_len"]) for p in plan] == [int.from_bytes(b[:8], "little") for _, b in new]
    assert list(plan["offset"]) == list(np.concatenate([[0], np.cumsum(plan["size"])[:-1]])) if plan.size else True
    assert total == sum(len(b) for _, b in new)
    return order, plan, en, tab, lv


@pytest.fixture(scope="module")
def big_store(pr):
    """More than 3 MiB of sealed bytes: 60 blobs of 70,000 bytes and some small ones."""
    rng = np.random.default_rng(23)
    b = pr.store.Builder(seed=23)
    for k in range(70):
        b.add(rng.integers(0, 256, 70000 if k % 7 else 300 + k, dtype=np.uint8).tobytes())
    return b.finish(target=9)[0]


def test_plan_nothing_and_everything_live(pr, big_store):
    n = sum(len(h[3]) for h in pr.pref.headers_of(pr.PRK, big_store))
    order, plan, *_ = _plan_case(pr, big_store, set(), [1] * len(big_store))
    assert order.size == 0 and plan.size == 0
    order, plan, *_ = _plan_case(pr, big_store, set(range(n)), [1] * len(big_store))
    assert order.size == n and plan.size >= 2 and plan["size"].sum() > 3 << 20


def test_plan_partial_rewrite_and_an_emptied_packfile(pr, big_store):
    npf = len(big_store)
    rewrite = [1 if p % 3 != 1 else 0 for p in range(npf)]
    live = {e for e in range(70) if e % 2 and not 9 <= e < 18}     # packfile 1 is not rewritten, packfile 2 ...
    live -= set(range(18, 27))                                       # ... is rewritten and left empty
    order, plan, en, *_ = _plan_case(pr, big_store, live | {10, 12}, rewrite)
    assert 10 not in order and 12 not in order                       # live, but their packfile is left alone
    assert not set(en["packfile"][order.astype(np.int64)]) & {1, 2}


def test_plan_bad_range_and_caps(pr, big_store):
    import ctypes
    L = pr.lib.load()
    hd = pr.pref.headers_of(pr.PRK, big_store)
    en = pr.pref.entries_array(hd)
    tab = pr.prune.packfile_table([p for _, p in big_store])
    live, rw = np.ones(en.size, dtype=np.uint8), np.ones(tab.size, dtype=np.uint8)
    EP, PP = ctypes.POINTER(pr.lib.BwUnpackEntry), ctypes.POINTER(pr.lib.BwPackfile)

    def call(en, order_cap, plan_cap):
        order, plan = np.zeros(max(order_cap, 1), dtype=np.uint64), np.zeros(max(plan_cap, 1), dtype=tab.dtype)
        v = [ctypes.c_uint64() for _ in range(4)]
        rc = L.bw_prune_plan(en.ctypes.data_as(EP), en.size, tab.ctypes.data_as(PP), tab.size, live.ctypes.data_as(pr.lib.u8p),
                             rw.ctypes.data_as(pr.lib.u8p), order.ctypes.data_as(pr.lib.u64p), order_cap, ctypes.byref(v[0]),
                             plan.ctypes.data_as(PP), plan_cap, ctypes.byref(v[1]), ctypes.byref(v[2]), ctypes.byref(v[3]))
        return rc, [x.value for x in v]

    rc, (nm, nn, total, bad) = call(en, en.size, 64)
    assert rc == pr.lib.BW_OK and nm == en.size and nn >= 2 and bad == 2**64 - 1
    for caps in ((en.size - 1, 64), (en.size, nn - 1), (0, 0)):
        rc2, got = call(en, *caps)
        assert rc2 == pr.lib.BW_ENOSPC and got == [nm, nn, total, 2**64 - 1]
    for field, value in (("length", 15), ("length", 1 << 24), ("offset", 1 << 24)):
        dmg = en.copy()
        dmg[33][field] = value
        rc3, got = call(dmg, en.size, 64)
        assert rc3 == pr.lib.BW_EINVAL and got[3] == 33, (field, rc3, got)
        with pytest.raises(pr.lib.BwError) as x:
            pr.prune.plan(dmg, tab, live, rw)
        assert x.value.bad_entry == 33
    live[33] = 0                                                     # a dead entry's range is nobody's business
    dmg = en.copy()
    dmg[33]["length"] = 15
    assert call(dmg, en.size, 64)[0] == pr.lib.BW_OK
    live[33] = 1


def test_plan_refuses_a_packfile_above_the_size_limit(pr):
    """Entries whose lengths the header claims: 6 live blobs of 2.9 MiB in one old packfile of 18 MiB would
    each close a new packfile; one blob of 17 MiB cannot be written at all."""
    from backuwup_amd.context import PACKFILE_DTYPE, UNPACK_ENTRY_DTYPE
    en = np.zeros(1, dtype=UNPACK_ENTRY_DTYPE)
    en[0]["length"] = 17 << 20
    tab = np.zeros(1, dtype=PACKFILE_DTYPE)
    tab[0]["size"], tab[0]["header_len"] = (18 << 20), 100
    with pytest.raises(pr.lib.BwError) as x:
        pr.prune.plan(en, tab, [1], [1])
    assert x.value.rc == pr.lib.BW_EINVAL and not hasattr(x.value, "bad_entry")


def test_choose_rewrite(pr):
    st = np.zeros(4, dtype=pr.prune.STAT_DTYPE)
    st["total_bytes"] = [100, 100, 100, 0]
    st["live_bytes"] = [100, 99, 40, 0]
    assert list(pr.prune.choose_rewrite(st)) == [0, 1, 1, 0]
    assert list(pr.prune.choose_rewrite(st, 0.5)) == [0, 0, 1, 0]
    assert list(pr.prune.choose_rewrite(st, 0.6)) == [0, 0, 0, 0]
