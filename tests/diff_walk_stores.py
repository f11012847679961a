"""One more store for the device diff walk (tests/test_gpu_diff_walk.py), built like the ones of
tests/diff_stores.py.  A helper, not a test.  Returns (packs, index, root_a, root_b, info)."""
import numpy as np

import diff_stores as ds

import restore_store as rs

WIDE = 300


def chain_names_itself():
    """On side B the Dir `loop` is one piece whose next_sibling is its own hash, between the sound siblings
    `before` and `after` (their mtimes change, so both give records); side A holds a sound Dir of the
    same name.  The walk follows the chain for as many pieces as the store has entries and refuses the
    next round unread.  info: loop = the looping hash, n_entries = the store's entries."""
    rng = np.random.default_rng(62)
    b = rs.Builder(seed=62)
    kid = b.add_file("in_loop", ds.blob(rng, 50))
    data_before, data_after = ds.blob(rng, 60), ds.blob(rng, 70)
    hl = b"\xab" * 32
    ds.raw_tree(b, 1, "loop", [kid], sib=hl, blob_hash=hl)
    sound = b.add_tree(1, "loop", None, None, None, [kid])
    ra = b.add_tree(1, "", None, None, None, [b.add_file("before", data_before, 1000), sound, b.add_file("after", data_after, 1000)])
    rb = b.add_tree(1, "", None, None, None, [b.add_file("before", data_before, 2000), hl, b.add_file("after", data_after, 2000)])
    n_entries = len(b.blobs)
    packs, index = b.finish(target=5)
    return packs, index, ra, rb, dict(loop=hl, n_entries=n_entries)


def wide_and_shared():
    """A directory with 300 unmatched children on each side between shared ones (odd positions keep
    their names and pair, even ones are renamed), so that the name join and the frontier compaction
    cross a 256-lane workgroup; and two two-level directories, p/q and r/s, that hold the same
    unmatched child hash at the same level: the directory `sub` leaves p/q and appears under r/s, so
    one hash is a node twice in a level and its children are nodes twice in the next."""
    rng = np.random.default_rng(61)
    da, db = {}, {}
    for k in range(WIDE):
        if k % 3 == 0:
            da["s%03d" % k] = db["s%03d" % k] = ds.blob(rng, 40)
        da["c%03d" % k] = ds.blob(rng, 41)
        db[("c%03d" if k % 2 else "n%03d") % k] = ds.blob(rng, 42)
    sub = {"in": ds.blob(rng, 90), "deeper": {"in2": ds.blob(rng, 70)}}
    a = {"wide": da, "p": {"q": {"sub": sub, "keep": b"k"}}, "r": {"s": {"keep": b"k", "old": b"o"}}}
    b = {"wide": db, "p": {"q": {"keep": b"k", "fresh": b"f"}}, "r": {"s": {"keep": b"k", "sub": sub}}}
    return ds.two(61, a, b, target=64)
