"""Small stores for the retain tests (tests/test_retain.py on the CPU, tests/test_gpu_retain.py and
tests/test_cpp_host_retain.py on the device), built with restore_store.Builder.  A helper, not a test.
Every case is a dict: packs, index, roots, n_entries, verify, slots, info.  Files of under 64 bytes are one
chunk, so the entry order of the small cases can be read off the builder calls (a blob's entry index is
its position in add order)."""
import functools

import numpy as np

import diff_stores as ds
import restore_store as rs
from oracle import oracle


def _case(b, roots, target=4, verify=False, slots=16, **info):
    n = len(b.blobs)
    packs, index = b.finish(target=target)
    return dict(packs=packs, index=index, roots=list(roots), n_entries=n, verify=verify, slots=slots, info=info)


def clean():
    """One root.  entries: A, a, B, b, d, r"""
    b = rs.Builder(seed=171)
    root = b.add_dir("r", {"a": b"A" * 40, "d": {"b": b"B" * 40}})
    return _case(b, [root])


def shared():
    """Two roots that share a directory, and a chunk named by files in both.
    entries: X, f, d1, g, Y, h, d2, r, Z, z, w (names X again), r2"""
    b = rs.Builder(seed=172)
    d1, d2 = {"f": b"X" * 40}, {"g": b"X" * 40, "h": b"Y" * 40}
    r1 = b.add_dir("r", {"d1": d1, "d2": d2})
    r2 = b.add_dir("r2", {"d2": d2, "z": b"Z" * 40, "w": b"X" * 40})
    return _case(b, [r1, r2])


def late_parent():
    """A subtree hung directly under root A and five levels down under root B: B's bit arrives at s after s
    was swept.  entries: X, x, s, a, b5, b4, b3, b2, b1, b"""
    b = rs.Builder(seed=173)
    s = {"x": b"X" * 40}
    ra = b.add_dir("a", {"s": s})
    rb = b.add_dir("b", {"b1": {"b2": {"b3": {"b4": {"b5": {"s": s}}}}}})
    return _case(b, [ra, rb])


def file_row_names_a_tree():
    """Root A reaches Dir d only as a File's child row, root B as a Dir child: d's children carry B alone.
    entries: K, k, d, f, a, b"""
    b = rs.Builder(seed=174)
    d = b.add_dir("d", {"k": b"K" * 40})
    f = b.add_tree(0, "f", 40, None, None, [d])
    ra = b.add_tree(1, "a", None, None, None, [f])
    rb = b.add_tree(1, "b", None, None, None, [d])
    return _case(b, [ra, rb])


def root_is_a_later_piece():
    """A Dir of 10,001 rows in two pieces, root B being the hash of its second piece: the first piece's rows
    are A's alone.  entries: P, p, Q, q, big piece 1, big piece 2"""
    b = rs.Builder(seed=175)
    p, q = b.add_file("p", b"P" * 40), b.add_file("q", b"Q" * 40)
    kids = [p] * 10000 + [q]
    big = b.add_tree(1, "big", None, None, None, kids)
    second = oracle.split_serialize_tree(1, "big", None, None, None, b"".join(kids))[1][1]
    return _case(b, [big, second], second=second)


def wide(slots=16):
    """Dirs of 63, 64, 65, 256 and 257 files under two roots; the second root takes every other Dir."""
    b = rs.Builder(seed=176)
    dirs = []
    for n in (63, 64, 65, 256, 257):
        kids = [b.add_file("f%03d" % i, ("%d-%d" % (n, i)).encode().ljust(24, b".")) for i in range(n)]
        dirs.append(b.add_tree(1, "d%d" % n, None, None, None, kids))
    r1 = b.add_tree(1, "r1", None, None, None, dirs)
    r2 = b.add_tree(1, "r2", None, None, None, dirs[::2])
    return _case(b, [r1, r2], target=64, slots=slots)


def many_roots(n):
    """n roots, each a Dir with one file of its own and one file common to all."""
    b = rs.Builder(seed=177)
    common = b.add_file("common", b"C" * 40)
    roots = [b.add_tree(1, "r%d" % i, None, None, None, [b.add_file("own", ("own-%d" % i).encode().ljust(24, b".")), common])
             for i in range(n)]
    return _case(b, roots, target=16)


def _small(seed):
    b = rs.Builder(seed=seed)
    f = b.add_file("f", b"F" * 40)
    root = b.add_tree(1, "r", None, None, None, [f, b.add_file("g", b"G" * 40)])
    return b, f, root


def duplicate_roots():
    """The same hash given twice: each gets its own bit.  entries: F, f, G, g, r"""
    b, _, root = _small(178)
    return _case(b, [root, root])


def zero_roots():
    b, _, _ = _small(179)
    return _case(b, [])


def root_missing():
    b, _, root = _small(180)
    return _case(b, [b"\x11" * 32, root])


def root_is_a_chunk():
    b, _, root = _small(181)
    return _case(b, [oracle.blake3(b"F" * 40), root])


def duplicate_hashes():
    """One hash held by two entries of one packfile; locate resolves it to entry 0, the other is an orphan.
    entries: D, D again, f, r"""
    b = rs.Builder(seed=182)
    b.add(b"D" * 40)
    b.add(b"D" * 40, again=True)
    root = b.add_dir("r", {"f": b"D" * 40})
    return _case(b, [root], target=8)


def real_damage():
    """A flipped ciphertext byte in a tree blob both roots reach (BW_UNPACK_ETAG), a sound tree body under a
    hash that is not its own (_EDIGEST under VERIFY) below root 0 alone; the walk goes on beside them.
    entries: A, a, B, b, t, C, c, u (under the forged hash), r, r2"""
    import prune_ref
    b = rs.Builder(seed=183)
    a = b.add_file("a", b"A" * 40)
    t = b.add_dir("t", {"b": b"B" * 40})
    c = b.add_file("c", b"C" * 40)
    fake = b"\x5a" * 32
    ds.raw_tree(b, 1, "u", [c], blob_hash=fake)
    r1 = b.add_tree(1, "r", None, None, None, [a, t, fake])
    r2 = b.add_tree(1, "r2", None, None, None, [t, c])
    case = _case(b, [r1, r2], verify=True, tag=t, digest=fake)
    hd = prune_ref.headers_of(rs.PRK, case["packs"])
    for p, h, _, _, length, offset in prune_ref.flat_entries(hd):
        if h == t:
            pid, buf = case["packs"][p]
            buf = bytearray(buf)
            buf[8 + hd[p][2] + offset + 12 + length // 2] ^= 0x40
            case["packs"][p] = (pid, bytes(buf))
    return case


CASES = [("clean", None), ("shared", None), ("late_parent", None), ("file_row_names_a_tree", None),
         ("root_is_a_later_piece", None), ("wide", 16), ("wide", 4)] + [("many_roots", n) for n in (1, 2, 63, 64, 65, 128, 129)] + [
             ("duplicate_roots", None), ("zero_roots", None), ("root_missing", None), ("root_is_a_chunk", None),
             ("duplicate_hashes", None), ("real_damage", None)]


def drop_sets(n_roots, seed=7):
    """The questions every case is asked: forget nothing, each single root (seven at most, spread over the
    words), all roots, four seeded random subsets."""
    singles = sorted(set(np.linspace(0, n_roots - 1, min(n_roots, 7)).astype(int).tolist())) if n_roots else []
    rng = np.random.default_rng(seed + n_roots)
    rand = [sorted(np.flatnonzero(rng.integers(0, 2, n_roots)).tolist()) for _ in range(4)]
    return [[]] + [[r] for r in singles] + [list(range(n_roots))] + rand


@functools.lru_cache(maxsize=None)
def reference(name, arg=None):
    """A case and what tests/retain_ref.py says of it, once per process: (case, headers, masks, damaged,
    per_root, errors, info)."""
    import prune_ref
    import restore_ref
    import retain_ref
    if name == "wide" and arg != 16:  # the same store through fewer slots: the reference does not know slots
        case, *rest = reference("wide", 16)
        return (dict(case, slots=arg), *rest)
    case = globals()[name]() if arg is None else globals()[name](arg)
    store = restore_ref.Store(rs.PRK, case["packs"], case["index"], verify=case["verify"])
    hd = prune_ref.headers_of(rs.PRK, case["packs"])
    masks, damaged, per_root, errors, info = retain_ref.mark(store, hd, case["roots"])
    return case, hd, masks, damaged, per_root, errors, info
