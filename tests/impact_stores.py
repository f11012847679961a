"""Small stores for the impact tests (tests/test_impact.py on the CPU, tests/test_gpu_impact.py on the
device), built with restore_store.Builder.  A helper, not a test.  Every case is a dict: packs, index,
roots, bad (entry indices treated as lost, from the header order: a blob's entry index is its position in
add order), verify, slots, and whatever the tests assert beside the reference (info).  Files of under 64
bytes are one chunk, so the entry order of the small cases can be read off the builder calls."""
import functools

import numpy as np

import diff_stores as ds
import restore_store as rs
from oracle import oracle
from oracle import pack_oracle as po


def _case(b, roots, bad=(), target=4, verify=False, slots=16, **info):
    n = len(b.blobs)
    packs, index = b.finish(target=target)
    return dict(packs=packs, index=index, roots=list(roots), bad=sorted(bad), n_entries=n, verify=verify, slots=slots, info=info)


def _entry(b, h):
    """The first entry (add order) that holds hash h."""
    return next(i for i, blob in enumerate(b.blobs) if blob[0] == bytes(h))


def clean():
    b = rs.Builder(seed=71)
    root = b.add_dir("r", {"a": b"A" * 40, "d": {"b": b"B" * 40}})
    return _case(b, [root])


def shared_chunk():
    """One chunk named by two files in different directories; two roots share one of those directories."""
    b = rs.Builder(seed=72)
    d1, d2 = {"f": b"X" * 40}, {"g": b"X" * 40, "h": b"Y" * 40}
    r1 = b.add_dir("r", {"d1": d1, "d2": d2})
    r2 = b.add_dir("r2", {"d2": d2, "z": b"Z" * 40})
    return _case(b, [r1, r2], bad=[_entry(b, oracle.blake3(b"X" * 40))], n_tree_blobs=8)


def lost_directory():
    """bad on a Dir's first piece, two levels down."""
    b = rs.Builder(seed=73)
    root = b.add_dir("r", {"a": b"A" * 40, "m": {"d": {"b": b"B" * 40}}})
    d = b.blobs[4][0]
    return _case(b, [root], bad=[4], lost=d)


def lost_later_piece():
    """A Dir of 10,001 children rows and a File of 10,001 chunk rows, each with bad on its second piece."""
    b = rs.Builder(seed=74)
    small = b.add_file("s", b"S" * 40)
    chunk = b.add(b"C" * 40)
    big = b.add_tree(1, "big", None, None, None, [small] * 10001)
    long_file = b.add_tree(0, "f", 40 * 10001, None, None, [chunk] * 10001)
    second = [oracle.split_serialize_tree(1, "big", None, None, None, small * 10001)[1][1],
              oracle.split_serialize_tree(0, "f", 40 * 10001, None, None, chunk * 10001)[1][1]]
    root = b.add_tree(1, "r", None, None, None, [big, long_file])
    return _case(b, [root], bad=[_entry(b, h) for h in second])


def late_parent():
    """A subtree hung directly under the root and again five levels down, a bad chunk at its bottom."""
    b = rs.Builder(seed=75)
    s = {"x": b"X" * 40}
    root = b.add_dir("r", {"s": s, "a1": {"a2": {"a3": {"a4": {"a5": {"s": s}}}}}})
    return _case(b, [root], bad=[0])


def wide(slots=16):
    """One Dir each of 63, 64, 65, 256 and 257 files, every 7th file's only chunk bad."""
    b = rs.Builder(seed=76)
    bad, dirs = [], []
    for n in (63, 64, 65, 256, 257):
        kids = []
        for i in range(n):
            data = ("%d-%d" % (n, i)).encode().ljust(24, b".")
            if i % 7 == 0:
                bad.append(len(b.blobs))  # the chunk is the next blob added
            kids.append(b.add_file("f%03d" % i, data))
        dirs.append(b.add_tree(1, "d%d" % n, None, None, None, kids))
    root = b.add_tree(1, "r", None, None, None, dirs)
    return _case(b, [root], bad=bad, target=64, slots=slots)


def four_slots():
    return wide(slots=4)


def duplicate_hashes(which):
    """One hash held by two entries of one packfile; locate resolves it to entry 0.  which: the bad one."""
    b = rs.Builder(seed=77)
    b.add(b"D" * 40)
    b.add(b"D" * 40, again=True)
    root = b.add_dir("r", {"f": b"D" * 40})
    return _case(b, [root], bad=[which], target=8)


def whole_packfile(p):
    """A store of 6 packfiles; bad = every entry of packfile p (what impact.lost_packfiles gives)."""
    b = rs.Builder(seed=78)
    spec = {"d%d" % i: {"f%d" % j: ("%d/%d" % (i, j)).encode() * 9 for j in range(3)} for i in range(3)}
    root = b.add_dir("r", spec)
    assert len(b.blobs) == 22
    return _case(b, [root], bad=range(4 * p, min(4 * p + 4, 22)), n_packfiles=6)


def _flip(packs, p, at):
    pid, buf = packs[p]
    buf = bytearray(buf)
    buf[at] ^= 0x40
    packs[p] = (pid, bytes(buf))


def real_damage():
    """No bad vector: a flipped ciphertext byte in a chunk (never read, so not found), one in a tree blob
    (BW_UNPACK_ETAG) and a sound tree body under a hash that is not its own (_EDIGEST under VERIFY)."""
    import prune_ref
    b = rs.Builder(seed=79)
    a = b.add_file("a", b"A" * 40)
    t = b.add_dir("t", {"b": b"B" * 40})
    c = b.add_file("c", b"C" * 40)
    fake = b"\x5a" * 32
    ds.raw_tree(b, 1, "u", [c], blob_hash=fake)
    root = b.add_tree(1, "r", None, None, None, [a, t, fake])
    case = _case(b, [root], verify=True, tag=t, digest=fake, chunk=oracle.blake3(b"A" * 40))
    hd = prune_ref.headers_of(rs.PRK, case["packs"])
    for p, h, _, _, length, offset in prune_ref.flat_entries(hd):
        if h in (t, case["info"]["chunk"]):
            _flip(case["packs"], p, 8 + hd[p][2] + offset + 12 + length // 2)
    return case


def dir_contains_itself():
    """A Dir that names itself, above a file with a bad chunk."""
    b = rs.Builder(seed=80)
    f = b.add_file("f", b"F" * 40)
    loop = b"\xcd" * 32
    ds.raw_tree(b, 1, "loop", [loop, f], blob_hash=loop)
    return _case(b, [loop], bad=[0], loop=loop)


def chain_names_itself():
    """A Dir of one piece whose next_sibling is its own hash, with a bad chunk below it."""
    b = rs.Builder(seed=81)
    f = b.add_file("f", b"F" * 40)
    loop = b"\xab" * 32
    ds.raw_tree(b, 1, "loop", [f], sib=loop, blob_hash=loop)
    root = b.add_tree(1, "r", None, None, None, [loop])
    return _case(b, [root], bad=[0], slots=4, loop=loop)


def edges(which):
    """Roots at the edges over one store: none, a root of kind File with a bad chunk, an unlocatable root,
    the same root twice, 100 roots that share one tree."""
    b = rs.Builder(seed=82)
    f = b.add_file("f", b"F" * 40)
    root = b.add_tree(1, "r", None, None, None, [f, b.add_file("g", b"G" * 40)])
    roots = dict(none=[], file_root=[f], unlocatable=[b"\x11" * 32, root], twice=[root, root], hundred=[root] * 100)[which]
    return _case(b, roots, bad=[0])


@functools.lru_cache(maxsize=None)
def reference(name, arg=None):
    """A case and what tests/impact_ref.py says of it, once per process: (case, taint, root_affected, mark
    errors, info, records, per_root, paths errors)."""
    import impact_ref
    import prune_ref
    import restore_ref
    case = globals()[name]() if arg is None else globals()[name](arg)
    store = restore_ref.Store(rs.PRK, case["packs"], case["index"], verify=case["verify"])
    hd = prune_ref.headers_of(rs.PRK, case["packs"])
    bad = [0] * case["n_entries"]
    for e in case["bad"]:
        bad[e] = 1
    taint, affected, errors, info = impact_ref.mark(store, hd, case["roots"], bad)
    records, per_root, perrors = impact_ref.paths(store, hd, case["roots"], taint)
    return case, taint, affected, errors, info, records, per_root, perrors
