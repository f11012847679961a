"""Small stores for the find tests (tests/test_find.py on the CPU, tests/test_gpu_find.py on the device),
built with restore_store.Builder as tests/impact_stores.py builds its own.  A helper, not a test.  Every
case is a dict: packs, index, roots, verify, slots, n_entries, and queries: a list of keyword dicts for
find_ref.walk / backuwup_amd.find.paths (patterns, icase, subtree, chunks, kinds, size, mtime)."""
import functools

import diff_stores as ds
import restore_store as rs
from oracle import oracle

U64 = 2**64 - 1


def q(*patterns, **kw):
    return dict(patterns=[p.encode() if isinstance(p, str) else p for p in patterns], **kw)


def _case(b, roots, queries, target=4, verify=False, slots=16):
    n = len(b.blobs)
    packs, index = b.finish(target=target)
    return dict(packs=packs, index=index, roots=list(roots), n_entries=n, verify=verify, slots=slots, queries=queries)


THIRTY_TWO = ["*.txt", "/d/*", "**/x", "?", "[a-c]*", "[!a-c]*", "/**", "d/", "é*", "/d/**/k", "*?*", "\\x"] + \
             ["/d/n%02d" % k for k in range(20)]


def names():
    """Names of 0, 1, 63, 64, 65 and 255 bytes, multi-byte names, a File and a Dir of one name."""
    b = rs.Builder(seed=91)
    long = {"": b"E" * 30, "x": b"X" * 40, "a" * 63: b"1" * 20, "b" * 64: b"2" * 20, "c" * 65: b"3" * 20, "z" * 255: b"4" * 20,
            "été.txt": b"5" * 20, "€": b"6" * 20, "\U0001f600k": b"7" * 20, "K": {"k": b"8" * 20, "x": {"x": b"9" * 20}}}
    root = b.add_dir("r", {"d": long, "x": b"top" * 9, "Docs": {"d": b"D" * 25, "Read.TXT": b"R" * 33}})
    return _case(b, [root], [
        q("*"), q("x"), q("/x"), q("/d/?"), q("/d/??"), q("?", "??", "???"), q("*.txt", icase=True), q("/d/[!a-y]*"),
        q("/d/a*", "/d/b*b", "/d/" + "?" * 61, "/d/" + "c" * 60 + "*", "/d/z*z"), q("d/"), q("**/x/**"), q("/d/"), q("/*/"), q("/d/*/**/x"),
        q("/DOCS/READ.txt", icase=True), q("/DOCS/READ.txt"), q("é*", "\\x", "[k-k]"), q(*THIRTY_TWO),
        q("/d/K", subtree=True), q("x", kinds=1), q("x", kinds=2), q("/nothing/here")])


def wide(slots=16):
    """One Dir each of 63, 64, 65, 256 and 257 files."""
    b = rs.Builder(seed=92)
    dirs = []
    for n in (63, 64, 65, 256, 257):
        kids = [b.add_file("f%03d" % i, ("%d-%d" % (n, i)).encode().ljust(24 + i % 5, b".")) for i in range(n)]
        dirs.append(b.add_tree(1, "d%d" % n, None, None, None, kids))
    root = b.add_tree(1, "r", None, None, None, dirs)
    return _case(b, [root], [q("f*7"), q("/d64/f0?1", "/d257/f256", "/d65/*"), q("/d256", subtree=True, chunks=True),
                             q(*["/d%d/f%03d" % (n, 3 * k) for k, n in enumerate([63, 64, 65, 256, 257] * 6)] + ["f1*", "d*/"])],
                 target=64, slots=slots)


def four_slots():
    return wide(slots=4)


def two_pieces():
    """A Dir of 10,001 children rows and a File of 10,001 chunk rows: two pieces each."""
    b = rs.Builder(seed=93)
    small = b.add_file("s", b"S" * 40)
    chunk = b.add(b"C" * 40)
    big = b.add_tree(1, "big", None, None, None, [small] * 10001)
    long_file = b.add_tree(0, "f", 40 * 10001, None, None, [chunk] * 10001)
    root = b.add_tree(1, "r", None, None, None, [big, long_file])
    return _case(b, [root], [q("/f"), q("/f", chunks=True), q("s", chunks=True), q("/big/", subtree=True), q("/f/x")])


def deep():
    """A path 70 levels deep."""
    b = rs.Builder(seed=94)
    spec = {"leaf": b"L" * 40}
    for k in reversed(range(70)):
        spec = {"d%d" % k: spec, "side%d" % k: b"s" * (20 + k)}
    root = b.add_dir("r", spec)
    return _case(b, [root], [q("/**/leaf"), q("**/d69/*"), q("leaf", "side6?"), q("/d0/d1/d2/side3"), q("/d0/**/d40/**/side6[0-5]")])


def sibling():
    """A large directory beside the anchored target."""
    b = rs.Builder(seed=95)
    root = b.add_dir("r", {"big": {"f%03d.txt" % k: b"b%03d" % k * 8 for k in range(300)},
                           "target": {"a.txt": b"A" * 30, "b.bin": b"B" * 30, "sub": {"c.txt": b"C" * 30}}})
    return _case(b, [root], [q("/target/*.txt"), q("/target/**/*.txt"), q("*.txt", "/target/sub/")], target=32)


def shared():
    """The same subtree under two roots, and twice under one root."""
    b = rs.Builder(seed=96)
    sub = {"f.jpg": b"J" * 40, "g.txt": b"G" * 40}
    r1 = b.add_dir("r1", {"one": sub, "two": {"in": sub}, "f.jpg": b"J" * 40})
    r2 = b.add_dir("r2", {"one": sub, "z": b"Z" * 40})
    return _case(b, [r1, r2, r1], [q("*.jpg"), q("/one/*"), q("in/", subtree=True, chunks=True)])


def dir_contains_itself():
    b = rs.Builder(seed=97)
    f = b.add_file("f", b"F" * 40)
    loop = b"\xcd" * 32
    ds.raw_tree(b, 1, "loop", [loop, f], blob_hash=loop)
    return _case(b, [loop], [q("f"), q("loop"), q("**", subtree=True)])


def chain_names_itself():
    b = rs.Builder(seed=98)
    f = b.add_file("f", b"F" * 40)
    loop = b"\xab" * 32
    ds.raw_tree(b, 1, "loop", [f], sib=loop, blob_hash=loop)
    root = b.add_tree(1, "r", None, None, None, [loop])
    return _case(b, [root], [q("f"), q("/loop")], slots=4)


def _flip(packs, p, at):
    pid, buf = packs[p]
    buf = bytearray(buf)
    buf[at] ^= 0x40
    packs[p] = (pid, bytes(buf))


def damaged():
    """A child that is not in the store, a child whose first piece fails its tag, a Dir and a File whose second
    pieces are missing or fail their tag, a Dir row that names a chunk."""
    import prune_ref
    b = rs.Builder(seed=99)
    ok = b.add_file("ok.txt", b"O" * 40)
    torn = b.add_file("torn.txt", b"T" * 40)
    gone = b"\x77" * 32
    second_gone = b"\x66" * 32
    c1, c2 = b.add(b"c1" * 20), b.add(b"c2" * 20)
    second_bad = ds.raw_tree(b, 1, "", [ok], blob_hash=b"\x55" * 32)
    d1 = ds.raw_tree(b, 1, "cut1", [ok], sib=second_gone)
    d2 = ds.raw_tree(b, 1, "cut2", [ok], sib=second_bad)
    f2 = ds.raw_tree(b, 0, "long.txt", [c1], sib=second_gone, size=80)
    root = b.add_tree(1, "r", None, None, None, [ok, torn, gone, d1, d2, f2, c1])
    case = _case(b, [root, gone], [q("*.txt"), q("*.txt", chunks=True), q("/cut?", subtree=True)])
    hd = prune_ref.headers_of(rs.PRK, case["packs"])
    for p, h, _, _, length, offset in prune_ref.flat_entries(hd):
        if h in (torn, second_bad):
            _flip(case["packs"], p, 8 + hd[p][2] + offset + 12 + length // 2)
    return case


def filtered():
    """A SUBTREE hit on a directory where a size filter removes some of the files below it; mtimes; a File
    named as a trailing-'/' pattern names it."""
    b = rs.Builder(seed=100)
    docs = b.add_tree(1, "docs", None, 50, None, [b.add_file("s%d" % k, b"x" * (10 * k), mtime=100 + k) for k in range(1, 9)] +
                      [b.add_tree(0, "nosize", None, None, None, [])])
    root = b.add_tree(1, "r", None, None, None, [docs, b.add_file("name", b"N" * 30), b.add_dir("sub", {"name": {"in": b"I" * 20}})])
    return _case(b, [root], [q("/docs", subtree=True, size=(30, 60)), q("/docs", subtree=True, mtime=(103, 200), kinds=1),
                             q("/docs", subtree=True, size=(0, U64 - 1)), q("name/"), q("name"), q("/docs/*", size=(0, 0))])


NAMES = ("names", "wide", "four_slots", "two_pieces", "deep", "sibling", "shared", "dir_contains_itself", "chain_names_itself",
         "damaged", "filtered")


@functools.lru_cache(maxsize=None)
def case(name):
    import prune_ref
    import restore_ref
    c = globals()[name]()
    store = restore_ref.Store(rs.PRK, c["packs"], c["index"], verify=c["verify"])
    return c, store, prune_ref.headers_of(rs.PRK, c["packs"])


@functools.lru_cache(maxsize=None)
def reference(name, qi):
    """A case, query qi of it and what tests/find_ref.py says, once per process."""
    import find_ref
    c, store, hd = case(name)
    query = c["queries"][qi]
    return c, query, find_ref.walk(store, hd, c["roots"], **query)


# the queries per case, so that the tests can be parametrised without building a store at import
N_QUERIES = dict(names=22, wide=4, four_slots=4, two_pieces=5, deep=5, sibling=3, shared=3, dir_contains_itself=3,
                 chain_names_itself=2, damaged=3, filtered=6)


def all_queries():
    return [(n, i) for n in NAMES for i in range(N_QUERIES[n])]
