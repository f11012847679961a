"""Small stores with one parent snapshot each and the scans matched against it, for the parent match tests
(tests/test_parent.py, tests/test_gpu_parent_match.py).  A helper, not a test.  Every builder returns
dict(packs, index, root, scan, trust, ...): scan in parent_ref's form, trust = trust_before.

A spec is a Dir, a list of (name, value) pairs in child order (so that names may repeat): value = a
list (a Dir) or a dict (a File: size, mtime, ctime, any of them absent; data = its one chunk)."""
import numpy as np

import prune_ref
import restore_store as rs
from diff_stores import chain, raw_tree
from oracle import pack_oracle as po

NONE = 2**64 - 1


def F(size=0, mtime=1000, ctime=None, **kw):
    return dict(size=size, mtime=mtime, ctime=ctime, **kw)


def parent_of(b, name, v):
    """A spec value into the builder: the hash of its (first) tree blob."""
    if isinstance(v, list):
        return b.add_tree(1, name, None, None, None, [parent_of(b, k, x) for k, x in v])
    chunks = [b.add(v["data"])] if v.get("data") else []
    return b.add_tree(0, name, v.get("size"), v.get("mtime"), v.get("ctime"), chunks)


def scan_of(spec, root_name=""):
    """A spec as a scan: nodes in a listing's order (node 0 the root, a Dir's children consecutive,
    Dirs taken in node order)."""
    def node(name, v):
        if isinstance(v, list):
            return dict(kind=1, flags=0, size=0, mtime=0, ctime=0, child_first=0, n_children=0, name=name.encode(), spec=v)
        flags = (1 if v.get("size") is not None else 0) | (2 if v.get("mtime") is not None else 0) | \
            (4 if v.get("ctime") is not None else 0)
        return dict(kind=0, flags=flags, size=v.get("size") or 0, mtime=v.get("mtime") or 0, ctime=v.get("ctime") or 0,
                    child_first=0, n_children=0, name=name.encode(), spec=None)
    out = [node(root_name, spec)]
    i = 0
    while i < len(out):
        v = out[i].pop("spec")
        if v is not None:
            out[i]["child_first"], out[i]["n_children"] = len(out), len(v)
            out += [node(k, x) for k, x in v]
        i += 1
    return out


def case(seed, parent_spec, scan_spec, trust=NONE, target=9, **info):
    b = rs.Builder(seed=seed)
    root = parent_of(b, "", parent_spec)
    packs, index = b.finish(target=target)
    return dict(packs=packs, index=index, root=root, scan=scan_of(scan_spec), trust=trust, **info)


def where(scan, path):
    """The node of a path (names joined by /, first match of each name)."""
    i = 0
    for name in path.split("/") if path else []:
        n = scan[i]
        i = next(k for k in range(n["child_first"], n["child_first"] + n["n_children"]) if scan[k]["name"] == name.encode())
    return i


# ------------------------------------------------------------------ 1, 5: identity, and what the heuristic assumes
def identity_spec():
    return [("docs", [("a.txt", F(900, 1500, data=b"a" * 900)), ("b.txt", F(300, 1501, 1400)), ("empty", F(0, 1502)),
                      ("old", [("x", F(120, 1503)), ("y", F(80, 1504))])]),
            ("src", [("m.c", F(1200, 1505)), ("deep", [("deeper", [("z", F(100, 1506)), ("w", F(60, 1507))]), ("q", F(40, 1508))])]),
            ("top", F(500, 1509)), ("none", []), ("etc", [("conf", F(70, 1510))])]


def identity():
    s = identity_spec()
    return case(201, s, s)


def content_replaced():
    """The file's bytes differ, its name and metadata do not: the scan cannot tell."""
    a = [("d", [("f", F(4, 1700, 1600, data=b"old!")), ("g", F(9, 1701))])]
    b = [("d", [("f", F(4, 1700, 1600, data=b"new!")), ("g", F(9, 1701))])]
    return case(202, a, b)


# ------------------------------------------------------------------ 2: one field off
def fields():
    base = dict(size=10, mtime=2000, ctime=1900)
    pairs = {"same": (base, base), "size": (base, dict(base, size=11)), "mtime": (base, dict(base, mtime=2001)),
             "ctime": (base, dict(base, ctime=1901)),
             "size_parent_only": (base, dict(base, size=None)), "size_scan_only": (dict(base, size=None), base),
             "mtime_parent_only": (base, dict(base, mtime=None)), "mtime_scan_only": (dict(base, mtime=None), base),
             "ctime_parent_only": (base, dict(base, ctime=None)), "ctime_scan_only": (dict(base, ctime=None), base),
             "no_mtime_both": (dict(base, mtime=None), dict(base, mtime=None)),
             "no_size_both": (dict(base, size=None), dict(base, size=None)),
             "no_ctime_both": (dict(base, ctime=None), dict(base, ctime=None))}
    a = [(k, dict(p)) for k, (p, _) in pairs.items()]
    b = [(k, dict(s)) for k, (_, s) in pairs.items()]
    want = {k: 1 if k in ("same", "no_ctime_both") else 2 for k in pairs}
    return case(203, a, b, want=want)


# ------------------------------------------------------------------ 3: names
def names():
    long_ = "n" * 300
    p64 = "p" * 64
    both = ["", "a", "ab", "abc", long_, "été", "日本語", p64 + "one", p64 + "two"]
    a = [(n, F(10 + k, 3000 + k)) for k, n in enumerate(both)] + [("last1", F(1, 3100)), ("abcd", F(2, 3101))]
    b = [(n, F(10 + k, 3000 + k)) for k, n in enumerate(both)] + [("last2", F(1, 3100)), ("abce", F(2, 3101)),
                                                                   (long_[:-1], F(14, 3004)), (p64, F(17, 3007)),
                                                                   ("ét", F(15, 3005))]
    return case(204, [("names", a)], [("names", b)], n_same=len(both))


# ------------------------------------------------------------------ 4: trust_before
TRUST = 5000


def trust(limit):
    s = [("before", F(1, TRUST - 1)), ("at", F(2, TRUST)), ("after", F(3, TRUST + 7)), ("changed", F(4, TRUST + 1))]
    b = [(k, dict(v)) for k, v in s]
    b[3] = ("changed", F(5, TRUST + 1))
    return case(205, s, b, trust=limit)


# ------------------------------------------------------------------ 6, 7: duplicate names, and the item in the key
def duplicates():
    a = [("d", [("dup", F(1, 100)), ("x", F(2, 101)), ("dup", F(3, 102)), ("dup", F(4, 103))]),
         ("e", [("sub", [("in", F(5, 104))]), ("sub", [("other", F(6, 105))])])]
    b = [("d", [("dup", F(1, 100)), ("dup", F(1, 100)), ("x", F(2, 101)), ("dup", F(3, 102))]),
         ("e", [("sub", [("in", F(5, 104)), ("other", F(6, 105))]), ("sub", [("in", F(5, 104))])])]
    return case(206, a, b)


def same_name_in_many_dirs(n=300):
    a = [("d%03d" % k, [("a", F(7, 10000 + k))]) for k in range(n)]
    b = [("d%03d" % k, [("a", F(7, 10000 + (k if k % 7 else k + 1)))]) for k in range(n)]
    return case(207, a, b, target=64, n=n)


# ------------------------------------------------------------------ 8, 9: sizes at the wave and block boundaries
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)


def children_counts():
    a = [("c%d" % n, [("f%03d" % k, F(k, 20000 + k)) for k in range(n)]) for n in COUNTS]
    b = [("c%d" % n, [("f%03d" % k, F(k, 20000 + k + (1 if k % 5 == 4 else 0))) for k in range(n)]) for n in COUNTS]
    return case(208, a, b, target=64)


def level_of(n):
    """A level of n items."""
    a = [("i%03d" % k, [("f", F(3, 30000 + k))]) for k in range(n)]
    return case(209, a, a, target=64, n=n)


# ------------------------------------------------------------------ 10, 11: chains
def dir_chains():
    b = rs.Builder(seed=210)
    kids = [b.add_tree(0, "k%d" % k, 10 + k, 4000 + k, None, []) for k in range(6)]
    three = chain(b, 1, "split", [kids[:2], kids[2:3], kids[3:]])
    root = b.add_tree(1, "", None, None, None, [three])
    packs, index = b.finish(target=5)
    files = [("k%d" % k, F(10 + k, 4000 + k)) for k in range(6)]
    files[4] = ("k4", F(99, 4004))
    return dict(packs=packs, index=index, root=root, scan=scan_of([("split", files + [("k9", F(1, 1))])]), trust=NONE)


def big_dir(n=10001):
    """One true Dir of n empty files: split_serialize_tree cuts it after 10,000 children."""
    b = rs.Builder(seed=211)
    kids = [b.add_tree(0, "e%05d" % k, 0, 6000, None, []) for k in range(n)]
    root = b.add_tree(1, "", None, None, None, [b.add_tree(1, "big", None, None, None, kids)])
    packs, index = b.finish(target=2000)
    picks = [0, 1, 4999, 9998, 9999, 10000]
    files = [("e%05d" % k, F(0, 6000)) for k in picks] + [("e%05d" % n, F(0, 6000)), ("e09999", F(0, 6001))]
    return dict(packs=packs, index=index, root=root, scan=scan_of([("big", files)]), trust=NONE, picks=picks)


def file_chain_and_loop():
    b = rs.Builder(seed=212)
    c = [b.add(bytes([k]) * 20) for k in range(6)]
    f3 = chain(b, 0, "f3", [c[:2], c[2:4], c[4:]], size=120, mtime=7000)
    tail_hashes = []
    sib = None
    for rows in reversed([c[2:4], c[4:]]):          # the later pieces' hashes, to tell them from the first
        sib = raw_tree(b, 0, "f3", rows, sib, size=120, mtime=7000)
        tail_hashes.append(sib)
    kid = b.add_tree(0, "in_loop", 5, 7001, None, [])
    hl = b"\xab" * 32
    raw_tree(b, 1, "loop", [kid], sib=hl, blob_hash=hl)   # a chain that names itself
    root = b.add_tree(1, "", None, None, None, [f3, hl])
    packs, index = b.finish(target=4)
    scan = scan_of([("f3", F(120, 7000)), ("loop", [("in_loop", F(5, 7001)), ("other", F(1, 1))])])
    return dict(packs=packs, index=index, root=root, scan=scan, trust=NONE, later=tail_hashes, loop=hl)


# ------------------------------------------------------------------ 12, 13: structure
def structure():
    a = [("kept", [("f", F(1, 8000))]), ("removed", [("deep", [("g", F(2, 8001))]), ("h", F(3, 8002))]),
         ("was_file", F(4, 8003)), ("was_dir", [("below", F(5, 8004))])]
    b = [("kept", [("f", F(1, 8000))]), ("added", [("deep", [("g", F(2, 8001))]), ("h", F(3, 8002))]),
         ("was_file", [("below", F(5, 8004)), ("sub", [("x", F(6, 8005))])]), ("was_dir", F(5, 8004))]
    return case(213, a, b, target=3)


def root_is_file():
    b = rs.Builder(seed=214)
    root = b.add_tree(0, "lonely", 3, 8100, None, [b.add(b"abc")])
    packs, index = b.finish(target=3)
    return dict(packs=packs, index=index, root=root, scan=scan_of([("lonely", F(3, 8100))]), trust=NONE)


def root_unreadable():
    c = case(215, [("f", F(1, 8200))], [("f", F(1, 8200))])
    return dict(c, root=b"\x07" * 32)


# ------------------------------------------------------------------ 14, 15: damage
DAMAGE = ("absent", "no_packfile", "not_in_header", "bad_tag", "bad_zstd", "garbage", "chunk")


def damaged():
    """Every kind of damage to a child's first piece, each between good siblings; one scan node per name."""
    b = rs.Builder(seed=216)
    good = [b.add_tree(0, "good%d" % k, 30 + k, 9000 + k, None, []) for k in range(8)]
    bad = dict(absent=b"\x01" * 32, no_packfile=b"\x02" * 32, not_in_header=b"\x03" * 32)
    bad["bad_tag"] = b.add_tree(0, "bad_tag", 1, 9100, None, [])
    bad["bad_zstd"] = b.add(b"never decoded", po.KIND_TREE, blob_hash=b"\x04" * 32, payload=b"\x00this is no zstd frame")
    bad["garbage"] = b.add_raw_tree(b"\x02not a tree")
    bad["chunk"] = b.add(b"a chunk a Dir names")
    rows = []
    for k, name in enumerate(DAMAGE):
        rows += [good[k], bad[name]]
    rows.append(good[7])
    root = b.add_tree(1, "", None, None, None, rows)
    packs, index = b.finish(target=4)
    index = index + [(bad["no_packfile"], b"\xee" * 12), (bad["not_in_header"], packs[0][0])]
    hd = prune_ref.headers_of(rs.PRK, packs)
    for p, (_, _, hl, ents) in enumerate(hd):
        for h, _, _, length, offset in ents:
            if h == bad["bad_tag"]:
                buf = bytearray(packs[p][1])
                buf[8 + hl + offset + 12 + length - 1] ^= 1
                packs[p] = (packs[p][0], bytes(buf))
    scan = scan_of([("good%d" % k, F(30 + k, 9000 + k)) for k in range(8)] + [(n, F(1, 9100)) for n in DAMAGE])
    reasons = dict(absent=16, no_packfile=18, not_in_header=17, bad_tag=1, bad_zstd=2, garbage=20, chunk=19)
    return dict(packs=packs, index=index, root=root, scan=scan, trust=NONE, bad=bad, reasons=reasons, root_hash=root)


def broken_dir_chain():
    """A Dir chain whose second piece is not there: the list ends after the first."""
    b = rs.Builder(seed=217)
    kids = [b.add_tree(0, "k%d" % k, 10 + k, 9500 + k, None, []) for k in range(5)]
    lost = b"\x05" * 32
    third = raw_tree(b, 1, "d", kids[3:])
    first = raw_tree(b, 1, "d", kids[:2], sib=lost)
    root = b.add_tree(1, "", None, None, None, [first])
    packs, index = b.finish(target=4)
    scan = scan_of([("d", [("k%d" % k, F(10 + k, 9500 + k)) for k in range(5)])])
    return dict(packs=packs, index=index, root=root, scan=scan, trust=NONE, lost=lost, first=first, third=third)


# ------------------------------------------------------------------ 17: scans that are refused
def invalid_scans():
    """{what: scan}: each breaks one rule of a valid two-level scan."""
    ok = scan_of([("d", [("f", F(1, 1)), ("g", F(2, 2))]), ("e", [("h", F(3, 3))]), ("top", F(4, 4))])
    out = {}

    def broken(what, i, **kw):
        s = [dict(n) for n in ok]
        s[i].update(kw)
        out[what] = s
    broken("kind", 3, kind=2)
    broken("file_with_children", 3, n_children=1)
    broken("child_first_not_after", 1, child_first=1)
    broken("child_first_before", 2, child_first=0)
    broken("range_past_end", 2, n_children=3)
    broken("overlap", 2, child_first=5, n_children=1)
    broken("root_names_itself", 0, child_first=0)
    return ok, out
