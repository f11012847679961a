"""Diff: what changed between two snapshots of one store.  The reference has no diff.

Two forms.  trees() / diff() are the device walk (bw_diff_trees): it opens only the tree blobs on a
changed path, carries on past damage (errors are collected, flags mark unreadable and truncated
sides) and sees how a next_sibling chain was split, as the hashes do.  listing_changes() /
full_walk_diff() are the walk-everything form, from two full tree walks.

A Tree blob holds its own name, kind and metadata and names its children by hash
(filesystem/mod.rs:63-77), so two subtrees are equal exactly when their listings are.
listing_changes() compares two bw_restore_trees listings (restore.Session.trees) on the host by the
rules a hash walk follows: a child is matched when the other side's list holds an equal subtree; of
the children left over, the first of each name on a side represents it, representatives with equal
names pair up, and every other one is added or removed, with everything below it.
full_walk_diff() is the whole answer over a store held as lists of bytes: the two walks, the
comparison, and with sizes=True what each snapshot alone keeps alive in the store (two prune.mark
calls).

In the walk-everything form both roots are read in full, however little changed, a tree blob that
cannot be read ends the call as it ends a restore (restore.TreeError), and a listing does not show
how a next_sibling chain was split, so two chains with the same children are equal there."""
import ctypes
import hashlib
import struct

import numpy as np

from . import _lib, prune
from ._lib import check
from .context import UNPACK_ENTRY_DTYPE
from .prune import ERROR_DTYPE
from .restore import Session

ADDED, REMOVED, MODIFIED, TYPE_CHANGED = 1, 2, 3, 4
CHANGES = {ADDED: "added", REMOVED: "removed", MODIFIED: "modified", TYPE_CHANGED: "type_changed"}
SIDE_FIELDS = ("kind", "flags", "size", "mtime", "ctime", "n_children")
F_UNREADABLE, F_TRUNCATED = _lib.BW_DIFF_UNREADABLE, _lib.BW_DIFF_TRUNCATED
NONE = 2**64 - 1
SIDE_DTYPE = np.dtype([("hash", "u1", (32,)), ("kind", "<u4"), ("flags", "<u4"), ("size", "<u8"), ("mtime", "<u8"),
                       ("ctime", "<u8"), ("n_children", "<u8")])
RECORD_DTYPE = np.dtype([("change", "<u4"), ("flags", "<u4"), ("parent", "<u8"), ("name_off", "<u8"), ("name_len", "<u8"),
                         ("a", SIDE_DTYPE), ("b", SIDE_DTYPE), ("common_prefix", "<u8"), ("common_suffix", "<u8"),
                         ("n_new", "<u8")])
assert SIDE_DTYPE.itemsize == ctypes.sizeof(_lib.BwDiffSide) == 72
assert RECORD_DTYPE.itemsize == ctypes.sizeof(_lib.BwDiffRecord) == 200
COUNT_FIELDS = [f for f, _ in _lib.BwDiffCounts._fields_]


class _Listing:
    """One walk as Python lists, with a signature per node: equal signatures = equal subtrees, the
    node's own name and metadata included (what the hash of its tree blob says)."""

    def __init__(self, nodes, names, chunks):
        names = bytes(names)
        rows = np.ascontiguousarray(np.asarray(chunks, dtype=np.uint8).reshape(-1, 32))
        self.n = len(nodes)
        cols = [nodes[f].tolist() for f in SIDE_FIELDS]
        self.meta = list(zip(*cols)) if self.n else []
        self.dir = [k == _lib.BW_TREE_DIR for k in cols[0]]
        off, ln = nodes["name_off"].tolist(), nodes["name_len"].tolist()
        self.name = [names[o:o + n] for o, n in zip(off, ln)]
        first, count = nodes["child_first"].tolist(), cols[5]
        self.kids = [None] * self.n       # Dir: child node indices; File: its chunk rows as bytes
        self.sig = [None] * self.n
        for i in range(self.n - 1, -1, -1):   # children come after their parents
            if self.dir[i]:
                self.kids[i] = range(first[i], first[i] + count[i])
                body = b"".join([self.sig[k] for k in self.kids[i]])
            else:
                body = rows[first[i]:first[i] + count[i]].tobytes()
                self.kids[i] = [body[o:o + 32] for o in range(0, len(body), 32)]
            head = struct.pack("<7Q", *self.meta[i], len(self.name[i])) + self.name[i]
            self.sig[i] = hashlib.blake2b(head + body, digest_size=32).digest()

    def rows(self, i):
        """What a node's children list is compared by: signatures for a Dir, chunk hashes for a File."""
        return [self.sig[k] for k in self.kids[i]] if self.dir[i] else self.kids[i]

    def side(self, i):
        return dict(zip(SIDE_FIELDS, self.meta[i]))

    def path(self, parent, k):
        # a name is a Rust String, so UTF-8; a listing from elsewhere must not end the comparison
        name = self.name[k].decode("utf-8", "surrogateescape")
        return parent + "/" + name if parent else name


def listing_changes(listing_a, listing_b):
    """listing_a, listing_b: (nodes NODE_DTYPE, names, chunks) as Session.trees returns them, or None
    for an empty snapshot.  Returns [dict(path, change, a, b, common_prefix, common_suffix, n_new)]
    sorted by path: change = ADDED, REMOVED, MODIFIED or TYPE_CHANGED (1 .. 4; CHANGES names them),
    a / b = dict(kind, flags, size, mtime, ctime, n_children) or None for the absent side; the three
    counts are over the two children lists of a modified node (chunk hashes of a File, subtrees of a
    Dir): the equal leading entries, the equal trailing ones (capped at min(n_a, n_b) -
    common_prefix) and the entries of B that occur nowhere in A.  The roots pair whatever their
    names; the root's path is ''.  Duplicate names in one directory keep their order: the first
    unmatched child of a name is the one that pairs."""
    la = _Listing(*listing_a) if listing_a is not None else None
    lb = _Listing(*listing_b) if listing_b is not None else None
    out = []
    todo = []  # (A node or None, B node or None, path): a stack, so that deep trees need no recursion

    def push_a(kids, path):
        todo.extend((k, None, la.path(path, k)) for k in kids)

    def push_b(kids, path):
        todo.extend((None, k, lb.path(path, k)) for k in kids)

    if la is not None and lb is not None:
        if la.sig[0] != lb.sig[0]:
            todo.append((0, 0, ""))
    elif la is not None or lb is not None:
        todo.append((0 if la is not None else None, 0 if lb is not None else None, ""))
    while todo:
        a, b, path = todo.pop()
        rec = dict(path=path, change=MODIFIED, a=None if a is None else la.side(a), b=None if b is None else lb.side(b),
                   common_prefix=0, common_suffix=0, n_new=0)
        out.append(rec)
        if a is None or b is None:
            rec["change"] = ADDED if a is None else REMOVED
            if a is None and lb.dir[b]:
                push_b(lb.kids[b], path)
            elif b is None and la.dir[a]:
                push_a(la.kids[a], path)
            continue
        if la.dir[a] != lb.dir[b]:         # the two sides are expanded apart
            rec["change"] = TYPE_CHANGED
            if la.dir[a]:
                push_a(la.kids[a], path)
            else:
                push_b(lb.kids[b], path)
            continue
        ra, rb = la.rows(a), lb.rows(b)
        sa, sb = set(ra), set(rb)
        lim = min(len(ra), len(rb))
        p = 0
        while p < lim and ra[p] == rb[p]:
            p += 1
        s = 0
        while s < lim - p and ra[len(ra) - 1 - s] == rb[len(rb) - 1 - s]:
            s += 1
        rec["common_prefix"], rec["common_suffix"], rec["n_new"] = p, s, sum(1 for r in rb if r not in sa)
        if not la.dir[a]:
            continue
        left_a = [k for k, r in zip(la.kids[a], ra) if r not in sb]
        left_b = [k for k, r in zip(lb.kids[b], rb) if r not in sa]
        rep_a, rep_b = {}, {}
        for k in left_a:
            rep_a.setdefault(la.name[k], k)
        for k in left_b:
            rep_b.setdefault(lb.name[k], k)
        for k in left_a:
            name = la.name[k]
            if rep_a[name] == k and name in rep_b:
                todo.append((k, rep_b[name], la.path(path, k)))
            else:
                push_a([k], path)
        push_b([k for k in left_b if not (rep_b[lb.name[k]] == k and lb.name[k] in rep_a)], path)
    out.sort(key=lambda r: (r["path"], r["change"]))
    return out


def full_walk_diff(ctx, packfiles, ids, entries, index_items, prk, root_a, root_b, sizes=False, verify=False, slots=0):
    """What changed from snapshot root_a to snapshot root_b of one store (packfiles: list of bytes with
    their 12-byte ids, entries as unpack_headers returned them, index_items n x 44; a root may be
    None: an empty snapshot).  Returns listing_changes() of the two walks.  With sizes=True returns
    (changes, dict(only_a_blobs, only_a_bytes, only_b_blobs, only_b_bytes)): the blobs, and their
    sealed bytes (12 + length each), that only one of the two roots reaches.  A tree blob that cannot
    be read raises restore.TreeError, as a restore of that root would."""
    packfiles = [bytes(b) for b in packfiles]
    en = np.ascontiguousarray(entries, dtype=UNPACK_ENTRY_DTYPE)
    with Session(ctx, prk, packfiles, ids, en, index_items, slots=slots) as s:
        same = root_a is not None and root_b is not None and bytes(root_a) == bytes(root_b)
        la = None if root_a is None or same else s.trees(root_a, verify=verify)
        lb = None if root_b is None or same else s.trees(root_b, verify=verify)
        if sizes:
            live_a = prune.mark(s, [] if root_a is None else [root_a], verify=verify)[0].astype(bool)
            live_b = prune.mark(s, [] if root_b is None else [root_b], verify=verify)[0].astype(bool)
    ch = listing_changes(la, lb)
    if not sizes:
        return ch
    sealed = en["length"].astype(np.uint64) + np.uint64(12)
    only_a, only_b = live_a & ~live_b, live_b & ~live_a
    return ch, dict(only_a_blobs=int(only_a.sum()), only_a_bytes=int(sealed[only_a].sum()),
                    only_b_blobs=int(only_b.sum()), only_b_bytes=int(sealed[only_b].sum()))


# ------------------------------------------------------------------ the device walk
def trees(session, root_a, root_b, verify=False):
    """bw_diff_trees over an open restore Session: (records RECORD_DTYPE, names bytes, read u8 per
    entry, counts dict, errors prune.ERROR_DTYPE).  A root may be None: an empty snapshot.  The buffers
    grow until the walk fits them."""
    roots = [None if r is None else (ctypes.c_uint8 * 32).from_buffer_copy(bytes(r)) for r in (root_a, root_b)]
    read = np.zeros(max(session.n_entries, 1), dtype=np.uint8)
    cnt = _lib.BwDiffCounts()
    caps = [1024, 1 << 16, 64]
    while True:
        records = np.zeros(caps[0], dtype=RECORD_DTYPE)
        names = np.zeros(caps[1], dtype=np.uint8)
        errs = np.zeros(caps[2], dtype=ERROR_DTYPE)
        rc = session._L.bw_diff_trees(session.h, roots[0], roots[1], _lib.BW_UNPACK_VERIFY if verify else 0,
                                      records.ctypes.data_as(ctypes.POINTER(_lib.BwDiffRecord)), caps[0],
                                      names.ctypes.data_as(ctypes.c_void_p), caps[1], read.ctypes.data_as(_lib.u8p),
                                      ctypes.byref(cnt), errs.ctypes.data_as(ctypes.POINTER(_lib.BwPruneError)), caps[2])
        if rc != _lib.BW_ENOSPC:
            check(rc, session._ctx.h)
            break
        # the counts are the totals up to the level that did not fit: at least that, and twice the room
        caps = [max(2 * cap, int(n)) if n > cap else cap
                for cap, n in zip(caps, (cnt.n_records, cnt.name_bytes, cnt.n_errors))]
    counts = {f: int(getattr(cnt, f)) for f in COUNT_FIELDS}
    return (records[:counts["n_records"]], names[:counts["name_bytes"]].tobytes(), read[:session.n_entries], counts,
            errs[:counts["n_errors"]])


def record_changes(records, names):
    """The records of trees() as dicts in listing_changes' shape, plus flags and both hashes: [dict(path,
    change, flags, a, b, hash_a, hash_b, common_prefix, common_suffix, n_new)] sorted by path.  The path
    is joined through parent (a parent's record comes first); the root's path is ''.  An unreadable
    node has no name: its path ends in '?' and its hash in hex."""
    names = bytes(names)
    cols = {f: records[f].tolist() for f in ("change", "flags", "parent", "name_off", "name_len", "common_prefix",
                                              "common_suffix", "n_new")}
    sides = {x: list(zip(*[records[x][f].tolist() for f in SIDE_FIELDS])) if len(records) else [] for x in ("a", "b")}
    hashes = {x: [bytes(h) for h in records[x]["hash"]] for x in ("a", "b")}
    paths, out = [], []
    for i in range(len(records)):
        change, flags, parent = cols["change"][i], cols["flags"][i], cols["parent"][i]
        if flags & F_UNREADABLE:
            name = "?" + hashes["a" if change == REMOVED else "b"][i].hex()
        else:
            name = names[cols["name_off"][i]:cols["name_off"][i] + cols["name_len"][i]].decode("utf-8", "surrogateescape")
        if parent == NONE:
            path = ""
        else:
            path = paths[parent] + "/" + name if paths[parent] else name
        paths.append(path)
        out.append(dict(path=path, change=change, flags=flags,
                        a=None if change == ADDED else dict(zip(SIDE_FIELDS, sides["a"][i])),
                        b=None if change == REMOVED else dict(zip(SIDE_FIELDS, sides["b"][i])),
                        hash_a=None if change == ADDED else hashes["a"][i],
                        hash_b=None if change == REMOVED else hashes["b"][i],
                        common_prefix=cols["common_prefix"][i], common_suffix=cols["common_suffix"][i],
                        n_new=cols["n_new"][i]))
    out.sort(key=lambda r: (r["path"], r["change"]))
    return out


def diff(ctx, packfiles, ids, entries, index_items, prk, root_a, root_b, verify=False, slots=0):
    """What changed from snapshot root_a to snapshot root_b of one store (the arguments of
    full_walk_diff), by the device walk: (changes, errors, counts).  changes = record_changes() of the
    walk; errors = prune.ERROR_DTYPE records, which never end the call."""
    packfiles = [bytes(b) for b in packfiles]
    en = np.ascontiguousarray(entries, dtype=UNPACK_ENTRY_DTYPE)
    with Session(ctx, prk, packfiles, ids, en, index_items, slots=slots) as s:
        records, names, _, counts, errors = trees(s, root_a, root_b, verify=verify)
    return record_changes(records, names), errors, counts
