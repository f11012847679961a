"""Find: which paths of which snapshots match a set of patterns (include/backuwup_gpu_pack.h, "find").
The reference cannot ask it; restic answers it with find and restore --include.

paths() is bw_find_paths over an open restore Session with buffers that grow until the walk fits them;
find() is the whole question over a store held as lists of bytes; restore_paths() finds with SUBTREE |
CHUNKS and hands the hit files' chunk rows to Session.files: a partial restore."""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import check
from .context import UNPACK_ENTRY_DTYPE, _ptr
from .prune import ERROR_DTYPE, _hashes
from .restore import Session, _set_mtime, DEFAULT_WINDOW

F_HIT, F_UNREADABLE, F_TRUNCATED, F_CYCLIC, F_PRUNED = (_lib.BW_FIND_HIT, _lib.BW_FIND_UNREADABLE, _lib.BW_FIND_TRUNCATED,
                                                        _lib.BW_FIND_CYCLIC, _lib.BW_FIND_PRUNED)
NONE = 2**64 - 1
RECORD_DTYPE = np.dtype([("hash", "u1", (32,)), ("root", "<u8"), ("parent", "<u8"), ("name_off", "<u8"), ("name_len", "<u8"),
                         ("kind", "<u4"), ("meta_flags", "<u4"), ("size", "<u8"), ("mtime", "<u8"), ("ctime", "<u8"),
                         ("child_first", "<u8"), ("n_children", "<u8"), ("patterns", "<u4"), ("flags", "<u4")])
ROOT_DTYPE = np.dtype([("n_records", "<u8"), ("n_hits", "<u8"), ("n_hit_files", "<u8"), ("hit_bytes", "<u8"),
                       ("n_unreadable", "<u8")])
assert RECORD_DTYPE.itemsize == ctypes.sizeof(_lib.BwFindRecord) == 120
assert ROOT_DTYPE.itemsize == ctypes.sizeof(_lib.BwFindRoot) == 40
COUNT_FIELDS = [f for f, _ in _lib.BwFindCounts._fields_]


def flags_of(icase=False, subtree=False, chunks=False, verify=False):
    return ((_lib.BW_FIND_ICASE if icase else 0) | (_lib.BW_FIND_SUBTREE if subtree else 0) |
            (_lib.BW_FIND_CHUNKS if chunks else 0) | (_lib.BW_UNPACK_VERIFY if verify else 0))


def kinds_of(kinds):
    """None = both; an int is the query's mask itself; else an iterable of 'file' / 'dir' (or BW_TREE_FILE /
    BW_TREE_DIR)."""
    if kinds is None:
        return 0
    if isinstance(kinds, int):
        return kinds
    names = {"file": _lib.BW_TREE_FILE, "dir": _lib.BW_TREE_DIR}
    return sum({1 << (names[k] if isinstance(k, str) else int(k)) for k in kinds})


class Query:
    """A bw_find_query and the arrays it points into."""

    def __init__(self, patterns, kinds=None, size=None, mtime=None):
        pats = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in patterns]
        self.n = len(pats)
        self._bytes = np.frombuffer(b"".join(pats) + b"\0", dtype=np.uint8).copy()
        self._off = np.concatenate([[0], np.cumsum([len(p) for p in pats], dtype=np.int64)]).astype(np.uint64)
        lo_s, hi_s = (0, NONE) if size is None else size
        lo_m, hi_m = (0, NONE) if mtime is None else mtime
        self.q = _lib.BwFindQuery(self._bytes.ctypes.data, self._off.ctypes.data, self.n, kinds_of(kinds), int(lo_s), int(hi_s),
                                  int(lo_m), int(hi_m))


def paths(session, roots, patterns, icase=False, subtree=False, chunks=False, verify=False, kinds=None, size=None,
          mtime=None, caps=None):
    """bw_find_paths: (records RECORD_DTYPE, names bytes, chunk rows n x 32, per_root ROOT_DTYPE, counts
    dict, errors ERROR_DTYPE).  The buffers grow until the walk fits them; caps = (records, name bytes,
    chunk rows, errors) to start from."""
    r = _hashes(roots)
    query = Query(patterns, kinds, size, mtime)
    flags = flags_of(icase, subtree, chunks, verify)
    per_root = np.zeros(max(r.shape[0], 1), dtype=ROOT_DTYPE)
    cnt = _lib.BwFindCounts()
    caps = [1024, 1 << 16, 1024, 64] if caps is None else [max(int(x), 1) for x in caps]
    while True:
        records = np.zeros(caps[0], dtype=RECORD_DTYPE)
        names = np.zeros(caps[1], dtype=np.uint8)
        rows = np.zeros((caps[2], 32), dtype=np.uint8)
        errs = np.zeros(caps[3], dtype=ERROR_DTYPE)
        rc = session._L.bw_find_paths(session.h, _ptr(r), r.shape[0], ctypes.byref(query.q), flags,
                                      records.ctypes.data_as(ctypes.POINTER(_lib.BwFindRecord)), caps[0],
                                      names.ctypes.data_as(ctypes.c_void_p), caps[1], rows.ctypes.data_as(ctypes.c_void_p), caps[2],
                                      per_root.ctypes.data_as(ctypes.POINTER(_lib.BwFindRoot)), ctypes.byref(cnt),
                                      errs.ctypes.data_as(ctypes.POINTER(_lib.BwPruneError)), caps[3])
        if rc != _lib.BW_ENOSPC:
            check(rc, session._ctx.h)
            break
        # the counts are the totals up to the level that did not fit: at least that, and twice the room
        caps = [max(2 * cap, int(n)) if n > cap else cap
                for cap, n in zip(caps, (cnt.n_records, cnt.name_bytes, cnt.n_chunks, cnt.n_errors))]
    counts = {f: int(getattr(cnt, f)) for f in COUNT_FIELDS}
    return (records[:counts["n_records"]], names[:counts["name_bytes"]].tobytes(), rows[:counts["n_chunks"]],
            per_root[:r.shape[0]], counts, errs[:counts["n_errors"]])


def record_paths(records, names):
    """The path of every record, joined through parent (a parent's record comes first); a root's is ''.
    An unreadable item has no name: its path ends in '?' and its hash in hex."""
    names = bytes(names)
    cols = {f: records[f].tolist() for f in ("parent", "name_off", "name_len", "flags")}
    joined = []
    for i in range(len(records)):
        parent = cols["parent"][i]
        if cols["flags"][i] & F_UNREADABLE:
            name = "?" + bytes(records["hash"][i]).hex()
        else:
            name = names[cols["name_off"][i]:cols["name_off"][i] + cols["name_len"][i]].decode("utf-8", "surrogateescape")
        if parent == NONE:
            joined.append(name if cols["flags"][i] & F_UNREADABLE else "")
        else:
            joined.append(joined[parent] + "/" + name if joined[parent] else name)
    return joined


def find(ctx, packfiles, ids, entries, index_items, prk, roots, patterns, icase=False, subtree=False, kinds=None, size=None,
         mtime=None, verify=False, slots=0):
    """The hits under the snapshots `roots` of one store (packfiles: list of bytes with their 12-byte ids,
    entries as unpack_headers returned them, index_items n x 44).  Returns (per root the list of dict(path,
    kind, size, mtime, ctime, meta_flags, patterns, flags, hash) in record order, counts, errors)."""
    packfiles = [bytes(b) for b in packfiles]
    en = np.ascontiguousarray(entries, dtype=UNPACK_ENTRY_DTYPE)
    roots = [bytes(r) for r in roots]
    with Session(ctx, prk, packfiles, ids, en, index_items, slots=slots) as s:
        records, names, _, _, counts, errors = paths(s, roots, patterns, icase=icase, subtree=subtree, verify=verify,
                                                     kinds=kinds, size=size, mtime=mtime)
    joined = record_paths(records, names)
    out = [[] for _ in roots]
    for i in np.nonzero(records["flags"] & F_HIT)[0].tolist():
        r = records[i]
        out[int(r["root"])].append(dict(path=joined[i], kind=int(r["kind"]), size=int(r["size"]), mtime=int(r["mtime"]),
                                        ctime=int(r["ctime"]), meta_flags=int(r["meta_flags"]), patterns=int(r["patterns"]),
                                        flags=int(r["flags"]), hash=bytes(r["hash"])))
    return out, counts, errors


def restore_paths(ctx, packfiles, ids, entries, index_items, prk, root_hash, patterns, destination_dir=None, verify=False,
                  icase=False, window=DEFAULT_WINDOW, slots=0, counts=None, tree_errors=None):
    """restore.unpack for the part of a snapshot that the patterns match: a file that matches, and
    everything below a directory that matches.  Result as unpack's: ({relative path: bytes}, errors), or with
    destination_dir, which is created, the matched directories created below it, the files written (the
    directories above them created, their mtimes set), the matched directories' mtimes set and (None, errors).
      errors = [(path, status, bad child)]: unpack's entries for the files that failed, and, where unpack
    raises TreeError, an entry (path, reason, NONE) for every item of the walk that is UNREADABLE (its path ends
    in '?' and its hash; it may have been a match, its name is not known), CYCLIC or TRUNCATED (a Dir: what its
    lost pieces held is missing; a File: its bytes end where the lost piece begins, they are kept as unpack keeps
    a partial file, and its mtime is not set).  reason is the tree error's; for a TRUNCATED item it is known
    when the lost piece follows the first directly, else 0.  tree_errors: a list that receives find's errors
    as (hash, parent, child_pos, reason); counts: a dict that receives find's counts."""
    with Session(ctx, prk, [bytes(b) for b in packfiles], ids, np.ascontiguousarray(entries, dtype=UNPACK_ENTRY_DTYPE),
                 index_items, slots=slots) as s:
        records, names, rows, _, fcounts, ferrs = paths(s, [bytes(root_hash)], patterns, icase=icase, subtree=True, chunks=True,
                                                        verify=verify)
        joined = record_paths(records, names)
        is_file = records["kind"] == _lib.BW_TREE_FILE
        readable = (records["flags"] & F_UNREADABLE) == 0
        hits = np.nonzero(((records["flags"] & F_HIT) != 0) & is_file & readable)[0].tolist()
        dirs = np.nonzero((records["patterns"] != 0) & ~is_file & readable)[0].tolist()
        n = records["n_children"][hits].astype(np.uint64)
        ff = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
        sel = np.concatenate([rows[int(records["child_first"][i]):int(records["child_first"][i] + records["n_children"][i])]
                              for i in hits] + [np.zeros((0, 32), dtype=np.uint8)])
        data, status, bad = s.files(sel, ff, window=window, flags=_lib.BW_UNPACK_VERIFY if verify else 0)
    raw = [(bytes(e["hash"]), bytes(e["parent"]), int(e["child_pos"]), int(e["reason"])) for e in ferrs]
    if tree_errors is not None:
        tree_errors.extend(raw)
    own = {h: reason for h, _, _, reason in reversed(raw)}                        # the item's own reference
    later = {by: reason for _, by, pos, reason in reversed(raw) if pos == NONE}   # the piece behind this one
    result, errors = ({} if destination_dir is None else None), []
    for i in np.nonzero(records["flags"] & (F_UNREADABLE | F_CYCLIC | F_TRUNCATED))[0].tolist():
        h, fl = bytes(records["hash"][i]), int(records["flags"][i])
        if fl & (F_UNREADABLE | F_CYCLIC):
            errors.append((joined[i], own.get(h, 0), NONE))
        if fl & F_TRUNCATED:
            errors.append((joined[i], later.get(h, 0), NONE))
    if destination_dir is not None:
        os.makedirs(destination_dir, exist_ok=True)
        for i in dirs:
            p = os.path.join(destination_dir, joined[i])
            os.makedirs(p, exist_ok=True)
    for k, i in enumerate(hits):
        if status[k]:
            errors.append((joined[i], int(status[k]), int(bad[k])))
        if destination_dir is None:
            result[joined[i]] = data[k]
            continue
        p = os.path.join(destination_dir, joined[i])
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as fh:
            fh.write(data[k])
        if not status[k] and not int(records["flags"][i]) & F_TRUNCATED:
            _set_mtime(p, {"flags": int(records["meta_flags"][i]), "mtime": int(records["mtime"][i])})
    if destination_dir is not None:  # last, so that the files written below them do not move them
        for i in dirs:
            _set_mtime(os.path.join(destination_dir, joined[i]), {"flags": int(records["meta_flags"][i]), "mtime": int(records["mtime"][i])})
    if counts is not None:
        counts.update(fcounts)
    return result, errors
