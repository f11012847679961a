"""Impact: which files of which snapshots a set of lost blobs takes down (include/backuwup_gpu_pack.h,
"impact").  The reference cannot ask it; restic answers it with find --blob / --pack.

mark() gives every entry the roots reach its taint over an open restore Session, opening each distinct
tree blob once and never an entry of `bad`; paths() goes down from the affected roots and opens only
affected paths; bad_from_check() and lost_packfiles() make the `bad` vector, from a check report (what
is damaged now) or from packfile positions (what if this peer disappears); impact() is the whole
sequence over a store held as lists of bytes."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check
from .context import UNPACK_ENTRY_DTYPE, _ptr
from .prune import ERROR_DTYPE, _hashes
from .restore import Session

SELF, BELOW = _lib.BW_IMPACT_SELF, _lib.BW_IMPACT_BELOW
F_UNREADABLE, F_TRUNCATED, F_CYCLIC = _lib.BW_IMPACT_UNREADABLE, _lib.BW_IMPACT_TRUNCATED, _lib.BW_IMPACT_CYCLIC
NONE = 2**64 - 1
RECORD_DTYPE = np.dtype([("hash", "u1", (32,)), ("root", "<u8"), ("parent", "<u8"), ("name_off", "<u8"), ("name_len", "<u8"),
                         ("kind", "<u4"), ("meta_flags", "<u4"), ("size", "<u8"), ("mtime", "<u8"), ("ctime", "<u8"),
                         ("n_children", "<u8"), ("n_affected", "<u8"), ("first_affected", "<u8"), ("flags", "<u4"),
                         ("pad", "<u4")])
ROOT_DTYPE = np.dtype([("n_records", "<u8"), ("n_files", "<u8"), ("n_unreadable", "<u8"), ("lost_chunk_refs", "<u8")])
assert RECORD_DTYPE.itemsize == ctypes.sizeof(_lib.BwImpactRecord) == 128
assert ROOT_DTYPE.itemsize == ctypes.sizeof(_lib.BwImpactRoot) == 32
MARK_FIELDS = [f for f, _ in _lib.BwImpactCounts._fields_]
PATHS_FIELDS = [f for f, _ in _lib.BwImpactPathsCounts._fields_]


def _bad(session, bad):
    if bad is None:
        return None
    b = np.ascontiguousarray(np.asarray(bad) != 0, dtype=np.uint8)
    if b.size != session.n_entries:
        raise ValueError("impact: bad holds %d bytes for %d entries" % (b.size, session.n_entries))
    return b if b.size else None


def mark(session, roots, bad=None, verify=False, err_cap=None):
    """bw_impact_mark: (taint u8 per entry, root_affected u8 per root, counts dict, errors ERROR_DTYPE).
    bad: one value per entry, nonzero = treat its bytes as lost, or None.  err_cap=None grows the error
    list until it fits; with a number, BW_ENOSPC is not raised: counts["n_errors"] then exceeds len(errors)."""
    r = _hashes(roots)
    b = _bad(session, bad)
    taint = np.zeros(max(session.n_entries, 1), dtype=np.uint8)
    affected = np.zeros(max(r.shape[0], 1), dtype=np.uint8)
    cnt = _lib.BwImpactCounts()
    cap = 64 if err_cap is None else int(err_cap)
    while True:
        errs = np.zeros(max(cap, 1), dtype=ERROR_DTYPE)
        rc = session._L.bw_impact_mark(session.h, _ptr(r), r.shape[0], None if b is None else b.ctypes.data_as(_lib.u8p),
                                       _lib.BW_UNPACK_VERIFY if verify else 0, taint.ctypes.data_as(_lib.u8p),
                                       affected.ctypes.data_as(_lib.u8p), ctypes.byref(cnt),
                                       errs.ctypes.data_as(ctypes.POINTER(_lib.BwPruneError)), cap)
        if rc != _lib.BW_ENOSPC:
            check(rc, session._ctx.h)
        if rc == _lib.BW_OK or err_cap is not None:
            break
        cap = int(cnt.n_errors)
    counts = {f: int(getattr(cnt, f)) for f in MARK_FIELDS}
    return taint[:session.n_entries], affected[:r.shape[0]], counts, errs[:min(cap, counts["n_errors"])]


def paths(session, roots, taint, verify=False, caps=None):
    """bw_impact_paths: (records RECORD_DTYPE, names bytes, per_root ROOT_DTYPE, counts dict, errors
    ERROR_DTYPE).  taint as mark() returned it.  The buffers grow until the walk fits them; caps = (records,
    name bytes, errors) to start from, for a caller that knows what the walk needs."""
    r = _hashes(roots)
    t = np.ascontiguousarray(taint, dtype=np.uint8)
    if t.size != session.n_entries:
        raise ValueError("impact: taint holds %d bytes for %d entries" % (t.size, session.n_entries))
    per_root = np.zeros(max(r.shape[0], 1), dtype=ROOT_DTYPE)
    cnt = _lib.BwImpactPathsCounts()
    caps = [1024, 1 << 16, 64] if caps is None else [max(int(x), 1) for x in caps]
    while True:
        records = np.zeros(caps[0], dtype=RECORD_DTYPE)
        names = np.zeros(caps[1], dtype=np.uint8)
        errs = np.zeros(caps[2], dtype=ERROR_DTYPE)
        rc = session._L.bw_impact_paths(session.h, _ptr(r), r.shape[0], t.ctypes.data_as(_lib.u8p) if t.size else None,
                                        _lib.BW_UNPACK_VERIFY if verify else 0,
                                        records.ctypes.data_as(ctypes.POINTER(_lib.BwImpactRecord)), caps[0],
                                        names.ctypes.data_as(ctypes.c_void_p), caps[1],
                                        per_root.ctypes.data_as(ctypes.POINTER(_lib.BwImpactRoot)), ctypes.byref(cnt),
                                        errs.ctypes.data_as(ctypes.POINTER(_lib.BwPruneError)), caps[2])
        if rc != _lib.BW_ENOSPC:
            check(rc, session._ctx.h)
            break
        # the counts are the totals up to the level that did not fit: at least that, and twice the room
        caps = [max(2 * cap, int(n)) if n > cap else cap
                for cap, n in zip(caps, (cnt.n_records, cnt.name_bytes, cnt.n_errors))]
    counts = {f: int(getattr(cnt, f)) for f in PATHS_FIELDS}
    return (records[:counts["n_records"]], names[:counts["name_bytes"]].tobytes(), per_root[:r.shape[0]], counts,
            errs[:counts["n_errors"]])


def bad_from_check(report, entries):
    """The `bad` vector of a check.check() report: the entries with a failed data status or a structure
    flag, and every entry of a packfile in bad_packfiles."""
    en = np.ascontiguousarray(entries, dtype=UNPACK_ENTRY_DTYPE)
    bad = np.asarray(report["entry_flags"]) != 0
    st = report.get("data_status")
    if st is not None:
        st = np.asarray(st)
        bad |= (st != _lib.BW_UNPACK_OK) & (st != _lib.BW_CHECK_SKIPPED)
    bad |= lost_packfiles(en, report["bad_packfiles"]) != 0
    return bad.astype(np.uint8)


def lost_packfiles(entries, positions):
    """The what-if vector: every entry of the packfiles at these positions."""
    en = np.ascontiguousarray(entries, dtype=UNPACK_ENTRY_DTYPE)
    return np.isin(en["packfile"], np.asarray(list(positions), dtype=np.int64)).astype(np.uint8)


def record_paths(records, names, n_roots):
    """Per root the list of (path, kind, flags, n_affected, n_children), in record order.  The path is
    joined through parent (a parent's record comes first); a root's path is ''.  An unreadable item has no
    name: its path ends in '?' and its hash in hex."""
    names = bytes(names)
    out = [[] for _ in range(n_roots)]
    joined = []
    cols = {f: records[f].tolist() for f in ("root", "parent", "name_off", "name_len", "kind", "flags", "n_affected",
                                              "n_children")}
    for i in range(len(records)):
        flags, parent = cols["flags"][i], cols["parent"][i]
        if flags & F_UNREADABLE:
            name = "?" + bytes(records["hash"][i]).hex()
        else:
            name = names[cols["name_off"][i]:cols["name_off"][i] + cols["name_len"][i]].decode("utf-8", "surrogateescape")
        path = "" if parent == NONE else (joined[parent] + "/" + name if joined[parent] else name)
        if parent == NONE and flags & F_UNREADABLE:
            path = name
        joined.append(path)
        out[cols["root"][i]].append((path, cols["kind"][i], flags, cols["n_affected"][i], cols["n_children"][i]))
    return out


def impact(ctx, packfiles, ids, entries, index_items, prk, roots, bad=None, verify=False, slots=0):
    """What `bad` costs the snapshots `roots` of one store (packfiles: list of bytes with their 12-byte
    ids, entries as unpack_headers returned them, index_items n x 44).  Returns (per root the list of
    (path, kind, flags, n_affected, n_children), the mark's counts, the mark's errors)."""
    packfiles = [bytes(b) for b in packfiles]
    en = np.ascontiguousarray(entries, dtype=UNPACK_ENTRY_DTYPE)
    roots = [bytes(r) for r in roots]
    with Session(ctx, prk, packfiles, ids, en, index_items, slots=slots) as s:
        taint, _, counts, errors = mark(s, roots, bad, verify=verify)
        records, names, _, _, _ = paths(s, roots, taint, verify=verify)
    return record_paths(records, names, len(roots)), counts, errors
