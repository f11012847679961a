"""Prune: which header entries a set of roots reaches, and packfiles of the live ones
(include/backuwup_gpu_pack.h, "prune").  The reference has no prune.

mark() walks the trees of the kept roots over an open restore Session and returns the live bit of
every header entry with per-packfile sums; choose_rewrite() is the policy (which packfiles are worth
rewriting); plan() and repack() move the live blobs of those packfiles, sealed as they are, into new
packfiles; prune() is the whole sequence over a store held as lists of bytes."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check
from .context import PACKFILE_DTYPE, UNPACK_ENTRY_DTYPE, _ptr
from .restore import REASONS, Session

STAT_DTYPE = np.dtype([("live_blobs", "<u8"), ("live_bytes", "<u8"), ("total_blobs", "<u8"), ("total_bytes", "<u8")])
ERROR_DTYPE = np.dtype([("hash", "u1", (32,)), ("parent", "u1", (32,)), ("child_pos", "<u8"), ("reason", "<u4"),
                        ("pad", "<u4")])
assert STAT_DTYPE.itemsize == ctypes.sizeof(_lib.BwPrunePackfileStat) == 32
assert ERROR_DTYPE.itemsize == ctypes.sizeof(_lib.BwPruneError) == 80
NONE = 2**64 - 1
COUNT_FIELDS = [f for f, _ in _lib.BwPruneCounts._fields_]


class PruneError(_lib.BwError):
    """The mark met damage and the caller did not allow it: .errors holds the ERROR_DTYPE records."""

    def __init__(self, errors):
        e = errors[0]
        super().__init__(_lib.BW_EFORMAT, "prune: %d errors in the kept graph, the first %s at %s" % (
            len(errors), REASONS.get(int(e["reason"]), int(e["reason"])), bytes(e["hash"]).hex()))
        self.errors = errors


def _hashes(roots):
    if isinstance(roots, np.ndarray):
        return np.ascontiguousarray(roots, dtype=np.uint8).reshape(-1, 32)
    return np.frombuffer(b"".join(bytes(r) for r in roots), dtype=np.uint8).reshape(-1, 32)


def mark(session, roots, verify=False, err_cap=None):
    """bw_prune_mark: (live u8 per entry, stats STAT_DTYPE per packfile, counts dict, errors ERROR_DTYPE).
    err_cap=None grows the error list until it fits; with a number, (rc BW_ENOSPC) is not raised:
    counts["n_errors"] then exceeds len(errors)."""
    r = _hashes(roots)
    live = np.zeros(max(session.n_entries, 1), dtype=np.uint8)
    stats = np.zeros(max(session.n_packfiles, 1), dtype=STAT_DTYPE)
    cnt = _lib.BwPruneCounts()
    cap = 64 if err_cap is None else int(err_cap)
    while True:
        errs = np.zeros(max(cap, 1), dtype=ERROR_DTYPE)
        rc = session._L.bw_prune_mark(session.h, _ptr(r), r.shape[0], _lib.BW_UNPACK_VERIFY if verify else 0,
                                      live.ctypes.data_as(_lib.u8p),
                                      stats.ctypes.data_as(ctypes.POINTER(_lib.BwPrunePackfileStat)), ctypes.byref(cnt),
                                      errs.ctypes.data_as(ctypes.POINTER(_lib.BwPruneError)), cap)
        if rc != _lib.BW_ENOSPC:
            check(rc, session._ctx.h)
        if rc == _lib.BW_OK or err_cap is not None:
            break
        cap = int(cnt.n_errors)
    counts = {f: int(getattr(cnt, f)) for f in COUNT_FIELDS}
    return live[:session.n_entries], stats[:session.n_packfiles], counts, errs[:min(cap, counts["n_errors"])]


def choose_rewrite(stats, max_dead_fraction=0.0):
    """A packfile is rewritten when dead_bytes / total_bytes exceeds the threshold."""
    total = stats["total_bytes"].astype(np.float64)
    dead = total - stats["live_bytes"].astype(np.float64)
    return ((total > 0) & (dead > max_dead_fraction * total)).astype(np.uint8)


def plan(entries, packfile_table, live, rewrite):
    """bw_prune_plan: (order u64, plan PACKFILE_DTYPE, total bytes).  packfile_table: PACKFILE_DTYPE
    (size and header_len of every old packfile)."""
    L = _lib.load()
    en = np.ascontiguousarray(entries, dtype=UNPACK_ENTRY_DTYPE)
    pf = np.ascontiguousarray(packfile_table, dtype=PACKFILE_DTYPE)
    lv = np.ascontiguousarray(live, dtype=np.uint8)
    rw = np.ascontiguousarray(rewrite, dtype=np.uint8)
    assert lv.size == en.size and rw.size == pf.size
    nm, nn, total, bad = (ctypes.c_uint64() for _ in range(4))
    order, pl = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=PACKFILE_DTYPE)
    caps = (0, 0)
    while True:
        rc = L.bw_prune_plan(en.ctypes.data_as(ctypes.POINTER(_lib.BwUnpackEntry)), en.size,
                             pf.ctypes.data_as(ctypes.POINTER(_lib.BwPackfile)), pf.size, lv.ctypes.data_as(_lib.u8p),
                             rw.ctypes.data_as(_lib.u8p), order.ctypes.data_as(_lib.u64p), caps[0], ctypes.byref(nm),
                             pl.ctypes.data_as(ctypes.POINTER(_lib.BwPackfile)), caps[1], ctypes.byref(nn),
                             ctypes.byref(total), ctypes.byref(bad))
        if rc == _lib.BW_EINVAL and bad.value != NONE:
            err = _lib.BwError(rc, "prune: live entry %d leaves its packfile" % bad.value)
            err.bad_entry = bad.value
            raise err
        if rc != _lib.BW_ENOSPC:
            check(rc)
            return order[:nm.value], pl[:nn.value], total.value
        caps = (nm.value, nn.value)
        order, pl = np.zeros(max(caps[0], 1), dtype=np.uint64), np.zeros(max(caps[1], 1), dtype=PACKFILE_DTYPE)


def _ids(new_ids, n):
    b = b"".join(bytes(i) for i in new_ids[:n]) if not isinstance(new_ids, np.ndarray) else new_ids.tobytes()[:12 * n]
    if len(b) < 12 * n:
        raise ValueError("prune: %d new packfile ids needed" % n)
    return np.frombuffer(b or b"\0", dtype=np.uint8)


def repack(session, order, pl, new_ids):
    """bw_prune_repack: the new packfiles as a list of bytes."""
    order = np.ascontiguousarray(order, dtype=np.uint64)
    pl = np.ascontiguousarray(pl, dtype=PACKFILE_DTYPE)
    total = int(pl["offset"][-1] + pl["size"][-1]) if pl.size else 0
    out = np.zeros(max(total, 1), dtype=np.uint8)
    ids = _ids(new_ids, pl.size)
    check(session._L.bw_prune_repack(session.h, order.ctypes.data_as(_lib.u64p), order.size,
                                     pl.ctypes.data_as(ctypes.POINTER(_lib.BwPackfile)), pl.size, _ptr(ids), _ptr(out)),
          session._ctx.h)
    return [out[int(p["offset"]):int(p["offset"] + p["size"])].tobytes() for p in pl]


def repack_device(session, order, pl, new_ids, d_out):
    """bw_prune_repack_device into d_out (a device pointer)."""
    order = np.ascontiguousarray(order, dtype=np.uint64)
    pl = np.ascontiguousarray(pl, dtype=PACKFILE_DTYPE)
    ids = _ids(new_ids, pl.size)
    check(session._L.bw_prune_repack_device(session.h, order.ctypes.data_as(_lib.u64p), order.size,
                                            pl.ctypes.data_as(ctypes.POINTER(_lib.BwPackfile)), pl.size, _ptr(ids),
                                            ctypes.c_void_p(d_out)), session._ctx.h)


def packfile_table(packfiles):
    """PACKFILE_DTYPE of packfiles held as bytes, back to back: offset, size and the u64 header_len prefix."""
    tab = np.zeros(len(packfiles), dtype=PACKFILE_DTYPE)
    off = 0
    for i, b in enumerate(packfiles):
        tab[i]["offset"], tab[i]["size"] = off, len(b)
        tab[i]["header_len"] = int.from_bytes(bytes(b[:8]), "little") if len(b) >= 8 else 0
        off += len(b)
    return tab


def prune(ctx, packfiles, ids, entries, index_items, prk, roots, new_ids, max_dead_fraction=0.0, verify=False,
          allow_errors=False, slots=0, last_file_num=None):
    """Keep `roots`, drop what no kept root reaches.  packfiles: list of bytes with their 12-byte ids,
    entries as unpack_headers returned them, index_items n x 44.  Returns (packs, ids, index_items,
    report): the kept packfiles verbatim, then the new ones (ids from new_ids, in order); every old
    index item whose packfile id is not a rewritten one, in the old order, then (hash, new id) per
    moved blob.  Raises PruneError when the mark reported an error, unless allow_errors: a prune over
    a damaged graph must be a decision.  With last_file_num the index files are built too
    (report["index_files"], from index_files_build)."""
    packfiles = [bytes(b) for b in packfiles]
    ids = [bytes(i) for i in ids]
    items = np.ascontiguousarray(np.asarray(index_items, dtype=np.uint8).reshape(-1, 44))
    en = np.ascontiguousarray(entries, dtype=UNPACK_ENTRY_DTYPE)
    with Session(ctx, prk, packfiles, ids, en, items, slots=slots) as s:
        live, stats, counts, errors = mark(s, roots, verify=verify)
        if len(errors) and not allow_errors:
            raise PruneError(errors)
        rewrite = choose_rewrite(stats, max_dead_fraction)
        order, pl, total = plan(en, packfile_table(packfiles), live, rewrite)
        if pl.size > len(new_ids):
            raise ValueError("prune: %d new packfile ids needed" % pl.size)
        new_packs = repack(s, order, pl, new_ids) if pl.size else []
    used = [bytes(i) for i in new_ids[:pl.size]]
    gone = {ids[p] for p in range(len(ids)) if rewrite[p]}
    keep = [p for p in range(len(ids)) if not rewrite[p]]
    id12 = np.dtype([("lo", "<u8"), ("hi", "<u4")])  # a 12-byte id as one sortable record
    gone_ids = np.frombuffer(b"".join(sorted(gone)), dtype=id12)
    keep_item = ~np.isin(np.ascontiguousarray(items[:, 32:]).view(id12).reshape(-1), gone_ids)
    moved = np.zeros((order.size, 44), dtype=np.uint8)
    for g, p in enumerate(pl):
        f, n = int(p["first_blob"]), int(p["n_blobs"])
        moved[f:f + n, :32] = en["hash"][order[f:f + n].astype(np.int64)]
        moved[f:f + n, 32:] = np.frombuffer(used[g], dtype=np.uint8)
    new_items = np.concatenate([items[keep_item], moved])
    report = dict(live=live, stats=stats, counts=counts, errors=errors, rewrite=rewrite, order=order, plan=pl,
                  total_bytes=total)
    if last_file_num is not None:
        report["index_files"] = ctx.index_files_build(prk, new_items, last_file_num)
    return [packfiles[p] for p in keep] + new_packs, [ids[p] for p in keep] + used, new_items, report
