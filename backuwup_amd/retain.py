"""Retain: which snapshots keep each blob alive, and what forgetting a set of them frees
(include/backuwup_gpu_pack.h, "retain").  The reference cannot ask it; restic answers it with stats and
forget --dry-run.

mark() walks all roots at once over an open restore Session, opening each distinct tree blob once, and
gives every header entry the set of roots that reach it, with per root what it reaches and what it alone
holds; drop() answers "what if these roots are forgotten" from those sets alone: the live vector and the
per-packfile sums prune.mark over the kept roots would give, ready for prune.plan; mask_of() builds the
words of one root set; retain() is the whole sequence over a store held as lists of bytes."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check
from .context import UNPACK_ENTRY_DTYPE, _ptr
from .prune import ERROR_DTYPE, STAT_DTYPE, _hashes
from .restore import Session

MAX_ROOTS = _lib.BW_RETAIN_MAX_ROOTS
ROOT_DTYPE = np.dtype([("reached_blobs", "<u8"), ("reached_bytes", "<u8"), ("unique_blobs", "<u8"), ("unique_bytes", "<u8"),
                       ("n_damaged", "<u8"), ("status", "<u4"), ("pad", "<u4")])
FREED_DTYPE = np.dtype([("freed_blobs", "<u8"), ("freed_bytes", "<u8"), ("live_blobs", "<u8"), ("live_bytes", "<u8")])
assert ROOT_DTYPE.itemsize == ctypes.sizeof(_lib.BwRetainRoot) == 48
assert FREED_DTYPE.itemsize == ctypes.sizeof(_lib.BwRetainFreed) == 32
COUNT_FIELDS = [f for f, _ in _lib.BwRetainCounts._fields_]


def words(n_roots):
    """W: the u64 words of one root set."""
    return max(1, (int(n_roots) + 63) // 64)


def mask_of(indices, n_roots):
    """The W words of the set of these root indices."""
    out = np.zeros(words(n_roots), dtype=np.uint64)
    for r in indices:
        r = int(r)
        if not 0 <= r < n_roots:
            raise ValueError("retain: root %d of %d" % (r, n_roots))
        out[r // 64] |= np.uint64(1 << (r % 64))
    return out


def roots_of(mask):
    """The root indices of one set's words, ascending."""
    return [64 * w + b for w, x in enumerate(np.asarray(mask, dtype=np.uint64).tolist()) for b in range(64) if x >> b & 1]


def mark(session, roots, verify=False, err_cap=None):
    """bw_retain_mark: (masks u64 (n_entries, W), damaged u8 per entry, per_root ROOT_DTYPE, counts dict,
    errors ERROR_DTYPE).  err_cap=None grows the error list until it fits; with a number, BW_ENOSPC is
    not raised: counts["n_errors"] then exceeds len(errors)."""
    r = _hashes(roots)
    n, W = r.shape[0], words(r.shape[0])
    masks = np.zeros((max(session.n_entries, 1), W), dtype=np.uint64)
    damaged = np.zeros(max(session.n_entries, 1), dtype=np.uint8)
    per_root = np.zeros(max(n, 1), dtype=ROOT_DTYPE)
    cnt = _lib.BwRetainCounts()
    cap = 64 if err_cap is None else int(err_cap)
    while True:
        errs = np.zeros(max(cap, 1), dtype=ERROR_DTYPE)
        rc = session._L.bw_retain_mark(session.h, _ptr(r), n, _lib.BW_UNPACK_VERIFY if verify else 0,
                                       masks.ctypes.data_as(_lib.u64p), damaged.ctypes.data_as(_lib.u8p),
                                       per_root.ctypes.data_as(ctypes.POINTER(_lib.BwRetainRoot)), ctypes.byref(cnt),
                                       errs.ctypes.data_as(ctypes.POINTER(_lib.BwPruneError)), cap)
        if rc != _lib.BW_ENOSPC:
            check(rc, session._ctx.h)
        if rc == _lib.BW_OK or err_cap is not None:
            break
        cap = int(cnt.n_errors)
    counts = {f: int(getattr(cnt, f)) for f in COUNT_FIELDS}
    return masks[:session.n_entries], damaged[:session.n_entries], per_root[:n], counts, errs[:min(cap, counts["n_errors"])]


def drop(session, masks, n_roots, drop_sets, want_live=True):
    """bw_retain_drop: (live u8 (n_sets, n_entries) or None, stats STAT_DTYPE (n_sets, n_packfiles), freed
    FREED_DTYPE per set).  drop_sets: one list of root indices per question."""
    W = words(n_roots)
    m = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, W)
    if m.shape[0] != session.n_entries:
        raise ValueError("retain: masks hold %d rows for %d entries" % (m.shape[0], session.n_entries))
    sets = [mask_of(d, n_roots) for d in drop_sets]
    n_sets = len(sets)
    d = np.ascontiguousarray(np.stack(sets) if sets else np.zeros((1, W), dtype=np.uint64))
    # a row's stride is n_entries (n_packfiles) whenever the library writes one
    live = np.zeros((max(n_sets, 1), max(session.n_entries, 1)), dtype=np.uint8) if want_live else None
    stats = np.zeros((max(n_sets, 1), max(session.n_packfiles, 1)), dtype=STAT_DTYPE)
    freed = np.zeros(max(n_sets, 1), dtype=FREED_DTYPE)
    check(session._L.bw_retain_drop(session.h, m.ctypes.data_as(_lib.u64p) if m.size else None, int(n_roots),
                                    d.ctypes.data_as(_lib.u64p), n_sets,
                                    None if live is None else live.ctypes.data_as(_lib.u8p),
                                    stats.ctypes.data_as(ctypes.POINTER(_lib.BwPrunePackfileStat)),
                                    freed.ctypes.data_as(ctypes.POINTER(_lib.BwRetainFreed))), session._ctx.h)
    return (None if live is None else live[:n_sets, :session.n_entries]), stats[:n_sets, :session.n_packfiles], freed[:n_sets]


def retain(ctx, packfiles, ids, entries, index_items, prk, roots, drop_sets=(), verify=False, slots=0):
    """What each snapshot of `roots` costs, and what forgetting each of `drop_sets` frees, over one store
    (packfiles: list of bytes with their 12-byte ids, entries as unpack_headers returned them,
    index_items n x 44).  Returns a dict: masks, damaged, per_root, counts, errors as mark() gives them,
    and live, stats, freed as drop() gives them for drop_sets."""
    packfiles = [bytes(b) for b in packfiles]
    en = np.ascontiguousarray(entries, dtype=UNPACK_ENTRY_DTYPE)
    roots = [bytes(r) for r in roots]
    with Session(ctx, prk, packfiles, ids, en, index_items, slots=slots) as s:
        masks, damaged, per_root, counts, errors = mark(s, roots, verify=verify)
        live, stats, freed = drop(s, masks, len(roots), list(drop_sets))
    return dict(masks=masks, damaged=damaged, per_root=per_root, counts=counts, errors=errors, live=live, stats=stats,
                freed=freed)
