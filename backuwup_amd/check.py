"""Check: is a store sound, are these bytes still the bytes that were sealed
(include/backuwup_gpu_pack.h, "check").  The reference has no check.

auth() recomputes AES-GCM tags without decrypting; structure() cross-checks the headers and the index
items of an open restore Session and the layout of every blob section, without reading a blob byte;
data() reads every selected entry's bytes (mode "auth": tags only, mode "full": the unpack chain with
verify, tree blobs parsed); check() is the whole sequence over a store held as lists of bytes."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check as _check
from .context import UNPACK_ENTRY_DTYPE, _as_u8, _ptr
from .restore import Session

STAT_DTYPE = np.dtype([("n_entries", "<u8"), ("n_range", "<u8"), ("n_order", "<u8"), ("n_unindexed", "<u8"),
                       ("n_shadowed", "<u8"), ("claimed_bytes", "<u8"), ("section_bytes", "<u8"), ("tail", "<i8")])
assert STAT_DTYPE.itemsize == ctypes.sizeof(_lib.BwCheckPackfileStat) == 64
assert ctypes.sizeof(_lib.BwCheckCounts) == 96
COUNT_FIELDS = [f for f, _ in _lib.BwCheckCounts._fields_]
MODES = {"auth": _lib.BW_CHECK_AUTH, "full": _lib.BW_CHECK_FULL}


def _auth_tables(src_off, src_len, infos, nonces):
    so = np.ascontiguousarray(src_off, dtype=np.uint64)
    sl = np.ascontiguousarray(src_len, dtype=np.uint64)
    n = len(so)
    info = np.ascontiguousarray(np.asarray(infos, dtype=np.uint8).reshape(n, -1)) if n else np.zeros((0, 0), np.uint8)
    non = np.ascontiguousarray(np.asarray(nonces, dtype=np.uint8).reshape(n, 12)) if n else np.zeros((0, 12), np.uint8)
    assert len(sl) == n
    return so, sl, info, non, n


def auth(ctx, prk, src, src_off, src_len, infos, nonces):
    """bw_auth: ok u8 per item, 1 exactly where Context.seal(open_=True) reports 1.  src: host bytes;
    src_len includes the tag."""
    buf = _as_u8(src)
    so, sl, info, non, n = _auth_tables(src_off, src_len, infos, nonces)
    ok = np.zeros(n, dtype=np.uint8)
    k = (ctypes.c_uint8 * 32).from_buffer_copy(bytes(prk))
    _check(ctx._L.bw_auth(ctx.h, k, _ptr(buf), so.ctypes.data_as(_lib.u64p), sl.ctypes.data_as(_lib.u64p), n, _ptr(info),
                          info.shape[1] if n else 0, _ptr(non), ok.ctypes.data_as(_lib.u8p)), ctx.h)
    return ok


def auth_device(ctx, prk, d_src, src_off, src_len, infos, nonces):
    """bw_auth_device: d_src is a device pointer (int); tables on the host."""
    so, sl, info, non, n = _auth_tables(src_off, src_len, infos, nonces)
    ok = np.zeros(n, dtype=np.uint8)
    k = (ctypes.c_uint8 * 32).from_buffer_copy(bytes(prk))
    _check(ctx._L.bw_auth_device(ctx.h, k, ctypes.c_void_p(d_src), so.ctypes.data_as(_lib.u64p),
                                 sl.ctypes.data_as(_lib.u64p), n, _ptr(info), info.shape[1] if n else 0, _ptr(non),
                                 ok.ctypes.data_as(_lib.u8p)), ctx.h)
    return ok


def structure(session):
    """bw_check_structure: (entry_flags u8 per entry, item_status u8 per index item, stats STAT_DTYPE per
    packfile, counts dict)."""
    n_items = session.n_items
    flags = np.zeros(max(session.n_entries, 1), dtype=np.uint8)
    ist = np.zeros(max(int(n_items), 1), dtype=np.uint8)
    stats = np.zeros(max(session.n_packfiles, 1), dtype=STAT_DTYPE)
    cnt = _lib.BwCheckCounts()
    _check(session._L.bw_check_structure(session.h, flags.ctypes.data_as(_lib.u8p), ist.ctypes.data_as(_lib.u8p),
                                         stats.ctypes.data_as(ctypes.POINTER(_lib.BwCheckPackfileStat)), ctypes.byref(cnt)),
           session._ctx.h)
    counts = {f: int(getattr(cnt, f)) for f in COUNT_FIELDS}
    return flags[:session.n_entries], ist[:int(n_items)], stats[:session.n_packfiles], counts


def data(session, mode, select=None):
    """bw_check_data: status u8 per entry.  mode "auth" or "full"; select: one byte per entry, None = all."""
    st = np.zeros(max(session.n_entries, 1), dtype=np.uint8)
    sel = None
    if select is not None:
        sel = np.ascontiguousarray(np.asarray(select).astype(bool), dtype=np.uint8)
        assert sel.size == session.n_entries
        sel = np.concatenate([sel, np.zeros(1, np.uint8)])  # never an empty array behind the pointer
    _check(session._L.bw_check_data(session.h, MODES[mode], sel.ctypes.data_as(_lib.u8p) if sel is not None else None,
                                    st.ctypes.data_as(_lib.u8p)), session._ctx.h)
    return st[:session.n_entries]


def check(ctx, packfiles, ids, entries, index_items, prk, roots=None, read_data="auth", packfiles_selected=None, slots=0):
    """The whole check of a store held as lists of bytes (packfiles with their 12-byte ids, entries as
    unpack_headers returned them, index_items n x 44).  Returns a report dict:
      entry_flags, item_status, stats, counts   structure()'s outputs
      data_status                               data()'s statuses (None when read_data is None); with
                                                packfiles_selected only the entries of those packfiles
                                                (positions) are read: "a peer just returned these"
      mark_errors, live, unreachable_blobs, unreachable_bytes
                                                with roots: prune.mark's errors and live bits (verify when
                                                read_data == "full") and what no root reaches
      bad_packfiles                             sorted positions of the packfiles with a flagged entry, a
                                                nonzero tail, a data failure, or an entry whose hash a
                                                mark error names: the list to fetch again from a peer
      ok                                        nothing at all was found"""
    from . import prune
    assert read_data in (None, "auth", "full")
    packfiles = [bytes(b) for b in packfiles]
    items = np.ascontiguousarray(np.asarray(index_items, dtype=np.uint8).reshape(-1, 44))
    en = np.ascontiguousarray(entries, dtype=UNPACK_ENTRY_DTYPE)
    rep = dict(data_status=None, mark_errors=None, live=None, unreachable_blobs=None, unreachable_bytes=None)
    with Session(ctx, prk, packfiles, ids, en, items, slots=slots) as s:
        flags, ist, stats, counts = structure(s)
        rep.update(entry_flags=flags, item_status=ist, stats=stats, counts=counts)
        bad = set(int(p) for p in np.flatnonzero((stats["tail"] != 0)))
        bad |= set(int(p) for p in en["packfile"][flags != 0])
        ok = not bad and not (ist != _lib.BW_RESTORE_OK).any()
        if read_data is not None:
            select = None
            if packfiles_selected is not None:
                select = np.isin(en["packfile"], np.asarray(list(packfiles_selected), dtype=np.int64))
            st = data(s, read_data, select)
            rep["data_status"] = st
            failed = (st != _lib.BW_UNPACK_OK) & (st != _lib.BW_CHECK_SKIPPED)
            bad |= set(int(p) for p in en["packfile"][failed])
            ok = ok and not failed.any()
        if roots is not None:
            live, pstats, pcounts, errs = prune.mark(s, roots, verify=(read_data == "full"))
            rep.update(mark_errors=errs, live=live, unreachable_blobs=pcounts["total_blobs"] - pcounts["live_blobs"],
                       unreachable_bytes=pcounts["total_bytes"] - pcounts["live_bytes"])
            named = {e["hash"].tobytes() for e in errs}
            if named:
                bad |= set(int(x["packfile"]) for x in en if x["hash"].tobytes() in named)
            ok = ok and not len(errs)
    rep["bad_packfiles"] = sorted(bad)
    rep["ok"] = bool(ok)
    return rep
