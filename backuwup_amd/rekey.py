"""Rekey: a store under a new backup secret (include/backuwup_gpu_pack.h, "reseal" and "rekey").  The
reference cannot change its secret.

reseal() / reseal_device() turn items sealed under one PRK into the same plaintexts sealed under
another in one pass over the ciphertext (c ^ keystream_old ^ keystream_new: no plaintext is stored);
rekey_store() does that to every header and blob of an open restore Session; rekey() is the whole
sequence over a store held as lists of bytes, index files included."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check as _check
from .context import UNPACK_ENTRY_DTYPE, _as_u8, _ptr
from .restore import Session


def _tables(src_off, src_len, infos, nonces, new_nonces, dst_off):
    so = np.ascontiguousarray(src_off, dtype=np.uint64)
    sl = np.ascontiguousarray(src_len, dtype=np.uint64)
    do = np.ascontiguousarray(dst_off, dtype=np.uint64)
    n = len(so)
    assert len(sl) == n and len(do) == n

    def rows(a, w):
        return np.ascontiguousarray(np.asarray(a, dtype=np.uint8).reshape(n, w)) if n else np.zeros((0, max(w, 0)), np.uint8)
    info = rows(infos, -1)
    return so, sl, info, rows(nonces, 12), (None if new_nonces is None else rows(new_nonces, 12)), do, n


def _prk(prk):
    return (ctypes.c_uint8 * 32).from_buffer_copy(bytes(prk))


def reseal(ctx, old_prk, new_prk, src, src_off, src_len, infos, nonces, dst_off, dst_size, new_nonces=None, out=None):
    """bw_reseal over host buffers: (out, ok).  src_len includes the tag; output i is src_len[i] bytes at
    out[dst_off[i]:]; ok[i] = 1 where item i was authentic under old_prk (else its new tag is the
    complement of the valid one).  new_nonces None: the nonces are kept.  out: a caller's uint8 array of
    at least dst_size bytes (only the output ranges are written); default a new zeroed buffer."""
    buf = _as_u8(src)
    so, sl, info, non, nn, do, n = _tables(src_off, src_len, infos, nonces, new_nonces, dst_off)
    if out is None:
        out = np.zeros(max(int(dst_size), 1), dtype=np.uint8)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.ndim == 1 and out.flags.c_contiguous and \
        out.flags.writeable and out.size >= max(int(dst_size), 1)
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    _check(ctx._L.bw_reseal(ctx.h, _prk(old_prk), _prk(new_prk), _ptr(buf), so.ctypes.data_as(_lib.u64p),
                            sl.ctypes.data_as(_lib.u64p), n, _ptr(info), info.shape[1] if n else 0, _ptr(non),
                            _ptr(nn) if nn is not None else None, _ptr(out), do.ctypes.data_as(_lib.u64p),
                            ok.ctypes.data_as(_lib.u8p)), ctx.h)
    return out[:int(dst_size)], ok[:n]


def reseal_device(ctx, old_prk, new_prk, d_src, src_off, src_len, infos, nonces, d_dst, dst_off, new_nonces=None):
    """bw_reseal_device: d_src and d_dst are device pointers (ints), tables on the host.  Returns ok."""
    so, sl, info, non, nn, do, n = _tables(src_off, src_len, infos, nonces, new_nonces, dst_off)
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    _check(ctx._L.bw_reseal_device(ctx.h, _prk(old_prk), _prk(new_prk), ctypes.c_void_p(d_src), so.ctypes.data_as(_lib.u64p),
                                   sl.ctypes.data_as(_lib.u64p), n, _ptr(info), info.shape[1] if n else 0, _ptr(non),
                                   _ptr(nn) if nn is not None else None, ctypes.c_void_p(d_dst),
                                   do.ctypes.data_as(_lib.u64p), ok.ctypes.data_as(_lib.u8p)), ctx.h)
    return ok[:n]


def rekey_store(session, new_prk, out=None, d_out=None):
    """bw_rekey_store (into `out`, a host uint8 array of the packfile table's extent) or, with d_out (a
    device pointer, int), bw_rekey_store_device: (entry_status u8 per entry, packfile_status u8 per
    packfile).  The output has the session's packfile table."""
    est = np.zeros(max(session.n_entries, 1), dtype=np.uint8)
    pst = np.zeros(max(session.n_packfiles, 1), dtype=np.uint8)
    args = (est.ctypes.data_as(_lib.u8p), pst.ctypes.data_as(_lib.u8p))
    if d_out is not None:
        _check(session._L.bw_rekey_store_device(session.h, _prk(new_prk), ctypes.c_void_p(d_out), *args), session._ctx.h)
    else:
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable
        _check(session._L.bw_rekey_store(session.h, _prk(new_prk), _ptr(out), *args), session._ctx.h)
    return est[:session.n_entries], pst[:session.n_packfiles]


def rekey(ctx, packfiles, ids, entries, index_items, index_files, old_prk, new_prk):
    """The whole change of secret for a store held as lists of bytes (packfiles with their 12-byte ids,
    entries as unpack_headers returned them, index_items n x 44, index_files [(file_num, bytes)]).
    Returns (new packfiles [bytes], new index files [(file_num, bytes)], bad entries, bad packfiles):
    the positions of the entries and of the packfile headers that did not authenticate under old_prk
    (entries outside their blob section included).  Their outputs are not authentic under new_prk
    either.  The index files are loaded under old_prk and built again under new_prk with their numbers
    kept; index_items only feeds the session."""
    packfiles = [bytes(b) for b in packfiles]
    en = np.ascontiguousarray(entries, dtype=UNPACK_ENTRY_DTYPE)
    sizes = [len(b) for b in packfiles]
    out = np.zeros(max(sum(sizes), 1), dtype=np.uint8)
    with Session(ctx, old_prk, packfiles, ids, en, index_items) as s:
        est, pst = rekey_store(s, new_prk, out=out)
    new_packs, at = [], 0
    for n in sizes:
        new_packs.append(out[at:at + n].tobytes())
        at += n
    index_files = list(index_files)
    new_index = []
    if index_files:
        items = ctx.index_load_files(old_prk, index_files)
        first = min(int(num) for num, _ in index_files)
        new_index = ctx.index_files_build(new_prk, items, last_file_num=first - 1 if first > 0 else 0)
    bad_entries = [int(e) for e in np.flatnonzero(est != _lib.BW_UNPACK_OK)]
    bad_packfiles = [int(p) for p in np.flatnonzero(pst != _lib.BW_UNPACK_OK)]
    return new_packs, new_index, bad_entries, bad_packfiles
