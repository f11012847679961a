"""Parity: Reed-Solomon shards over packfiles, and repair from them (include/backuwup_gpu_pack.h,
"parity").  The reference has no redundancy.

matmul() / matmul_device() are the GF(2^8) primitive (k_gf_matmul); plan() groups a packfile table;
build() / build_device() write every parity shard and return every shard's BLAKE3; solve() is the host
Gauss-Jordan; repair() / repair_device() rebuild one group's missing or damaged shards.  protect() and
repair_store() are the whole sequence over a store held as lists of bytes: check.check()'s bad_packfiles
says which packfiles are bad, repair_store() makes them good again without a peer."""
import ctypes
import os
import struct

import numpy as np

from . import _lib
from ._lib import check as _check
from .context import PACKFILE_DTYPE, _as_u8, _ptr

GROUP_DTYPE = np.dtype([("first_packfile", "<u8"), ("k", "<u4"), ("m", "<u4"), ("shard_len", "<u8"), ("out_offset", "<u8")])
assert GROUP_DTYPE.itemsize == ctypes.sizeof(_lib.BwParityGroup) == 32
STATUS_NAMES = {_lib.BW_PARITY_OK: "ok", _lib.BW_PARITY_DAMAGED: "damaged", _lib.BW_PARITY_REBUILT: "rebuilt",
                _lib.BW_PARITY_REBUILT_BAD: "rebuilt_bad", _lib.BW_PARITY_LOST: "lost"}
MANIFEST_VERSION = 1
MANIFEST_INFO_TEXT = b"backuwup parity manifest v1"

_u32p = ctypes.POINTER(ctypes.c_uint32)
_grp = ctypes.POINTER(_lib.BwParityGroup)
_pfp = ctypes.POINTER(_lib.BwPackfile)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _matrix(matrix):
    m = np.ascontiguousarray(matrix, dtype=np.uint8)
    assert m.ndim == 2
    return m


def matmul(ctx, matrix, src, src_off, src_len, dst_off, length, dst_size=None, out=None):
    """bw_gf_matmul over host buffers: row r of the result is out[dst_off[r]:dst_off[r] + length]."""
    m = _matrix(matrix)
    buf = _as_u8(src)
    so, sl, do = _u64(src_off), _u64(src_len), _u64(dst_off)
    assert len(so) == len(sl) == m.shape[1] and len(do) == m.shape[0]
    if dst_size is None:
        dst_size = int(do.max()) + int(length) if len(do) else 0
    if out is None:
        out = np.zeros(max(int(dst_size), 1), dtype=np.uint8)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= max(int(dst_size), 1)
    _check(ctx._L.bw_gf_matmul(ctx.h, _ptr(m), m.shape[0], m.shape[1], _ptr(buf), so.ctypes.data_as(_lib.u64p),
                               sl.ctypes.data_as(_lib.u64p), _ptr(out), do.ctypes.data_as(_lib.u64p), int(length)), ctx.h)
    return out[:int(dst_size)]


def matmul_device(ctx, matrix, d_src, src_off, src_len, d_dst, dst_off, length):
    """bw_gf_matmul_device: d_src and d_dst are device pointers (ints), matrix and tables on the host."""
    m = _matrix(matrix)
    so, sl, do = _u64(src_off), _u64(src_len), _u64(dst_off)
    assert len(so) == len(sl) == m.shape[1] and len(do) == m.shape[0]
    _check(ctx._L.bw_gf_matmul_device(ctx.h, _ptr(m), m.shape[0], m.shape[1], ctypes.c_void_p(d_src),
                                      so.ctypes.data_as(_lib.u64p), sl.ctypes.data_as(_lib.u64p), ctypes.c_void_p(d_dst),
                                      do.ctypes.data_as(_lib.u64p), int(length)), ctx.h)


def plan(sizes, k, m):
    """bw_parity_plan (host only): (groups GROUP_DTYPE, out_bytes)."""
    L = _lib.load()
    sz = _u64(sizes)
    ng, total = ctypes.c_uint64(), ctypes.c_uint64()
    cap = (len(sz) + max(int(k), 1) - 1) // max(int(k), 1)
    groups = np.zeros(max(cap, 1), dtype=GROUP_DTYPE)
    _check(L.bw_parity_plan(sz.ctypes.data_as(_lib.u64p) if len(sz) else None, len(sz), int(k), int(m),
                            groups.ctypes.data_as(_grp), cap, ctypes.byref(ng), ctypes.byref(total)))
    return groups[:ng.value], int(total.value)


def _table(sizes):
    tab = np.zeros(len(sizes), dtype=PACKFILE_DTYPE)
    tab["size"] = sizes
    tab["offset"] = np.concatenate([[0], np.cumsum(sizes)[:-1]]) if len(sizes) else []
    return tab


def _n_shards(groups):
    return int(groups["k"].astype(np.int64).sum() + groups["m"].astype(np.int64).sum())


def build(ctx, data, packfiles, groups, out_bytes):
    """bw_parity_build over host buffers: data holds the packfile table's extent (packfiles: PACKFILE_DTYPE,
    offset and size used).  Returns (parity buffer uint8[out_bytes], digests n_shards x 32: per group the
    data shards' then the parity shards')."""
    buf = _as_u8(data)
    tab = np.ascontiguousarray(packfiles, dtype=PACKFILE_DTYPE)
    gr = np.ascontiguousarray(groups, dtype=GROUP_DTYPE)
    out = np.zeros(max(int(out_bytes), 1), dtype=np.uint8)
    dig = np.zeros((max(_n_shards(gr), 1), 32), dtype=np.uint8)
    _check(ctx._L.bw_parity_build(ctx.h, _ptr(buf), tab.ctypes.data_as(_pfp), len(tab), gr.ctypes.data_as(_grp), len(gr),
                                  _ptr(out), int(out_bytes), dig.ctypes.data_as(_lib.u8p)), ctx.h)
    return out[:int(out_bytes)], dig[:_n_shards(gr)]


def build_device(ctx, d_packfiles, packfiles, groups, d_out, out_bytes):
    """bw_parity_build_device: device pointers (ints); returns the digests."""
    tab = np.ascontiguousarray(packfiles, dtype=PACKFILE_DTYPE)
    gr = np.ascontiguousarray(groups, dtype=GROUP_DTYPE)
    dig = np.zeros((max(_n_shards(gr), 1), 32), dtype=np.uint8)
    _check(ctx._L.bw_parity_build_device(ctx.h, ctypes.c_void_p(d_packfiles), tab.ctypes.data_as(_pfp), len(tab),
                                         gr.ctypes.data_as(_grp), len(gr), ctypes.c_void_p(d_out), int(out_bytes),
                                         dig.ctypes.data_as(_lib.u8p)), ctx.h)
    return dig[:_n_shards(gr)]


def solve(k, m, present):
    """bw_parity_solve (host only): (used [k], missing, matrix len(missing) x k).  Fewer than k present
    raises BwError with rc BW_ETOOFEW."""
    L = _lib.load()
    pr = np.ascontiguousarray(np.asarray(present).astype(bool), dtype=np.uint8)
    assert len(pr) == k + m
    used = np.zeros(max(k, 1), dtype=np.uint32)
    missing = np.zeros(k + m, dtype=np.uint32)
    nm = ctypes.c_uint32()
    matrix = np.zeros((k + m) * max(k, 1), dtype=np.uint8)
    _check(L.bw_parity_solve(int(k), int(m), pr.ctypes.data_as(_lib.u8p), used.ctypes.data_as(_u32p),
                             missing.ctypes.data_as(_u32p), ctypes.byref(nm), matrix.ctypes.data_as(_lib.u8p)))
    n = nm.value
    return used[:k].tolist(), missing[:n].tolist(), matrix[:n * k].reshape(n, k).copy()


def _group(group):
    g = np.ascontiguousarray(group, dtype=GROUP_DTYPE).reshape(1)
    return g, int(g["k"][0]) + int(g["m"][0])


def _repair_args(group, present, shard_off, shard_size, digests, out_off):
    g, n = _group(group)
    pr = np.ascontiguousarray(np.asarray(present).astype(bool), dtype=np.uint8)
    so, ss, oo = _u64(shard_off), _u64(shard_size), _u64(out_off)
    assert len(pr) == len(so) == len(ss) == len(oo) == n
    dg = None
    if digests is not None:
        dg = np.ascontiguousarray(np.asarray(digests, dtype=np.uint8).reshape(n, 32))
    st = np.zeros(n, dtype=np.uint8)
    return g, pr, so, ss, dg, oo, st


def repair(ctx, group, present, shards, shard_off, shard_size, out_off, out_size, digests=None, out=None):
    """bw_parity_repair over host buffers: (out, status u8 per shard).  A rebuilt shard s is
    out[out_off[s]:out_off[s] + shard_len]; the caller keeps shard_size[s] bytes of it."""
    g, pr, so, ss, dg, oo, st = _repair_args(group, present, shard_off, shard_size, digests, out_off)
    buf = _as_u8(shards)
    if out is None:
        out = np.zeros(max(int(out_size), 1), dtype=np.uint8)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= max(int(out_size), 1)
    _check(ctx._L.bw_parity_repair(ctx.h, g.ctypes.data_as(_grp), pr.ctypes.data_as(_lib.u8p), _ptr(buf),
                                   so.ctypes.data_as(_lib.u64p), ss.ctypes.data_as(_lib.u64p),
                                   dg.ctypes.data_as(_lib.u8p) if dg is not None else None, _ptr(out),
                                   oo.ctypes.data_as(_lib.u64p), st.ctypes.data_as(_lib.u8p)), ctx.h)
    return out[:int(out_size)], st


def repair_device(ctx, group, present, d_shards, shard_off, shard_size, d_out, out_off, digests=None):
    """bw_parity_repair_device: device pointers (ints); returns the statuses."""
    g, pr, so, ss, dg, oo, st = _repair_args(group, present, shard_off, shard_size, digests, out_off)
    _check(ctx._L.bw_parity_repair_device(ctx.h, g.ctypes.data_as(_grp), pr.ctypes.data_as(_lib.u8p), ctypes.c_void_p(d_shards),
                                          so.ctypes.data_as(_lib.u64p), ss.ctypes.data_as(_lib.u64p),
                                          dg.ctypes.data_as(_lib.u8p) if dg is not None else None, ctypes.c_void_p(d_out),
                                          oo.ctypes.data_as(_lib.u64p), st.ctypes.data_as(_lib.u8p)), ctx.h)
    return st


# ---- the manifest: one sealed item under prk; plaintext little-endian: u32 version = 1, u32 n_groups, per
# group u32 k, u32 m, u64 shard_len, k x {id[12], u32 0, u64 size, digest[32]}, m x digest[32]
def manifest_info(ctx):
    """The HKDF info of the manifest's key: the 32-byte BLAKE3 of MANIFEST_INFO_TEXT."""
    return bytes(ctx.blake3(MANIFEST_INFO_TEXT))


def manifest_encode(groups):
    out = [struct.pack("<II", MANIFEST_VERSION, len(groups))]
    for g in groups:
        out.append(struct.pack("<IIQ", g["k"], g["m"], g["shard_len"]))
        for i, n, d in zip(g["ids"], g["sizes"], g["data_digests"]):
            out.append(bytes(i) + struct.pack("<IQ", 0, int(n)) + bytes(d))
        out += [bytes(d) for d in g["parity_digests"]]
    return b"".join(out)


def manifest_decode(buf):
    buf = bytes(buf)
    if len(buf) < 8:
        raise ValueError("parity manifest: too short")
    version, n = struct.unpack_from("<II", buf, 0)
    if version != MANIFEST_VERSION:
        raise ValueError("parity manifest version %d" % version)
    at, groups = 8, []
    for _ in range(n):
        if at + 16 > len(buf):
            raise ValueError("parity manifest: truncated")
        k, m, length = struct.unpack_from("<IIQ", buf, at)
        at += 16
        if not k or not m or k + m > 256 or at + 56 * k + 32 * m > len(buf):
            raise ValueError("parity manifest: a group that cannot be")
        g = dict(k=k, m=m, shard_len=length, ids=[], sizes=[], data_digests=[], parity_digests=[])
        for _ in range(k):
            pad, size = struct.unpack_from("<IQ", buf, at + 12)
            if pad:
                raise ValueError("parity manifest: nonzero padding")
            g["ids"].append(buf[at:at + 12])
            g["sizes"].append(size)
            g["data_digests"].append(buf[at + 24:at + 56])
            at += 56
        for _ in range(m):
            g["parity_digests"].append(buf[at:at + 32])
            at += 32
        groups.append(g)
    if at != len(buf):
        raise ValueError("parity manifest: trailing bytes")
    return groups


def seal_manifest(ctx, prk, plaintext, nonce=None):
    """nonce (12 bytes, random unless given) || the plaintext sealed under prk with manifest_info()."""
    nonce = os.urandom(12) if nonce is None else bytes(nonce)
    assert len(nonce) == 12
    n = len(plaintext)
    sealed = ctx.seal(prk, plaintext, [0], [n], np.frombuffer(manifest_info(ctx), np.uint8), np.frombuffer(nonce, np.uint8), [0],
                      n + 16)
    return nonce + sealed.tobytes()


def open_manifest(ctx, prk, manifest):
    """The groups of a sealed manifest; raises ValueError where its tag fails: it is never half-used."""
    manifest = bytes(manifest)
    if len(manifest) < 28:
        raise ValueError("parity manifest: too short")
    n = len(manifest) - 12
    pt, ok = ctx.seal(prk, manifest[12:], [0], [n], np.frombuffer(manifest_info(ctx), np.uint8),
                      np.frombuffer(manifest[:12], np.uint8), [0], n - 16, open_=True)
    if not ok[0]:
        raise ValueError("parity manifest: authentication failed")
    return manifest_decode(pt.tobytes())


def protect(ctx, packfiles, ids, prk, k=8, m=2, nonce=None):
    """Parity for a store held as a list of packfile bytes with their 12-byte ids: (parity shards [bytes],
    group by group, m per group; the sealed manifest)."""
    packfiles = [bytes(b) for b in packfiles]
    if not isinstance(ids, np.ndarray):
        ids = np.frombuffer(b"".join(bytes(i) for i in ids), dtype=np.uint8)
    ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(len(packfiles), 12)
    sizes = [len(b) for b in packfiles]
    groups, out_bytes = plan(sizes, k, m)
    out, dig = build(ctx, b"".join(packfiles), _table(sizes), groups, out_bytes)
    shards, man, at = [], [], 0
    for g in groups:
        first, kk, mm, length, off = int(g["first_packfile"]), int(g["k"]), int(g["m"]), int(g["shard_len"]), int(g["out_offset"])
        shards += [out[off + i * length:off + (i + 1) * length].tobytes() for i in range(mm)]
        man.append(dict(k=kk, m=mm, shard_len=length, ids=[ids[first + j].tobytes() for j in range(kk)],
                        sizes=sizes[first:first + kk], data_digests=[dig[at + j].tobytes() for j in range(kk)],
                        parity_digests=[dig[at + kk + i].tobytes() for i in range(mm)]))
        at += kk + mm
    return shards, seal_manifest(ctx, prk, manifest_encode(man), nonce)


def repair_store(ctx, packfiles, parity_shards, manifest, prk):
    """Entries of packfiles and parity_shards may be None ("not available"); a packfile that
    check.check()'s bad_packfiles names may be passed as it is: its digest demotes it.  Returns
    (packfiles [bytes or None], parity_shards [bytes or None], report): every shard that could be rebuilt
    is in place, the others are as they came.  report = dict(status: per group the list of per-shard
    status names, data shards then parity; lost_groups: positions of the groups with a lost shard;
    rebuilt_packfiles, rebuilt_parity: positions put back; ok: nothing is lost or rebuilt bad)."""
    groups = open_manifest(ctx, prk, manifest)
    packfiles, parity_shards = list(packfiles), list(parity_shards)
    assert len(packfiles) == sum(g["k"] for g in groups) and len(parity_shards) == sum(g["m"] for g in groups)
    report = dict(status=[], lost_groups=[], rebuilt_packfiles=[], rebuilt_parity=[], ok=True)
    first = pfirst = 0
    for gi, g in enumerate(groups):
        k, m, length = g["k"], g["m"], g["shard_len"]
        have = packfiles[first:first + k] + parity_shards[pfirst:pfirst + m]
        size = list(g["sizes"]) + [length] * m
        # a shard of another size than the manifest's cannot be the shard: not available
        present = [b is not None and len(b) == size[s] for s, b in enumerate(have)]
        off, at = [], 0
        for s in range(k + m):
            off.append(at)
            at += len(have[s]) if present[s] else 0
        out_off = [s * length for s in range(k + m)]
        out, st = repair(ctx, np.array([(first, k, m, length, 0)], dtype=GROUP_DTYPE), present,
                         b"".join(bytes(b) for s, b in enumerate(have) if present[s]), off, size, out_off, (k + m) * length,
                         digests=np.frombuffer(b"".join(g["data_digests"] + g["parity_digests"]), np.uint8))
        report["status"].append([STATUS_NAMES[int(x)] for x in st])
        if (st == _lib.BW_PARITY_LOST).any():
            report["lost_groups"].append(gi)
        for s in range(k + m):
            if st[s] in (_lib.BW_PARITY_REBUILT, _lib.BW_PARITY_DAMAGED):
                b = out[out_off[s]:out_off[s] + size[s]].tobytes()
                if s < k:
                    packfiles[first + s] = b
                    report["rebuilt_packfiles"].append(first + s)
                else:
                    parity_shards[pfirst + s - k] = b
                    report["rebuilt_parity"].append(pfirst + s - k)
            elif st[s] in (_lib.BW_PARITY_REBUILT_BAD, _lib.BW_PARITY_LOST):
                report["ok"] = False
        first += k
        pfirst += m
    return packfiles, parity_shards, report
