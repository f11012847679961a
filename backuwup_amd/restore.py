"""Restore: the data path of dir_unpacker.rs:14-130 on the GPU (include/backuwup_gpu_pack.h, "restore").

A Session holds a set of packfiles in device memory, the entries of their headers and the index
items; it finds blobs by hash, walks the trees (fetch_tree, fetch_full_tree, unpack's breadth-first
queue) and assembles files from their chunks (restore_file).  unpack() mirrors dir_unpacker::unpack:
with a destination directory it creates directories, writes files and sets mtimes; without one it
returns the files."""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import check
from .context import PACKFILE_DTYPE, UNPACK_ENTRY_DTYPE, _ptr

NODE_DTYPE = np.dtype([("kind", "<u4"), ("flags", "<u4"), ("size", "<u8"), ("mtime", "<u8"), ("ctime", "<u8"),
                       ("parent", "<u8"), ("child_first", "<u8"), ("n_children", "<u8"), ("name_off", "<u8"),
                       ("name_len", "<u8")])
assert NODE_DTYPE.itemsize == ctypes.sizeof(_lib.BwRestoreNode) == 72
NONE = 2**64 - 1
DEFAULT_WINDOW = 256 << 20

REASONS = {_lib.BW_UNPACK_ETAG: "ETAG", _lib.BW_UNPACK_EZSTD: "EZSTD", _lib.BW_UNPACK_EDIGEST: "EDIGEST",
           _lib.BW_UNPACK_ERANGE: "ERANGE", _lib.BW_RESTORE_ENOTFOUND: "ENOTFOUND",
           _lib.BW_RESTORE_EMISMATCH: "EMISMATCH", _lib.BW_RESTORE_ENOPACKFILE: "ENOPACKFILE",
           _lib.BW_RESTORE_ENOTTREE: "ENOTTREE", _lib.BW_RESTORE_EFORMAT: "EFORMAT"}


class TreeError(_lib.BwError):
    """A tree blob the walk refused: .hash names it, .reason is a BW_RESTORE_* / BW_UNPACK_* code."""

    def __init__(self, rc, msg, blob_hash, reason):
        super().__init__(rc, "%s: %s (%s)" % (msg, bytes(blob_hash).hex(), REASONS.get(reason, reason)))
        self.hash, self.reason = bytes(blob_hash), reason


class Session:
    """bw_restore_open .. bw_restore_close.  packfiles: a device pointer (int) with `plan`, their
    PACKFILE_DTYPE table (offset, size, header_len), or a list of bytes, which the session uploads."""

    def __init__(self, ctx, prk, packfiles, ids, entries, index_items, slots=0, plan=None):
        self._ctx, self._L = ctx, ctx._L
        en = np.ascontiguousarray(entries, dtype=UNPACK_ENTRY_DTYPE)
        items = np.ascontiguousarray(np.asarray(index_items, dtype=np.uint8).reshape(-1, 44))
        idb = np.ascontiguousarray(np.frombuffer(b"".join(bytes(i) for i in ids), dtype=np.uint8)
                                   if not isinstance(ids, np.ndarray) else ids.astype(np.uint8).reshape(-1))
        k = (ctypes.c_uint8 * 32).from_buffer_copy(bytes(prk))
        h = ctypes.c_void_p()
        if plan is not None:
            pl = np.ascontiguousarray(plan, dtype=PACKFILE_DTYPE)
            assert idb.size >= 12 * pl.size
            check(self._L.bw_restore_open(ctx.h, k, ctypes.c_void_p(packfiles),
                                          pl.ctypes.data_as(ctypes.POINTER(_lib.BwPackfile)), _ptr(idb), pl.size,
                                          en.ctypes.data_as(ctypes.POINTER(_lib.BwUnpackEntry)), en.size, _ptr(items),
                                          items.shape[0], slots, ctypes.byref(h)), ctx.h)
        else:
            blobs = [bytes(b) for b in packfiles]
            assert idb.size >= 12 * len(blobs)
            data = np.frombuffer(b"".join(blobs) or b"\0", dtype=np.uint8)
            hl = [int.from_bytes(b[:8], "little") if len(b) >= 8 else 0 for b in blobs]
            tab = ctx._packfile_table([len(b) for b in blobs], hl)
            check(self._L.bw_restore_open_host(ctx.h, k, _ptr(data), tab, _ptr(idb), len(blobs),
                                               en.ctypes.data_as(ctypes.POINTER(_lib.BwUnpackEntry)), en.size,
                                               _ptr(items), items.shape[0], slots, ctypes.byref(h)), ctx.h)
        self.h = h
        self.n_entries, self.n_packfiles = int(en.size), int(pl.size if plan is not None else len(blobs))
        self.n_items = int(items.shape[0])

    def close(self):
        if getattr(self, "h", None):
            self._L.bw_restore_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def locate(self, hashes):
        """(entry_idx u64, status u8) per hash; entry_idx = 2**64 - 1 where status != BW_RESTORE_OK."""
        h = np.ascontiguousarray(np.asarray(hashes, dtype=np.uint8).reshape(-1, 32)) if not isinstance(hashes, list) \
            else np.frombuffer(b"".join(bytes(x) for x in hashes), dtype=np.uint8).reshape(-1, 32)
        idx, st = np.zeros(h.shape[0], dtype=np.uint64), np.zeros(h.shape[0], dtype=np.uint8)
        check(self._L.bw_restore_locate(self.h, _ptr(h), h.shape[0], idx.ctypes.data_as(_lib.u64p),
                                        st.ctypes.data_as(_lib.u8p)), self._ctx.h)
        return idx, st

    def trees(self, root_hash, verify=False):
        """unpack()'s walk from root_hash: (nodes NODE_DTYPE, names bytes, chunks n x 32 u8).  Raises
        TreeError where fetch_full_tree(..)? ends the reference's restore."""
        root = (ctypes.c_uint8 * 32).from_buffer_copy(bytes(root_hash))
        flags = _lib.BW_UNPACK_VERIFY if verify else 0
        cnt, err = _lib.BwRestoreCounts(), _lib.BwRestoreError()
        caps = (1024, 1 << 16, 4096)
        while True:
            nodes = np.zeros(caps[0], dtype=NODE_DTYPE)
            names = np.zeros(caps[1], dtype=np.uint8)
            chunks = np.zeros((caps[2], 32), dtype=np.uint8)
            rc = self._L.bw_restore_trees(self.h, root, flags, nodes.ctypes.data_as(ctypes.POINTER(_lib.BwRestoreNode)),
                                          caps[0], _ptr(names), caps[1], _ptr(chunks), caps[2], ctypes.byref(cnt),
                                          ctypes.byref(err))
            if rc == _lib.BW_EFORMAT:
                raise TreeError(rc, "tree blob refused", bytes(err.hash), err.reason)
            if rc != _lib.BW_ENOSPC:
                check(rc, self._ctx.h)
                return nodes[:cnt.n_nodes], names[:cnt.name_bytes].tobytes(), chunks[:cnt.n_chunks]
            caps = (max(cnt.n_nodes, 1), max(cnt.name_bytes, 1), max(cnt.n_chunks, 1))

    def _files_args(self, chunks, file_first, flags):
        rows = np.ascontiguousarray(np.asarray(chunks, dtype=np.uint8).reshape(-1, 32))
        ff = np.ascontiguousarray(file_first, dtype=np.uint64)
        n = ff.size - 1
        off, ln, bad = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(3))
        st, done = np.zeros(max(n, 1), dtype=np.uint8), ctypes.c_uint64()
        return rows, ff, n, off, ln, st, bad, done

    def files_device(self, chunks, file_first, d_dst, dst_cap, flags=0):
        """bw_restore_files_device: (rc, n_done, file_off, file_len, file_status, file_bad_child); rc is
        BW_OK or BW_ENOSPC (the window is full: drain n_done files and call again with the rest)."""
        rows, ff, n, off, ln, st, bad, done = self._files_args(chunks, file_first, flags)
        rc = self._L.bw_restore_files_device(self.h, _ptr(rows), ff.ctypes.data_as(_lib.u64p), n, flags,
                                             ctypes.c_void_p(d_dst), dst_cap, off.ctypes.data_as(_lib.u64p),
                                             ln.ctypes.data_as(_lib.u64p), st.ctypes.data_as(_lib.u8p),
                                             bad.ctypes.data_as(_lib.u64p), ctypes.byref(done))
        if rc != _lib.BW_ENOSPC:
            check(rc, self._ctx.h)
        return rc, done.value, off[:n], ln[:n], st[:n], bad[:n]

    def files(self, chunks, file_first, window=DEFAULT_WINDOW, flags=0):
        """bw_restore_files until every file is back: ([bytes], status, bad_child).  A failed file's
        bytes are the partial file the reference leaves behind."""
        rows = np.ascontiguousarray(np.asarray(chunks, dtype=np.uint8).reshape(-1, 32))
        ff = np.ascontiguousarray(file_first, dtype=np.uint64)
        n_all = ff.size - 1
        out, status, bad_child = [], np.zeros(n_all, dtype=np.uint8), np.zeros(n_all, dtype=np.uint64)
        buf = np.empty(max(int(window), 1), dtype=np.uint8)
        at = 0
        while at < n_all:
            _, sub, n, off, ln, st, bad, done = self._files_args(rows, ff[at:], flags)
            rc = self._L.bw_restore_files(self.h, _ptr(rows), sub.ctypes.data_as(_lib.u64p), n, flags, _ptr(buf), buf.size,
                                          off.ctypes.data_as(_lib.u64p), ln.ctypes.data_as(_lib.u64p),
                                          st.ctypes.data_as(_lib.u8p), bad.ctypes.data_as(_lib.u64p), ctypes.byref(done))
            if rc != _lib.BW_ENOSPC:
                check(rc, self._ctx.h)
            k = done.value
            out += [buf[int(off[i]):int(off[i] + ln[i])].tobytes() for i in range(k)]
            status[at:at + k], bad_child[at:at + k] = st[:k], bad[:k]
            at += k
            if rc == _lib.BW_ENOSPC and not k:  # one file larger than the window
                buf = np.empty(max(2 * buf.size, int(ln[0])), dtype=np.uint8)
        return out, status, bad_child


def walk_paths(nodes, names):
    """Relative path per node ('' for the root), as unpack() joins them (path.join(child.name))."""
    paths = [""] * len(nodes)
    for i in range(1, len(nodes)):
        nd = nodes[i]
        name = names[int(nd["name_off"]):int(nd["name_off"] + nd["name_len"])].decode("utf-8")
        paths[i] = os.path.join(paths[int(nd["parent"])], name)
    return paths


def unpack(ctx, packfiles, ids, entries, index_items, prk, root_hash, destination_dir=None, window=DEFAULT_WINDOW,
           verify=False, slots=0, plan=None):
    """dir_unpacker::unpack(packfile_dir, destination_dir, root_hash).  Without destination_dir:
    ({relative path: bytes}, errors); with it the directories are created (mtimes set), the files
    written and their mtimes set, and (None, errors) returned.  errors = [(path, status, bad child)]
    for the files the reference prints "error restoring file" for; their partial bytes are kept, as
    it keeps them.  A root of kind File restores nothing (dir_unpacker.rs:66-67)."""
    with Session(ctx, prk, packfiles, ids, entries, index_items, slots=slots, plan=plan) as s:
        nodes, names, chunks = s.trees(root_hash, verify=verify)
        if destination_dir is not None:
            os.makedirs(destination_dir, exist_ok=True)
        result, errors = ({} if destination_dir is None else None), []
        if nodes[0]["kind"] != _lib.BW_TREE_DIR:
            return result, errors
        paths = walk_paths(nodes, names)
        file_nodes = [i for i in range(1, len(nodes)) if nodes[i]["kind"] == _lib.BW_TREE_FILE]
        if destination_dir is not None:
            for i in range(1, len(nodes)):
                if nodes[i]["kind"] == _lib.BW_TREE_DIR:
                    p = os.path.join(destination_dir, paths[i])
                    os.makedirs(p, exist_ok=True)
                    _set_mtime(p, nodes[i])
        counts = np.array([int(nodes[i]["n_children"]) for i in file_nodes], dtype=np.uint64)
        ff = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        rows = np.concatenate([chunks[int(nodes[i]["child_first"]):int(nodes[i]["child_first"] + nodes[i]["n_children"])]
                               for i in file_nodes] + [np.zeros((0, 32), dtype=np.uint8)])
        data, status, bad = s.files(rows, ff, window=window, flags=_lib.BW_UNPACK_VERIFY if verify else 0)
        for k, i in enumerate(file_nodes):
            if status[k]:
                errors.append((paths[i], int(status[k]), int(bad[k])))
            if destination_dir is None:
                result[paths[i]] = data[k]
                continue
            p = os.path.join(destination_dir, paths[i])
            with open(p, "wb") as fh:
                fh.write(data[k])
            if not status[k]:  # restore_file bails before set_path_mtime
                _set_mtime(p, nodes[i])
        return result, errors


def _set_mtime(path, node):
    if node["flags"] & _lib.BW_TREE_HAS_MTIME:  # set_path_mtime: FileTime::from_unix_time(mtime as i64, 0)
        st = os.stat(path)
        os.utime(path, (st.st_atime, int(node["mtime"])))
