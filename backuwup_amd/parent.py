"""Parent match: which files a new backup need not read (include/backuwup_gpu_pack.h, "parent match").

The reference maps and chunks every file on every run (dir_packer.rs:231-282) and lets dedup discard the
result; this goes past it.  A Tree blob holds its own name, kind and metadata and names its children by
hash (filesystem/mod.rs:63-77), so a File whose name, size, mtime and ctime are those of the parent
snapshot's File of that path keeps the parent's tree blob: its hash goes into the new directory tree as
it stands, no file byte is read and no tree blob is rebuilt.  That the chunk list is equal when
everything else is equal is the heuristic restic's parent snapshot, borg's files cache and git's index
all rest on; trust_before (the parent snapshot's start time) takes the files out of it whose whole-second
mtime cannot tell a later write from the one the parent saw.

match() is bw_parent_match over an open restore Session; scan_directory() is the stat-only walk that
feeds it; snapshot() is the whole sequence up to the new root hash."""
import ctypes
import os

import numpy as np

from . import _lib, packer
from ._lib import check
from .prune import ERROR_DTYPE
from .restore import NODE_DTYPE

NEW, UNCHANGED, CHANGED, RACY, DIR, TYPE_CHANGED = range(6)
STATUSES = {NEW: "new", UNCHANGED: "unchanged", CHANGED: "changed", RACY: "racy", DIR: "dir", TYPE_CHANGED: "type_changed"}
NONE = 2**64 - 1
RESULT_DTYPE = np.dtype([("hash", "u1", (32,)), ("status", "<u4"), ("pad", "<u4")])
assert RESULT_DTYPE.itemsize == ctypes.sizeof(_lib.BwParentResult) == 40
COUNT_FIELDS = [f for f, _ in _lib.BwParentCounts._fields_]


def match(session, parent_root, nodes, names, trust_before=NONE, verify=False):
    """bw_parent_match over an open restore Session: (results RESULT_DTYPE per scan node, read u8 per
    entry, counts dict, errors prune.ERROR_DTYPE).  nodes (restore.NODE_DTYPE) and names are the scan, in
    the layout of Session.trees' listing with every File's n_children zero; parent_root may be None: no
    parent, everything is NEW.  An invalid scan raises BwError (BW_EINVAL).  The error buffer grows
    until the walk's errors fit it."""
    sc = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    nm = np.frombuffer(bytes(names), dtype=np.uint8) if not isinstance(names, np.ndarray) else np.ascontiguousarray(names, dtype=np.uint8)
    root = None if parent_root is None else (ctypes.c_uint8 * 32).from_buffer_copy(bytes(parent_root))
    results = np.zeros(max(sc.size, 1), dtype=RESULT_DTYPE)
    read = np.zeros(max(session.n_entries, 1), dtype=np.uint8)
    cnt = _lib.BwParentCounts()
    cap = 64
    while True:
        errs = np.zeros(cap, dtype=ERROR_DTYPE)
        rc = session._L.bw_parent_match(session.h, root, trust_before, _lib.BW_UNPACK_VERIFY if verify else 0,
                                        sc.ctypes.data_as(ctypes.POINTER(_lib.BwRestoreNode)), sc.size,
                                        ctypes.c_void_p(nm.ctypes.data) if nm.size else None, nm.size,
                                        results.ctypes.data_as(ctypes.POINTER(_lib.BwParentResult)),
                                        read.ctypes.data_as(_lib.u8p), ctypes.byref(cnt),
                                        errs.ctypes.data_as(ctypes.POINTER(_lib.BwPruneError)), cap)
        if rc != _lib.BW_ENOSPC:
            check(rc, session._ctx.h)
            break
        cap = max(2 * cap, int(cnt.n_errors))
    counts = {f: int(getattr(cnt, f)) for f in COUNT_FIELDS}
    return results[:sc.size], read[:session.n_entries], counts, errs[:counts["n_errors"]]


def scan_directory(path):
    """The stat-only walk of a directory: (nodes restore.NODE_DTYPE, names bytes), node 0 the root, a
    Dir's children consecutive, Dirs taken in node order (the order of a Session.trees listing).  Only
    os.scandir and stat are used, no file is opened.  As the reference's walk does (dir_packer.rs:160-198)
    regular files and directories are taken and everything else is left out, symlinks included; the
    metadata is get_metadata's (dir_packer.rs:393-410): size = st_size for Files and Dirs alike, mtime in
    whole seconds, ctime = the creation time where the platform's stat has one (st_birthtime), each absent
    when negative or unknown.  The root's name is the path's last component.  An entry that cannot be
    stat'ed is left out, as the reference logs it and carries on."""
    def meta(st):
        out = [int(st.st_size), 0, 0, _lib.BW_TREE_HAS_SIZE]
        for k, t in ((1, st.st_mtime), (2, getattr(st, "st_birthtime", None))):
            if t is not None and int(t // 1) >= 0:
                out[k] = int(t // 1)
                out[3] |= _lib.BW_TREE_HAS_MTIME if k == 1 else _lib.BW_TREE_HAS_CTIME
        return out

    path = os.fspath(path)
    rows = [(_lib.BW_TREE_DIR, os.fsencode(os.path.basename(os.path.normpath(path))), meta(os.stat(path)), NONE, path)]
    i = 0
    while i < len(rows):
        kind, _, _, _, p = rows[i]
        if kind == _lib.BW_TREE_DIR:
            first = len(rows)
            try:
                entries = sorted(os.scandir(p), key=lambda e: os.fsencode(e.name))
            except OSError:
                entries = []
            for e in entries:
                try:
                    if e.is_file(follow_symlinks=False):
                        k = _lib.BW_TREE_FILE
                    elif e.is_dir(follow_symlinks=False):
                        k = _lib.BW_TREE_DIR
                    else:
                        continue
                    rows.append((k, os.fsencode(e.name), meta(e.stat(follow_symlinks=False)), i, e.path))
                except OSError:
                    continue
            rows[i] = rows[i] + (first, len(rows) - first)
        else:
            rows[i] = rows[i] + (0, 0)
        i += 1
    nodes = np.zeros(len(rows), dtype=NODE_DTYPE)
    names = bytearray()
    for i, (kind, name, (size, mtime, ctime, flags), parent, _, first, count) in enumerate(rows):
        nodes[i] = (kind, flags, size, mtime, ctime, parent, first, count, len(names), len(name))
        names += name
    return nodes, bytes(names)


def _opt(node, field, bit):
    return int(node[field]) if int(node["flags"]) & bit else None


def snapshot(ctx, session, parent_root, nodes, names, read_file, trust_before=NONE, verify=False, dedup=True, **chunking):
    """A backup of the scan against the parent snapshot parent_root (None: a full backup), up to the new
    root hash: match(); read_file(node_index) -> bytes for exactly the File nodes that are not UNCHANGED;
    their chunks and hashes through packer.process_files (one batch; chunking = its min_size, avg_size,
    max_size, small_file_threshold); their File trees, and every Dir tree bottom-up with children in scan
    order, through packer.add_trees_to_blobs, an UNCHANGED File standing in with the parent's hash.
    Returns (root hash bytes, tree pieces: [context.TREE_BLOB_DTYPE records] in the order they were made,
    the node indices read, ascending).  Writing the packfiles from the blobs is pack_build's."""
    sc = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    names = bytes(names)
    results, _, _, _ = match(session, parent_root, sc, names, trust_before=trust_before, verify=verify)
    n = sc.size
    kind, first, count = sc["kind"].tolist(), sc["child_first"].tolist(), sc["n_children"].tolist()
    name = [names[o:o + ln] for o, ln in zip(sc["name_off"].tolist(), sc["name_len"].tolist())]
    depth = [-1] * n                                  # -1: no Dir names it; children come after their parent
    depth[0] = 0
    for i in range(n):
        if depth[i] >= 0 and kind[i] == _lib.BW_TREE_DIR:
            for k in range(first[i], first[i] + count[i]):
                depth[k] = depth[i] + 1
    node_hash = [None] * n
    status = results["status"].tolist()
    to_read = [i for i in range(n) if depth[i] >= 0 and kind[i] == _lib.BW_TREE_FILE and status[i] != UNCHANGED]
    for i in range(n):
        if depth[i] >= 0 and kind[i] == _lib.BW_TREE_FILE and status[i] == UNCHANGED:
            node_hash[i] = results["hash"][i].tobytes()

    def tree_of(i, children):
        return (kind[i], name[i], _opt(sc[i], "size", _lib.BW_TREE_HAS_SIZE), _opt(sc[i], "mtime", _lib.BW_TREE_HAS_MTIME),
                _opt(sc[i], "ctime", _lib.BW_TREE_HAS_CTIME), children)

    pieces = []
    if to_read:
        datas = [bytes(read_file(i)) for i in to_read]
        lens = [len(d) for d in datas]
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        blobs = packer.process_files(np.frombuffer(b"".join(datas) or b"\0", dtype=np.uint8), offs, lens, ctx=ctx,
                                     dedup=dedup, **chunking)
        kids = [[] for _ in to_read]
        for f, d in zip(blobs["file"].tolist(), blobs["digest"]):
            kids[f].append(d.tobytes())
        hashes, recs = packer.add_trees_to_blobs([tree_of(i, b"".join(k)) for i, k in zip(to_read, kids)], ctx=ctx, dedup=dedup)
        pieces.append(recs)
        for i, h in zip(to_read, hashes):
            node_hash[i] = h.tobytes()
    dirs = [i for i in range(n) if depth[i] >= 0 and kind[i] == _lib.BW_TREE_DIR]
    for d in sorted({depth[i] for i in dirs}, reverse=True):
        level = [i for i in dirs if depth[i] == d]
        trees = [tree_of(i, b"".join(node_hash[k] for k in range(first[i], first[i] + count[i]))) for i in level]
        hashes, recs = packer.add_trees_to_blobs(trees, ctx=ctx, dedup=dedup)
        pieces.append(recs)
        for i, h in zip(level, hashes):
            node_hash[i] = h.tobytes()
    return node_hash[0], pieces, to_read
