#!/usr/bin/env python3
"""The parent match on one GPU (one JSON line on stdout):

  python tools/parent_bench.py [--small-files 200000] [--changed 0.01] [--reps 10] [--slots 0]

A C4-shaped tree store (--small-files files, one chunk each, 1,000 files to a directory) holds one
snapshot.  The scan is the snapshot's own listing with --changed of the files given a new mtime: what a
stat-only walk of the source tree yields on a repeat backup.  No walk opens a chunk, so the store holds
the tree blobs only and the chunk hashes are random.  Timed, each the median of --reps runs after one
warm-up with min and max beside it, in the same run:

  match      bw_parent_match(root, scan): every child's first piece is opened for its name
  full_walk  bw_restore_trees(root): the listing a host-side join would start from
  host_join  the join of scan against listing in Python dicts, (parent, name) -> node, with the verdict

The statuses are checked, not measured: the touched files are CHANGED, every other file UNCHANGED."""
import argparse
import ctypes
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from unpack_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-files", type=int, default=200000)
    ap.add_argument("--changed", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--slots", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch
    from backuwup_amd import Context, _lib, parent, restore
    from backuwup_amd.prune import ERROR_DTYPE

    dev = torch.device("cuda", 0)
    ctx = Context(0)
    sync = torch.cuda.synchronize
    prk = bytes(range(32))
    nf, per_dir = args.small_files, 1000
    rng = np.random.default_rng(3)

    MTIME = 1700000000

    def file_trees(idx, chunk_digests, lens):
        """bincode of Tree { kind: File, name: "f0000123", size: Some(len), mtime: Some(MTIME), ctime: None,
        children: [chunk], next_sibling: None } for the files idx: 80 bytes each."""
        n = idx.size
        t = np.zeros((n, 80), dtype=np.uint8)
        t[:, 4] = 8
        t[:, 12] = ord("f")
        for k in range(7):
            t[:, 13 + k] = 48 + (idx // 10 ** (6 - k)) % 10
        t[:, 20] = 1
        t[:, 21:29] = lens.astype("<u8").view(np.uint8).reshape(n, 8)
        t[:, 29] = 1
        t[:, 30:38] = np.full(n, MTIME, dtype="<u8").view(np.uint8).reshape(n, 8)
        t[:, 39] = 1
        t[:, 47:79] = chunk_digests
        return t

    def dir_tree(name, children):
        nm = name.encode()
        return struct.pack("<IQ", 1, len(nm)) + nm + bytes(3) + struct.pack("<Q", len(children)) + children.tobytes() + b"\0"

    def hashes(blobs):
        ln = np.array([len(b) for b in blobs], dtype=np.uint64)
        off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
        return np.asarray(ctx.blake3_many(np.frombuffer(b"".join(blobs), dtype=np.uint8), off, ln), dtype=np.uint8).reshape(-1, 32)

    def fixed(t):
        n = t.shape[0]
        return np.asarray(ctx.blake3_many(t.reshape(-1), np.arange(n, dtype=np.uint64) * 80, np.full(n, 80, dtype=np.uint64)),
                          dtype=np.uint8).reshape(-1, 32)

    # the snapshot
    idx = np.arange(nf)
    lens = rng.integers(2048, 6144, nf).astype(np.uint64)
    chunks = rng.integers(0, 256, (nf, 32), dtype=np.uint8)
    ft_a = file_trees(idx, chunks, lens)
    fh_a = fixed(ft_a)
    n_mod = max(1, int(nf * args.changed))
    mod = np.sort(rng.choice(nf, n_mod, replace=False))
    starts = list(range(0, nf, per_dir))
    dirs_a = [dir_tree("d%04d" % d, fh_a[lo:lo + per_dir]) for d, lo in enumerate(starts)]
    dh_a = hashes(dirs_a)
    root_a = dir_tree("", dh_a)
    rh = hashes([root_a])
    tail = dirs_a + [root_a]
    trees = np.concatenate([ft_a.reshape(-1), np.frombuffer(b"".join(tail), dtype=np.uint8)])
    t_len = np.concatenate([np.full(nf, 80, dtype=np.uint64), [len(b) for b in tail]]).astype(np.uint64)
    t_off = np.concatenate([[0], np.cumsum(t_len)[:-1]]).astype(np.uint64)
    digests = np.concatenate([fh_a, dh_a, rh]).astype(np.uint8)
    n_trees = int(t_len.size)

    data = torch.from_numpy(trees).to(dev)
    fl = ctx.pack_compress_device(data.data_ptr(), t_off, t_len)
    plan0, total0 = ctx.pack_plan(fl, flags=0)
    ids = rng.integers(0, 256, (len(plan0), 12), dtype=np.uint8)
    nonces = rng.integers(0, 256, (n_trees, 12), dtype=np.uint8)
    d_pf = torch.empty(total0, dtype=torch.uint8, device=dev)
    ctx.pack_build_compressed(prk, digests, np.ones(n_trees, dtype=np.uint8), nonces, plan0, ids, d_pf.data_ptr())
    sync()
    del data
    h = d_pf.cpu().numpy()
    files = [h[int(p["offset"]):int(p["offset"] + p["size"])].tobytes() for p in plan0]
    entries = ctx.unpack_headers(prk, files, [bytes(i) for i in ids])
    del h, files
    which = np.zeros(n_trees, dtype=np.int64)
    for k, p in enumerate(plan0):
        which[int(p["first_blob"]):int(p["first_blob"] + p["n_blobs"])] = k
    items = np.concatenate([digests, ids[which]], axis=1)

    def ms(ts):
        g = sorted(t * 1e3 for t in ts)
        return {"ms_median": round(g[len(g) // 2], 2), "ms_min": round(g[0], 2), "ms_max": round(g[-1], 2), "reps": len(ts)}

    out = {"commit": os.environ.get("BW_COMMIT"), "files": nf, "touched_files": n_mod, "tree_blobs": n_trees,
           "slots": args.slots or 1024}
    ra = rh[0].tobytes()
    with restore.Session(ctx, prk, d_pf.data_ptr(), ids, entries, items, slots=args.slots, plan=plan0) as s:
        nodes, names, chunk_rows = s.trees(ra)
        assert len(nodes) == n_trees
        nb, cb = np.zeros(len(names) + 1, dtype=np.uint8), np.zeros((len(chunk_rows) + 1, 32), dtype=np.uint8)
        wcnt, werr = _lib.BwRestoreCounts(), _lib.BwRestoreError()
        r = (ctypes.c_uint8 * 32).from_buffer_copy(ra)

        def walk():
            rc = s._L.bw_restore_trees(s.h, r, 0, nodes.ctypes.data_as(ctypes.POINTER(_lib.BwRestoreNode)), len(nodes),
                                       nb.ctypes.data_as(ctypes.c_void_p), nb.size, cb.ctypes.data_as(ctypes.c_void_p),
                                       len(cb), ctypes.byref(wcnt), ctypes.byref(werr))
            assert rc == 0, rc

        # the scan: the listing as a stat-only walk would give it, the touched files with a later mtime
        scan = nodes.copy()
        is_file = scan["kind"] == _lib.BW_TREE_FILE
        scan["child_first"][is_file] = 0
        scan["n_children"][is_file] = 0
        file_nodes = np.flatnonzero(is_file)
        touched = file_nodes[mod]
        scan["mtime"][touched] += 60
        sn = np.frombuffer(names, dtype=np.uint8)
        res = np.zeros(len(scan), dtype=parent.RESULT_DTYPE)
        rd, er, cnt = np.zeros(s.n_entries, dtype=np.uint8), np.zeros(1, dtype=ERROR_DTYPE), _lib.BwParentCounts()

        def match():
            rc = s._L.bw_parent_match(s.h, r, 2**64 - 1, 0, scan.ctypes.data_as(ctypes.POINTER(_lib.BwRestoreNode)), len(scan),
                                      sn.ctypes.data_as(ctypes.c_void_p), sn.size, res.ctypes.data_as(ctypes.POINTER(_lib.BwParentResult)),
                                      rd.ctypes.data_as(_lib.u8p), ctypes.byref(cnt), er.ctypes.data_as(ctypes.POINTER(_lib.BwPruneError)), 1)
            assert rc == 0, rc

        match()
        want = np.where(is_file, parent.UNCHANGED, parent.DIR)
        want[touched] = parent.CHANGED
        assert (res["status"] == want).all() and cnt.n_read == n_trees and cnt.n_errors == 0
        assert cnt.n_unchanged == nf - n_mod and cnt.unchanged_bytes == int(scan["size"][is_file].sum() - scan["size"][touched].sum())
        out["match"] = dict(ms(timed(match, args.reps, sync)), n_read=int(cnt.n_read), n_levels=int(cnt.n_levels),
                            n_unchanged=int(cnt.n_unchanged), unchanged_bytes=int(cnt.unchanged_bytes))
        out["full_walk"] = dict(ms(timed(walk, args.reps, sync)), tree_blobs_read=n_trees)

        def host_join():
            """Scan against listing on the host: (matched parent, name) -> listing node, then the verdict."""
            def cols(a):
                return [a[f].tolist() for f in ("kind", "flags", "size", "mtime", "ctime", "child_first", "n_children",
                                                "name_off", "name_len")]
            lk, lf, lsz, lm, lc, lfirst, lcount, loff, llen = cols(nodes)
            table = {}
            for i in range(len(lk)):
                if lk[i] == 1:
                    for k in range(lfirst[i], lfirst[i] + lcount[i]):
                        table.setdefault((i, names[loff[k]:loff[k] + llen[k]]), k)
            sk, sf, ssz, sm, sc, sfirst, scount, soff, slen = cols(scan)
            status, hit = [0] * len(sk), [-1] * len(sk)
            status[0], hit[0] = 4, 0
            n_unch = 0
            for i in range(len(sk)):
                if status[i] != 4:
                    continue
                for k in range(sfirst[i], sfirst[i] + scount[i]):
                    m = table.get((hit[i], names[soff[k]:soff[k] + slen[k]]))
                    if m is None:
                        continue
                    hit[k] = m
                    if sk[k] != lk[m]:
                        status[k] = 5
                    elif sk[k] == 1:
                        status[k] = 4
                    else:
                        same = sf[k] == lf[m] and sf[k] & 3 == 3 and ssz[k] == lsz[m] and sm[k] == lm[m] and \
                            (not sf[k] & 4 or sc[k] == lc[m])
                        status[k] = 1 if same else 2
                        n_unch += same
            assert n_unch == nf - n_mod
        out["host_join"] = ms(timed(host_join, max(3, args.reps // 3), sync))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
