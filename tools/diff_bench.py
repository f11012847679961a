#!/usr/bin/env python3
"""The diff walk on one GPU (one JSON line on stdout):

  python tools/diff_bench.py [--small-files 200000] [--changed 0.01] [--reps 10] [--slots 0]

A C4-shaped tree store (--small-files files, one chunk each, 1,000 files to a directory) holds two
snapshots: B is A with --changed of the files modified (another chunk hash and size).  Neither walk
opens a chunk, so the store holds the tree blobs only and the chunk hashes are random.  Timed, each
the median of --reps runs after one warm-up with min and max beside it, in the same run:

  diff          bw_diff_trees(A, B): the walk that opens only the tree blobs on changed paths
  full_walks    bw_restore_trees(A) and bw_restore_trees(B): what full_walk_diff spends on the device
  diff_vs_null  bw_diff_trees(NULL, B): lists all of B, the walk's worst case
  full_walk_b   bw_restore_trees(B) alone, the yardstick of diff_vs_null

n_read is checked, not measured: it is what rule 7 of the walk gives (both roots, both sides of every
changed directory and file)."""
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
    from backuwup_amd import Context, _lib, diff, restore
    from backuwup_amd.prune import ERROR_DTYPE

    dev = torch.device("cuda", 0)
    ctx = Context(0)
    sync = torch.cuda.synchronize
    prk = bytes(range(32))
    nf, per_dir = args.small_files, 1000
    rng = np.random.default_rng(3)

    def file_trees(idx, chunk_digests, lens):
        """bincode of Tree { kind: File, name: "f0000123", size: Some(len), mtime: None, ctime: None,
        children: [chunk], next_sibling: None } for the files idx: 72 bytes each."""
        n = idx.size
        t = np.zeros((n, 72), dtype=np.uint8)
        t[:, 4] = 8
        t[:, 12] = ord("f")
        for k in range(7):
            t[:, 13 + k] = 48 + (idx // 10 ** (6 - k)) % 10
        t[:, 20] = 1
        t[:, 21:29] = lens.astype("<u8").view(np.uint8).reshape(n, 8)
        t[:, 31] = 1
        t[:, 39:71] = chunk_digests
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
        return np.asarray(ctx.blake3_many(t.reshape(-1), np.arange(n, dtype=np.uint64) * 72, np.full(n, 72, dtype=np.uint64)),
                          dtype=np.uint8).reshape(-1, 32)

    # snapshot A, and B with n_mod files modified
    idx = np.arange(nf)
    lens = rng.integers(2048, 6144, nf).astype(np.uint64)
    chunks = rng.integers(0, 256, (nf, 32), dtype=np.uint8)
    ft_a = file_trees(idx, chunks, lens)
    fh_a = fixed(ft_a)
    n_mod = max(1, int(nf * args.changed))
    mod = np.sort(rng.choice(nf, n_mod, replace=False))
    ft_m = file_trees(mod, rng.integers(0, 256, (n_mod, 32), dtype=np.uint8), lens[mod] + np.uint64(1))
    fh_b = fh_a.copy()
    fh_b[mod] = fixed(ft_m)
    starts = list(range(0, nf, per_dir))
    dirs_a = [dir_tree("d%04d" % d, fh_a[lo:lo + per_dir]) for d, lo in enumerate(starts)]
    changed_dirs = sorted(set((mod // per_dir).tolist()))
    dirs_m = [dir_tree("d%04d" % d, fh_b[starts[d]:starts[d] + per_dir]) for d in changed_dirs]
    dh_a = hashes(dirs_a)
    dh_b = dh_a.copy()
    dh_b[changed_dirs] = hashes(dirs_m)
    root_a, root_b = dir_tree("", dh_a), dir_tree("", dh_b)
    rh = hashes([root_a, root_b])
    tail = dirs_a + dirs_m + [root_a, root_b]
    trees = np.concatenate([ft_a.reshape(-1), ft_m.reshape(-1), np.frombuffer(b"".join(tail), dtype=np.uint8)])
    t_len = np.concatenate([np.full(nf + n_mod, 72, dtype=np.uint64), [len(b) for b in tail]]).astype(np.uint64)
    t_off = np.concatenate([[0], np.cumsum(t_len)[:-1]]).astype(np.uint64)
    digests = np.concatenate([fh_a, fh_b[mod], dh_a, dh_b[changed_dirs], rh]).astype(np.uint8)
    n_trees = int(t_len.size)
    n_trees_b = nf + len(dirs_a) + 1

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

    out = {"commit": os.environ.get("BW_COMMIT"), "files": nf, "modified_files": n_mod, "changed_dirs": len(changed_dirs),
           "tree_blobs": n_trees, "tree_blobs_of_b": n_trees_b, "slots": args.slots or 1024}
    ra, rb = rh[0].tobytes(), rh[1].tobytes()
    with restore.Session(ctx, prk, d_pf.data_ptr(), ids, entries, items, slots=args.slots, plan=plan0) as s:
        def diff_call(a, b):
            """bw_diff_trees into arrays sized by a first walk: the timed call allocates nothing."""
            records, names, read, counts, errors = diff.trees(s, a, b)
            assert not len(errors), len(errors)
            rec = np.zeros(len(records) + 1, dtype=diff.RECORD_DTYPE)
            nm, rd = np.zeros(len(names) + 1, dtype=np.uint8), np.zeros(s.n_entries, dtype=np.uint8)
            er, cnt = np.zeros(1, dtype=ERROR_DTYPE), _lib.BwDiffCounts()
            roots = [None if r is None else (ctypes.c_uint8 * 32).from_buffer_copy(r) for r in (a, b)]

            def call():
                rc = s._L.bw_diff_trees(s.h, roots[0], roots[1], 0, rec.ctypes.data_as(ctypes.POINTER(_lib.BwDiffRecord)),
                                        len(rec), nm.ctypes.data_as(ctypes.c_void_p), nm.size, rd.ctypes.data_as(_lib.u8p),
                                        ctypes.byref(cnt), er.ctypes.data_as(ctypes.POINTER(_lib.BwPruneError)), 1)
                assert rc == 0, rc
            return call, counts

        def walk_call(root):
            nodes, names, chunk_rows = s.trees(root)
            nb, cb = np.zeros(len(names) + 1, dtype=np.uint8), np.zeros((len(chunk_rows) + 1, 32), dtype=np.uint8)
            cnt, err = _lib.BwRestoreCounts(), _lib.BwRestoreError()
            r = (ctypes.c_uint8 * 32).from_buffer_copy(root)

            def call():
                rc = s._L.bw_restore_trees(s.h, r, 0, nodes.ctypes.data_as(ctypes.POINTER(_lib.BwRestoreNode)), len(nodes),
                                           nb.ctypes.data_as(ctypes.c_void_p), nb.size, cb.ctypes.data_as(ctypes.c_void_p),
                                           len(cb), ctypes.byref(cnt), ctypes.byref(err))
                assert rc == 0, rc
            return call, len(nodes)

        call, counts = diff_call(ra, rb)
        want_read = 2 + 2 * len(changed_dirs) + 2 * n_mod          # rule 7: both sides of every changed node
        assert counts["n_read"] == want_read and counts["n_records"] == 1 + len(changed_dirs) + n_mod, counts
        out["diff"] = dict(ms(timed(call, args.reps, sync)), n_read=counts["n_read"], n_records=counts["n_records"],
                           n_levels=counts["n_levels"])
        walk_a, na = walk_call(ra)
        walk_b, nb_ = walk_call(rb)
        assert na == nb_ == n_trees_b
        out["full_walks"] = dict(ms(timed(lambda: (walk_a(), walk_b()), args.reps, sync)), tree_blobs_read=2 * n_trees_b)
        call0, counts0 = diff_call(None, rb)
        assert counts0["n_read"] == n_trees_b and counts0["n_records"] == n_trees_b, counts0
        out["diff_vs_null"] = dict(ms(timed(call0, args.reps, sync)), n_read=counts0["n_read"], n_records=counts0["n_records"])
        out["full_walk_b"] = dict(ms(timed(walk_b, args.reps, sync)), tree_blobs_read=n_trees_b)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
