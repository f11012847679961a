#!/usr/bin/env python3
"""Impact on one GPU (one JSON line on stdout):

  python tools/impact_bench.py [--small-files 200000] [--snapshots 8] [--changed 0.01] [--reps 10] [--slots 0]

A C4-shaped store (--small-files files of 2-6 KiB, one chunk each, 1,000 files to a directory, every chunk
and every File and Dir tree blob in the packfiles) holds --snapshots snapshots, each with --changed of the
files given a new chunk against the one before.  `bad` is one packfile's entries ("one_packfile"), and again
every tenth packfile's ("tenth").  Timed, each the median of --reps runs after one warm-up with min and max
beside it, in the same run:

  prune_mark    bw_prune_mark over the snapshots' roots: the walk bw_impact_mark does, without the taint
  impact_mark   bw_impact_mark over the same roots, per bad vector, with n_sweeps, n_edges and n_tainted
  impact_paths  bw_impact_paths over the mark's taint, with the records produced
  full_walks    one bw_restore_trees per root: the listings a host-side join would start from

The propagate kernels' share of the mark is not timed here: it is the k_im_propagate rows of a kernel trace
of this tool beside its impact_mark time.  Checked, not measured: no error, every root affected when a
chunk packfile is lost, n_trees_expanded equal to prune's when no tree blob is lost."""
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


def store_arguments(ap):
    ap.add_argument("--small-files", type=int, default=200000)
    ap.add_argument("--snapshots", type=int, default=8)
    ap.add_argument("--changed", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--slots", type=int, default=0)


def build_store(args):
    """The store on the device, shared with tools/retain_bench.py: a dict of ctx, sync, prk, d_pf, ids,
    entries, items, plan0, roots, nf, ns, n_mod, n_trees."""
    import numpy as np
    import torch
    from backuwup_amd import Context
    from backuwup_amd.synth import splitmix_torch

    dev = torch.device("cuda", 0)
    ctx = Context(0)
    sync = torch.cuda.synchronize
    prk = bytes(range(32))
    nf, per_dir, ns = args.small_files, 1000, args.snapshots
    n_mod = max(1, int(nf * args.changed))
    rng = np.random.default_rng(5)

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

    # the chunks: one per file, and one more per changed file and later snapshot
    nc = nf + (ns - 1) * n_mod
    lens = rng.integers(2048, 6144, nc).astype(np.uint64)
    so = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    n_bytes = int(lens.sum())
    data = splitmix_torch(44, n_bytes, dev)
    sync()
    dig = np.asarray(ctx.blake3_many(data.cpu().numpy(), so, lens), dtype=np.uint8).reshape(-1, 32)

    # the snapshots: the file trees and the directories that changed, and a root each
    starts = list(range(0, nf, per_dir))
    cur = np.arange(nf)  # file -> its chunk
    ft = file_trees(np.arange(nf), dig[:nf], lens[:nf])
    fh = fixed(ft)
    file_blobs, tail, tail_hashes, roots = [ft], [], [], []
    dh = np.zeros((len(starts), 32), dtype=np.uint8)
    dirty = set(range(len(starts)))
    for k in range(ns):
        if k:
            mod = np.sort(rng.choice(nf, n_mod, replace=False))
            cur[mod] = nf + (k - 1) * n_mod + np.arange(n_mod)
            t = file_trees(mod, dig[cur[mod]], lens[cur[mod]])
            fh[mod] = fixed(t)
            file_blobs.append(t)
            dirty = set((mod // per_dir).tolist())
        ds = sorted(dirty)
        blobs = [dir_tree("d%04d" % d, fh[starts[d]:starts[d] + per_dir]) for d in ds]
        dh[ds] = hashes(blobs)
        root = dir_tree("", dh)
        rh = hashes([root])
        tail += blobs + [root]
        tail_hashes += [dh[ds].copy(), rh]
        roots.append(rh[0].tobytes())
    ft_all = np.concatenate(file_blobs)
    trees = np.concatenate([ft_all.reshape(-1), np.frombuffer(b"".join(tail), dtype=np.uint8)])
    t_len = np.concatenate([np.full(len(ft_all), 72, dtype=np.uint64), [len(b) for b in tail]]).astype(np.uint64)
    t_off = n_bytes + np.concatenate([[0], np.cumsum(t_len)[:-1]]).astype(np.uint64)
    n_trees = int(t_len.size)
    data = torch.cat([data, torch.from_numpy(trees).to(dev)])
    all_off, all_len = np.concatenate([so, t_off]).astype(np.uint64), np.concatenate([lens, t_len]).astype(np.uint64)
    digests = np.concatenate([dig, fixed(ft_all)] + tail_hashes).astype(np.uint8)
    kinds = np.concatenate([np.zeros(nc, dtype=np.uint8), np.ones(n_trees, dtype=np.uint8)])
    fl = ctx.pack_compress_device(data.data_ptr(), all_off, all_len)
    plan0, total0 = ctx.pack_plan(fl, flags=0)
    ids = rng.integers(0, 256, (len(plan0), 12), dtype=np.uint8)
    nonces = rng.integers(0, 256, (all_len.size, 12), dtype=np.uint8)
    d_pf = torch.empty(total0, dtype=torch.uint8, device=dev)
    ctx.pack_build_compressed(prk, digests, kinds, nonces, plan0, ids, d_pf.data_ptr())
    sync()
    del data
    h = d_pf.cpu().numpy()
    files = [h[int(p["offset"]):int(p["offset"] + p["size"])].tobytes() for p in plan0]
    entries = ctx.unpack_headers(prk, files, [bytes(i) for i in ids])
    del h, files
    which = np.zeros(all_len.size, dtype=np.int64)
    for k, p in enumerate(plan0):
        which[int(p["first_blob"]):int(p["first_blob"] + p["n_blobs"])] = k
    items = np.concatenate([digests, ids[which]], axis=1)
    return dict(ctx=ctx, sync=sync, prk=prk, d_pf=d_pf, ids=ids, entries=entries, items=items, plan0=plan0, roots=roots, nf=nf,
                ns=ns, n_mod=n_mod, n_trees=n_trees)


def ms(ts):
    g = sorted(t * 1e3 for t in ts)
    return {"ms_median": round(g[len(g) // 2], 2), "ms_min": round(g[0], 2), "ms_max": round(g[-1], 2), "reps": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    store_arguments(ap)
    args = ap.parse_args()

    import numpy as np
    from backuwup_amd import _lib, impact, prune, restore
    st = build_store(args)
    ctx, sync, prk, d_pf, ids, entries, items, plan0, roots = (st[k] for k in ("ctx", "sync", "prk", "d_pf", "ids", "entries", "items",
                                                                                 "plan0", "roots"))
    nf, ns, n_mod, n_trees = st["nf"], st["ns"], st["n_mod"], st["n_trees"]

    out = {"commit": os.environ.get("BW_COMMIT"), "files": nf, "snapshots": ns, "changed_per_snapshot": n_mod,
           "tree_blobs": n_trees, "entries": int(len(entries)), "packfiles": int(len(plan0)), "slots": args.slots or 1024}
    with restore.Session(ctx, prk, d_pf.data_ptr(), ids, entries, items, slots=args.slots, plan=plan0) as s:
        live, _, pcounts, perrs = prune.mark(s, roots)
        assert not len(perrs) and live.all() and pcounts["n_trees_expanded"] == n_trees, (len(perrs), pcounts)
        out["prune_mark"] = dict(ms(timed(lambda: prune.mark(s, roots), args.reps, sync)), n_levels=pcounts["n_levels"])

        nodes, names, chunk_rows = s.trees(roots[0])
        nb, cb = np.zeros(len(names) + 64, dtype=np.uint8), np.zeros((len(chunk_rows) + 1, 32), dtype=np.uint8)
        wcnt, werr = _lib.BwRestoreCounts(), _lib.BwRestoreError()
        rbuf = [(ctypes.c_uint8 * 32).from_buffer_copy(r) for r in roots]

        def walks():
            for r in rbuf:  # every snapshot has as many nodes, name bytes and chunk rows as the first
                rc = s._L.bw_restore_trees(s.h, r, 0, nodes.ctypes.data_as(ctypes.POINTER(_lib.BwRestoreNode)), len(nodes),
                                           nb.ctypes.data_as(ctypes.c_void_p), nb.size, cb.ctypes.data_as(ctypes.c_void_p),
                                           len(cb), ctypes.byref(wcnt), ctypes.byref(werr))
                assert rc == 0, rc
        out["full_walks"] = dict(ms(timed(walks, args.reps, sync)), walks=ns, nodes_per_walk=int(len(nodes)))

        chunk_pf = int(entries["packfile"][0])  # the first packfile holds chunks only
        cases = {"one_packfile": [chunk_pf], "tenth": list(range(0, len(plan0), 10))}
        for name, positions in cases.items():
            bad = impact.lost_packfiles(entries, positions)
            taint, affected, counts, errs = impact.mark(s, roots, bad)
            assert not len(errs), len(errs)
            if not (bad[entries["kind"] == 1]).any():
                assert counts["n_trees_expanded"] == n_trees and affected.all()
            res = dict(mark=dict(ms(timed(lambda: impact.mark(s, roots, bad), args.reps, sync)),
                                 **{f: counts[f] for f in ("n_trees_expanded", "n_levels", "n_edges", "n_sweeps", "n_tainted",
                                                           "n_roots_affected")}),
                       bad_entries=int(bad.sum()), bad_tree_entries=int(bad[entries["kind"] == 1].sum()))
            records, _, per_root, pc, perr = impact.paths(s, roots, taint)
            caps = (pc["n_records"], pc["name_bytes"], 64)  # the walk once, not the growing of its buffers
            res["paths"] = dict(ms(timed(lambda: impact.paths(s, roots, taint, caps=caps), args.reps, sync)), n_records=pc["n_records"],
                                n_levels=pc["n_levels"], n_errors=pc["n_errors"], n_files=int(per_root["n_files"].sum()),
                                n_unreadable=int(per_root["n_unreadable"].sum()),
                                lost_chunk_refs=int(per_root["lost_chunk_refs"].sum()))
            out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
