#!/usr/bin/env python3
"""Prune throughput on one GPU (one JSON line on stdout):

  python tools/prune_bench.py [--gib 1] [--small-files 200000] [--reps 10] [--parts repack,mark]

Repack rate: a C2-shaped store (--gib of random data in ~1 MiB chunks, built on the device) with every
second blob dead; bw_prune_repack_device moves the live half into new packfiles, in GB/s of moved
bytes.  The yardstick, timed in the same run, is a device-to-device copy of the same number of bytes:
both move two bytes per byte.  Every figure is the median of --reps timed runs after one warm-up,
with min and max beside it.

Mark rate: a C4-shaped store (--small-files files of 2-6 KiB, one chunk each, 1,000 files to a
directory, every File and Dir tree blob in the packfiles) marked from its root, in tree blobs per
second.  Beside it, in the same run: bw_restore_trees from the same root, and the unpack chain alone
over the same tree blobs `slots` at a time, which is what every sub-batch of the mark goes through."""
import argparse
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from unpack_bench import rate, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small-files", type=int, default=200000)
    ap.add_argument("--slots", type=int, default=0)
    ap.add_argument("--parts", default="repack,mark")
    ap.add_argument("--repack-only", action="store_true", help="skip the yardstick (for a kernel-trace run)")
    args = ap.parse_args()

    import numpy as np
    import torch
    from backuwup_amd import Context, make_params, prune, restore

    dev = torch.device("cuda", 0)
    ctx = Context(0)
    sync = torch.cuda.synchronize
    prk = bytes(range(32))
    out = {"commit": os.environ.get("BW_COMMIT")}

    parts = args.parts.split(",")
    from backuwup_amd.synth import splitmix_torch
    if "repack" in parts:
        n = int(args.gib * (1 << 30))
        data = splitmix_torch(42, n, dev)
        sync()
        blobs = ctx.wait(ctx.submit_device(data.data_ptr(), n, np.array([0], np.uint64), np.array([n], np.uint64), make_params()))
        so, lens, digests = blobs["offset"].astype(np.uint64), blobs["length"].astype(np.uint64), blobs["digest"].copy()
        rng = np.random.default_rng(1)
        fl = ctx.pack_compress_device(data.data_ptr(), so, lens)
        plan0, total0 = ctx.pack_plan(fl, flags=0)
        ids = rng.integers(0, 256, (len(plan0), 12), dtype=np.uint8)
        nonces = rng.integers(0, 256, (lens.size, 12), dtype=np.uint8)
        d_pf = torch.empty(total0, dtype=torch.uint8, device=dev)
        ctx.pack_build_compressed(prk, digests, np.zeros(lens.size, dtype=np.uint8), nonces, plan0, ids, d_pf.data_ptr())
        sync()
        del data
        h = d_pf.cpu().numpy()
        files = [h[int(p["offset"]):int(p["offset"] + p["size"])].tobytes() for p in plan0]
        entries = ctx.unpack_headers(prk, files, [bytes(i) for i in ids])
        which = np.zeros(lens.size, dtype=np.int64)
        for k, p in enumerate(plan0):
            which[int(p["first_blob"]):int(p["first_blob"] + p["n_blobs"])] = k
        items = np.concatenate([digests, ids[which]], axis=1)

        live = (np.arange(len(entries)) % 2 == 0).astype(np.uint8)  # half the blobs dead
        tab = plan0.copy()
        order, plan, total = prune.plan(entries, tab, live, np.ones(len(plan0), dtype=np.uint8))
        moved = int((entries["length"][order.astype(np.int64)] + 12).sum())
        new_ids = rng.integers(0, 256, (len(plan), 12), dtype=np.uint8)
        d_out = torch.empty(total + 64, dtype=torch.uint8, device=dev)
        with restore.Session(ctx, prk, d_pf.data_ptr(), ids, entries, items, plan=plan0) as s:
            prune.repack_device(s, order, plan, new_ids, d_out.data_ptr())
            sync()
            # spot check: the first and the last moved blob arrived verbatim
            for k in (0, order.size - 1):
                e = entries[int(order[k])]
                g = int(np.searchsorted(plan["first_blob"], k, side="right") - 1)
                src = int(plan0[int(e["packfile"])]["offset"] + 8 + plan0[int(e["packfile"])]["header_len"] + e["offset"])
                sect = int((entries["length"][order[int(plan[g]["first_blob"]):k].astype(np.int64)] + 12).sum())
                dst = int(plan[g]["offset"] + 8 + plan[g]["header_len"]) + sect
                ln = 12 + int(e["length"])
                assert torch.equal(d_out[dst:dst + ln], d_pf[src:src + ln]), k
            out["repack"] = dict(rate(moved, timed(lambda: prune.repack_device(s, order, plan, new_ids, d_out.data_ptr()), args.reps, sync)),
                                 moved_bytes=moved, moved_blobs=int(order.size), new_packfiles=int(len(plan)))
            if not args.repack_only:
                a, b = d_pf[:moved], d_out[:moved]
                out["copy_dtod"] = dict(rate(moved, timed(lambda: b.copy_(a), args.reps, sync)), bytes=moved)

        del d_pf, d_out

    def file_trees(chunk_digests, lens):
        """bincode of Tree { kind: File, name: "f0000123", size: Some(len), mtime: None, ctime: None,
        children: [chunk], next_sibling: None } for every file: 72 bytes each."""
        n = lens.size
        t = np.zeros((n, 72), dtype=np.uint8)
        t[:, 4] = 8                                        # name length (u64 LE); kind 0 = File before it
        t[:, 12] = ord("f")
        idx = np.arange(n)
        for k in range(7):
            t[:, 13 + k] = 48 + (idx // 10 ** (6 - k)) % 10
        t[:, 20] = 1                                       # size: Some
        t[:, 21:29] = lens.astype("<u8").view(np.uint8).reshape(n, 8)
        t[:, 31] = 1                                       # one child (u64 LE at 31; mtime and ctime None before it)
        t[:, 39:71] = chunk_digests
        return t

    def dir_tree(name, children):
        nm = name.encode()
        return struct.pack("<IQ", 1, len(nm)) + nm + bytes(3) + struct.pack("<Q", len(children)) + children.tobytes() + b"\0"

    if "mark" in parts:
        import ctypes
        from backuwup_amd import _lib
        nf, per_dir = args.small_files, 1000
        rng = np.random.default_rng(2)
        lens = rng.integers(2048, 6144, nf).astype(np.uint64)
        so = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        n = int(lens.sum())
        data = splitmix_torch(43, n, dev)
        sync()
        dig = ctx.blake3_many_device(data.data_ptr(), n, so, lens) if hasattr(ctx, "blake3_many_device") else \
            ctx.blake3_many(data.cpu().numpy(), so, lens)
        dig = np.asarray(dig, dtype=np.uint8).reshape(-1, 32)
        ft = file_trees(dig, lens)
        fh = ctx.blake3_many(ft.reshape(-1), np.arange(nf, dtype=np.uint64) * 72, np.full(nf, 72, dtype=np.uint64))
        dirs = [dir_tree("d%04d" % d, fh[lo:lo + per_dir]) for d, lo in enumerate(range(0, nf, per_dir))]
        dl = np.array([len(d) for d in dirs], dtype=np.uint64)
        do = np.concatenate([[0], np.cumsum(dl)[:-1]]).astype(np.uint64)
        dh = ctx.blake3_many(np.frombuffer(b"".join(dirs), dtype=np.uint8), do, dl)
        root = dir_tree("", dh)
        root_hash = ctx.blake3_many(np.frombuffer(root, dtype=np.uint8), [0], [len(root)])
        trees = np.concatenate([ft.reshape(-1), np.frombuffer(b"".join(dirs) + root, dtype=np.uint8)])
        t_len = np.concatenate([np.full(nf, 72, dtype=np.uint64), dl, [len(root)]]).astype(np.uint64)
        t_off = n + np.concatenate([[0], np.cumsum(t_len)[:-1]]).astype(np.uint64)
        n_trees = int(t_len.size)
        data = torch.cat([data, torch.from_numpy(trees).to(dev)])
        all_off, all_len = np.concatenate([so, t_off]).astype(np.uint64), np.concatenate([lens, t_len]).astype(np.uint64)
        digests = np.concatenate([dig, fh, dh, root_hash]).astype(np.uint8)
        kinds = np.concatenate([np.zeros(nf, dtype=np.uint8), np.ones(n_trees, dtype=np.uint8)])
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
        slots = args.slots or 1024

        def per_s(ts):
            g = sorted(n_trees / t for t in ts)
            return {"tree_blobs_per_s_median": round(g[len(g) // 2]), "tree_blobs_per_s_min": round(g[0]),
                    "tree_blobs_per_s_max": round(g[-1]), "ms_median": round(sorted(ts)[len(ts) // 2] * 1e3, 2), "reps": len(ts)}

        with restore.Session(ctx, prk, d_pf.data_ptr(), ids, entries, items, slots=args.slots, plan=plan0) as s:
            live, stats, counts, errs = prune.mark(s, root_hash)
            assert not len(errs) and live.all() and counts["n_trees_expanded"] == n_trees, (len(errs), counts)
            out["mark"] = dict(per_s(timed(lambda: prune.mark(s, root_hash), args.reps, sync)), tree_blobs=n_trees,
                               files=nf, entries=int(len(entries)), packfiles=int(len(plan0)), slots=slots,
                               levels=counts["n_levels"], sub_batches=sum(-(-m // slots) for m in (1, len(dirs), nf)))
            nodes, names, chunks = s.trees(root_hash[0].tobytes())
            assert len(nodes) == n_trees and len(chunks) == nf
            nb, cb = np.zeros(len(names) + 1, dtype=np.uint8), np.zeros((nf, 32), dtype=np.uint8)
            cnt, err = _lib.BwRestoreCounts(), _lib.BwRestoreError()
            rh = (ctypes.c_uint8 * 32).from_buffer_copy(root_hash[0].tobytes())

            def walk():
                rc = s._L.bw_restore_trees(s.h, rh, 0, nodes.ctypes.data_as(ctypes.POINTER(_lib.BwRestoreNode)), len(nodes),
                                           nb.ctypes.data_as(ctypes.c_void_p), nb.size, cb.ctypes.data_as(ctypes.c_void_p), nf,
                                           ctypes.byref(cnt), ctypes.byref(err))
                assert rc == 0, rc
            out["restore_trees"] = per_s(timed(walk, args.reps, sync))
        # the chain alone over the tree blobs, `slots` at a time
        te = entries[entries["kind"] == 1]
        assert te.size == n_trees
        d_tmp = torch.empty(slots * (3 << 20), dtype=torch.uint8, device=dev)
        dof = np.arange(slots, dtype=np.uint64) * np.uint64(3 << 20)

        def chain():
            for lo in range(0, te.size, slots):
                part = te[lo:lo + slots]
                ctx.unpack_blobs_device(prk, d_pf.data_ptr(), plan0, part, d_tmp.data_ptr(), dof[:len(part)])
        out["unpack_chain_tree_blobs"] = dict(per_s(timed(chain, args.reps, sync)), sub_batches=-(-te.size // slots))
        del d_tmp, d_pf
    print(json.dumps(out))


if __name__ == "__main__":
    main()
