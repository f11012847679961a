#!/usr/bin/env python3
"""Parity throughput on one GPU (one JSON line on stdout):

  python tools/parity_bench.py [--gib 1] [--reps 10]

A C2-shaped store (--gib of random data in ~1 MiB chunks, built on the device as tools/check_bench.py
builds it), k = 8 and m in {1, 2, 4}.  Timed in the same run, each the median of --reps runs after one
warm-up with min and max beside it, in GB/s of source bytes read (the packfiles' bytes; for repair the
bytes of the k shards each group is rebuilt from):
  build         bw_parity_build_device: every group in one k_gf_matmul launch, then the BLAKE3 of every shard
  repair        bw_parity_repair_device group after group with m shards lost in each (the first m packfiles),
                digests given: the survivors are hashed, the lost shards rebuilt and hashed
  gf_matmul     bw_gf_matmul_device alone: an m x 8 matrix over 8 sources of an eighth of the store each
  copy_dtod     a device-to-device copy of the store's bytes, the yardstick"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from check_bench import build_store  # noqa: E402
from unpack_bench import rate, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()

    import numpy as np
    import torch
    import parity_ref
    from backuwup_amd import Context, _lib, make_params, parity
    from backuwup_amd.synth import splitmix_torch

    dev = torch.device("cuda", 0)
    ctx = Context(0)
    sync = torch.cuda.synchronize
    out = {"commit": os.environ.get("BW_COMMIT"), "k": 8}

    n = int(args.gib * (1 << 30))
    data = splitmix_torch(42, n, dev)
    sync()
    blobs = ctx.wait(ctx.submit_device(data.data_ptr(), n, np.array([0], np.uint64), np.array([n], np.uint64), make_params()))
    so, lens = blobs["offset"].astype(np.uint64), blobs["length"].astype(np.uint64)
    d_pf, plan, ids, entries, items, h = build_store(ctx, torch, np, dev, 1, data, so, lens, bytes(range(32)))
    del data
    sizes = plan["size"].astype(np.uint64)
    store = int(sizes.sum())
    out["store_bytes"], out["packfiles"] = store, int(len(plan))
    d_copy = torch.empty(d_pf.numel(), dtype=torch.uint8, device=dev)
    out["copy_dtod"] = rate(store, timed(lambda: d_copy.copy_(d_pf), args.reps, sync))
    del d_copy

    for m in (1, 2, 4):
        groups, total = parity.plan(sizes, 8, m)
        d_par = torch.empty(total + 16, dtype=torch.uint8, device=dev)
        dig = []

        def build():
            dig[:] = [parity.build_device(ctx, d_pf.data_ptr(), plan, groups, d_par.data_ptr(), total)]
        res = {"build": dict(rate(store, timed(build, args.reps, sync)), parity_bytes=total, groups=int(len(groups)))}
        # one group against the numpy reference, and every digest's place
        g0 = groups[0]
        k0, len0 = int(g0["k"]), int(g0["shard_len"])
        want = parity_ref.matmul(parity_ref.cauchy(k0, m), [h[int(p["offset"]):int(p["offset"] + p["size"])] for p in plan[:k0]], len0)
        assert np.array_equal(d_par[:m * len0].cpu().numpy().reshape(m, len0), want), "group 0 differs from the reference"
        assert bytes(dig[0][0]) == ctx.blake3(h[:int(sizes[0])]) and len(dig[0]) == len(plan) + m * len(groups)

        # repair: the first min(m, k) packfiles of every group are lost
        d_out = torch.empty(m * int(groups["shard_len"].max()) + 16, dtype=torch.uint8, device=dev)
        calls, read, at = [], 0, 0
        for g in groups:
            first, k, length, off = int(g["first_packfile"]), int(g["k"]), int(g["shard_len"]), int(g["out_offset"])
            lost = min(m, k)
            present = [s >= lost for s in range(k + m)]
            shard_off = [int(plan["offset"][first + s]) for s in range(k)] + [d_pf.numel() + off + i * length for i in range(m)]
            size = [int(sizes[first + s]) for s in range(k)] + [length] * m
            out_off = [min(s, lost - 1) * length if s < lost else 0 for s in range(k + m)]
            calls.append((np.array([tuple(g)], dtype=parity.GROUP_DTYPE), present, shard_off, size, out_off,
                          dig[0][at:at + k + m], lost))
            read += sum(size[s] for s in range(lost, lost + k))
            at += k + m
        # the parity shards behind the packfiles in one buffer: one base pointer for every shard
        d_all = torch.cat([d_pf, d_par[:total]])
        sync()  # torch's stream is not the context's

        def repair():
            for grp, present, shard_off, size, out_off, dg, lost in calls:
                st = parity.repair_device(ctx, grp, present, d_all.data_ptr(), shard_off, size, d_out.data_ptr(), out_off, digests=dg)
                assert (st[:lost] == _lib.BW_PARITY_REBUILT).all() and not st[lost:].any(), (int(grp["first_packfile"][0]), st.tolist())
        res["repair"] = dict(rate(read, timed(repair, args.reps, sync)), source_bytes=read, lost_per_group=m)
        del d_all, d_out, d_par

        # the kernel alone: m rows over 8 sources of store / 8 bytes each
        part = store // 8 // 16 * 16
        d_dst = torch.empty(m * part, dtype=torch.uint8, device=dev)
        mat = parity_ref.cauchy(8, m)

        def matmul():
            parity.matmul_device(ctx, mat, d_pf.data_ptr(), [c * part for c in range(8)], [part] * 8, d_dst.data_ptr(),
                                 [r * part for r in range(m)], part)
        res["gf_matmul"] = dict(rate(8 * part, timed(matmul, args.reps, sync)), written_bytes=m * part)
        del d_dst
        res["build_vs_copy"] = round(res["build"]["GBps_median"] / out["copy_dtod"]["GBps_median"], 3)
        res["gf_matmul_vs_copy"] = round(res["gf_matmul"]["GBps_median"] / out["copy_dtod"]["GBps_median"], 3)
        out["m%d" % m] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
