#!/usr/bin/env python3
"""Rekey throughput on one GPU (one JSON line on stdout):

  python tools/rekey_bench.py [--gib 1] [--reps 10]

A C2-shaped store (--gib of random data in ~1 MiB chunks, built on the device as tools/check_bench.py
builds it).  Timed in the same run, each the median of --reps runs after one warm-up with min and max
beside it, in GB/s of sealed bytes:
  reseal        bw_reseal_device over every blob (k_reseal_ctr: two keystreams and two GHASH in one pass,
                every byte read once and written once, no plaintext stored)
  open_seal     bw_open_device followed by bw_seal_device over the same blobs: the composition the ABI
                allowed before, with the store's plaintext in a second buffer
  copy_dtod     a device-to-device copy of the same number of bytes
  rekey_store   bw_rekey_store_device over the session (headers, blobs and the bytes between them)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from check_bench import build_store  # noqa: E402
from unpack_bench import rate, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()

    import numpy as np
    import torch
    from backuwup_amd import Context, check, make_params, rekey, restore
    from backuwup_amd.synth import splitmix_torch

    dev = torch.device("cuda", 0)
    ctx = Context(0)
    sync = torch.cuda.synchronize
    old, new = bytes(range(32)), bytes(range(100, 132))
    out = {"commit": os.environ.get("BW_COMMIT")}

    n = int(args.gib * (1 << 30))
    data = splitmix_torch(42, n, dev)
    sync()
    blobs = ctx.wait(ctx.submit_device(data.data_ptr(), n, np.array([0], np.uint64), np.array([n], np.uint64), make_params()))
    so, lens = blobs["offset"].astype(np.uint64), blobs["length"].astype(np.uint64)
    d_pf, plan, ids, entries, items, h = build_store(ctx, torch, np, dev, 1, data, so, lens, old)
    del data
    sealed = int(entries["length"].sum())
    pfo = plan["offset"][entries["packfile"]] + 8 + plan["header_len"][entries["packfile"]] + entries["offset"]
    nonces = np.stack([h[int(o):int(o) + 12] for o in pfo])
    src_off = (pfo + 12).astype(np.uint64)
    slen = entries["length"].astype(np.uint64)
    dof = np.concatenate([[0], np.cumsum((slen + 47) // 16 * 16)[:-1]]).astype(np.uint64)
    d_new = torch.empty(sealed + 64 * len(entries), dtype=torch.uint8, device=dev)
    d_plain = torch.empty(sealed + 64 * len(entries), dtype=torch.uint8, device=dev)

    def reseal():
        ok = rekey.reseal_device(ctx, old, new, d_pf.data_ptr(), src_off, slen, entries["hash"], nonces, d_new.data_ptr(), dof)
        assert ok.all()
    out["reseal"] = dict(rate(sealed, timed(reseal, args.reps, sync)), sealed_bytes=sealed, entries=int(len(entries)))
    assert check.auth_device(ctx, new, d_new.data_ptr(), dof, slen, entries["hash"], nonces).all()
    first = d_new.clone()

    def open_seal():
        ok = ctx.seal_device(old, d_pf.data_ptr(), src_off, slen, entries["hash"], nonces, d_plain.data_ptr(), dof, open_=True)
        assert ok.all()
        ctx.seal_device(new, d_plain.data_ptr(), dof, slen - 16, entries["hash"], nonces, d_new.data_ptr(), dof)
    out["open_seal"] = rate(sealed, timed(open_seal, args.reps, sync))
    sync()
    assert torch.equal(first, d_new), "the composition and the single pass disagree"
    del first
    a, b = d_pf[:sealed], d_plain[:sealed]
    out["copy_dtod"] = rate(sealed, timed(lambda: b.copy_(a), args.reps, sync))
    del d_plain, d_new

    d_out = torch.empty(d_pf.numel(), dtype=torch.uint8, device=dev)
    with restore.Session(ctx, old, d_pf.data_ptr(), ids, entries, items, plan=plan) as s:
        def store():
            est, pst = rekey.rekey_store(s, new, d_out=d_out.data_ptr())
            assert not est.any() and not pst.any()
        out["rekey_store"] = dict(rate(sealed, timed(store, args.reps, sync)), store_bytes=int(d_pf.numel()),
                                  packfiles=int(len(plan)))
    with restore.Session(ctx, new, d_out.data_ptr(), ids, entries, items, plan=plan) as s:
        assert not check.data(s, "auth").any()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
