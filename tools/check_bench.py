#!/usr/bin/env python3
"""Check throughput on one GPU (one JSON line on stdout):

  python tools/check_bench.py [--gib 1] [--small-files 200000] [--reps 10] [--parts data,structure]

Data rates: a C2-shaped store (--gib of random data in ~1 MiB chunks, built on the device; level 3
writes random data as raw blocks, so the packfiles hold store frames).  Timed in the same run, each the
median of --reps runs after one warm-up with min and max beside it, in GB/s of sealed bytes:
  check_auth     bw_check_data(BW_CHECK_AUTH) over every entry (k_seal_auth: GHASH only)
  open           bw_open_device over the same blobs (AES-CTR + GHASH, a plaintext written)
  copy_dtod      a device-to-device copy of the same number of bytes
  check_full     bw_check_data(BW_CHECK_FULL) over every entry
  unpack_verify  bw_unpack_blobs_device with BW_UNPACK_VERIFY over the same entries, `slots` at a time
BW_SEAL_AUTH_WAVES=16 in the environment selects k_seal_auth's 16-wave workgroups (one per CU) for an
A/B run against the default 8-wave ones.

Structure: the chunk entries of a C4-shaped store (--small-files blobs of 2-6 KiB; the structure pass
reads no blob byte, so the tree blobs are left out), bw_check_structure in ms and entries per second."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from unpack_bench import rate, timed  # noqa: E402


def build_store(ctx, torch, np, dev, seed, data, so, lens, prk):
    """The blobs packed on the device: (d_pf, plan, ids, entries, items)."""
    rng = np.random.default_rng(seed)
    n = int(lens.sum())
    digests = np.asarray(ctx.blake3_many(data.cpu().numpy(), so, lens), dtype=np.uint8).reshape(-1, 32)
    fl = ctx.pack_compress_device(data.data_ptr(), so, lens)
    plan, total = ctx.pack_plan(fl, flags=0)
    ids = rng.integers(0, 256, (len(plan), 12), dtype=np.uint8)
    nonces = rng.integers(0, 256, (lens.size, 12), dtype=np.uint8)
    d_pf = torch.empty(total, dtype=torch.uint8, device=dev)
    ctx.pack_build_compressed(prk, digests, np.zeros(lens.size, dtype=np.uint8), nonces, plan, ids, d_pf.data_ptr())
    torch.cuda.synchronize()
    h = d_pf.cpu().numpy()
    files = [h[int(p["offset"]):int(p["offset"] + p["size"])].tobytes() for p in plan]
    entries = ctx.unpack_headers(prk, files, [bytes(i) for i in ids])
    which = np.zeros(lens.size, dtype=np.int64)
    for k, p in enumerate(plan):
        which[int(p["first_blob"]):int(p["first_blob"] + p["n_blobs"])] = k
    items = np.concatenate([digests, ids[which]], axis=1)
    assert n > 0 and len(entries) == lens.size
    return d_pf, plan, ids, entries, items, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small-files", type=int, default=200000)
    ap.add_argument("--slots", type=int, default=0)
    ap.add_argument("--parts", default="data,structure")
    args = ap.parse_args()

    import numpy as np
    import torch
    from backuwup_amd import Context, check, make_params, restore
    from backuwup_amd.synth import splitmix_torch

    dev = torch.device("cuda", 0)
    ctx = Context(0)
    sync = torch.cuda.synchronize
    prk = bytes(range(32))
    out = {"commit": os.environ.get("BW_COMMIT"), "auth_waves": int(os.environ.get("BW_SEAL_AUTH_WAVES") or 8)}
    parts = args.parts.split(",")

    if "data" in parts:
        n = int(args.gib * (1 << 30))
        data = splitmix_torch(42, n, dev)
        sync()
        blobs = ctx.wait(ctx.submit_device(data.data_ptr(), n, np.array([0], np.uint64), np.array([n], np.uint64), make_params()))
        so, lens = blobs["offset"].astype(np.uint64), blobs["length"].astype(np.uint64)
        d_pf, plan, ids, entries, items, h = build_store(ctx, torch, np, dev, 1, data, so, lens, prk)
        del data
        sealed = int(entries["length"].sum())
        slots = args.slots or 1024
        pfo = plan["offset"][entries["packfile"]] + 8 + plan["header_len"][entries["packfile"]] + entries["offset"]
        nonces = np.stack([h[int(o):int(o) + 12] for o in pfo])
        with restore.Session(ctx, prk, d_pf.data_ptr(), ids, entries, items, slots=args.slots, plan=plan) as s:
            assert not check.data(s, "auth").any() and not check.data(s, "full").any()
            out["check_auth"] = dict(rate(sealed, timed(lambda: check.data(s, "auth"), args.reps, sync)), sealed_bytes=sealed,
                                     entries=int(len(entries)))
            d_tmp = torch.empty(sealed + 64 * len(entries), dtype=torch.uint8, device=dev)
            dof = np.concatenate([[0], np.cumsum((entries["length"] + 47) // 16 * 16)[:-1]]).astype(np.uint64)
            src_off = (pfo + 12).astype(np.uint64)

            def opened():
                ok = ctx.seal_device(prk, d_pf.data_ptr(), src_off, entries["length"], entries["hash"], nonces, d_tmp.data_ptr(), dof,
                                     open_=True)
                assert ok.all()
            out["open"] = rate(sealed, timed(opened, args.reps, sync))
            a, b = d_pf[:sealed], d_tmp[:sealed]
            out["copy_dtod"] = rate(sealed, timed(lambda: b.copy_(a), args.reps, sync))
            del d_tmp
            out["check_full"] = dict(rate(sealed, timed(lambda: check.data(s, "full"), args.reps, sync)), slots=slots)
            flags, ist, stats, counts = check.structure(s)
            assert not flags.any() and not ist.any() and counts["n_packfiles_clean"] == len(plan)
        d_dst = torch.empty(slots * (3 << 20), dtype=torch.uint8, device=dev)
        d_off = np.arange(slots, dtype=np.uint64) * np.uint64(3 << 20)

        def chain():
            for lo in range(0, len(entries), slots):
                part = entries[lo:lo + slots]
                _, st = ctx.unpack_blobs_device(prk, d_pf.data_ptr(), plan, part, d_dst.data_ptr(), d_off[:len(part)], verify=True)
                assert not st.any()
        out["unpack_verify"] = rate(sealed, timed(chain, args.reps, sync))
        del d_dst, d_pf

    if "structure" in parts:
        nf = args.small_files
        rng = np.random.default_rng(2)
        lens = rng.integers(2048, 6144, nf).astype(np.uint64)
        so = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        data = splitmix_torch(43, int(lens.sum()), dev)
        sync()
        d_pf, plan, ids, entries, items, _ = build_store(ctx, torch, np, dev, 3, data, so, lens, prk)
        del data
        with restore.Session(ctx, prk, d_pf.data_ptr(), ids, entries, items, plan=plan) as s:
            flags, ist, stats, counts = check.structure(s)
            assert not flags.any() and not ist.any() and counts["n_packfiles_clean"] == len(plan) and counts["n_entries"] == nf
            ts = sorted(timed(lambda: check.structure(s), args.reps, sync))
            out["structure"] = {"ms_median": round(ts[len(ts) // 2] * 1e3, 3), "ms_min": round(ts[0] * 1e3, 3),
                                "ms_max": round(ts[-1] * 1e3, 3), "entries_per_s_median": round(nf / ts[len(ts) // 2]),
                                "entries": nf, "items": nf, "packfiles": int(len(plan)), "reps": len(ts)}
        del d_pf
    print(json.dumps(out))


if __name__ == "__main__":
    main()
