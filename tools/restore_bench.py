#!/usr/bin/env python3
"""Restore throughput on one GPU, in GB/s of file bytes (one JSON line on stdout):

  python tools/restore_bench.py [--gib 1] [--small-files 200000] [--reps 10] [--stores c2,c4,shared]

Three stores, each built on the device (bw_pack_compress_device + bw_pack_build_compressed):
  c2      --gib of random data in ~1 MiB chunks, one file;
  c4      --small-files files of 2-6 KiB, one chunk each;
  shared  the same 64 MiB laid out as 16 files: every distinct blob is decoded once per sub-batch.
Per store: bw_restore_files_device (locate, open, decode, scan, gather) into one window, and, as
the yardstick, bw_unpack_blobs_device over the same packfiles and the same distinct blobs.  Every
figure is the median of --reps timed runs after one warm-up, with min and max beside it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from unpack_bench import rate, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--small-files", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--stores", default="c2,c4,shared")
    ap.add_argument("--slots", type=int, default=0)
    ap.add_argument("--restore-only", action="store_true", help="skip the yardstick (for a kernel-trace run)")
    args = ap.parse_args()

    import numpy as np
    import torch
    from backuwup_amd import Context, make_params, restore
    from backuwup_amd.synth import splitmix_torch

    dev = torch.device("cuda", 0)
    ctx = Context(0)
    sync = torch.cuda.synchronize
    prk = bytes(range(32))
    out = {"commit": os.environ.get("BW_COMMIT"), "slots": args.slots or 1024}

    def store(data, so, lens, digests):
        """Packfiles on the device from the blobs data[so[i] .. + lens[i]) -> (d_pf, plan, ids, entries, items)."""
        rng = np.random.default_rng(1)
        fl = ctx.pack_compress_device(data.data_ptr(), so, lens)
        plan, total = ctx.pack_plan(fl, flags=0)
        ids = rng.integers(0, 256, (len(plan), 12), dtype=np.uint8)
        nonces = rng.integers(0, 256, (lens.size, 12), dtype=np.uint8)
        d_pf = torch.empty(total, dtype=torch.uint8, device=dev)
        ctx.pack_build_compressed(prk, digests, np.zeros(lens.size, dtype=np.uint8), nonces, plan, ids, d_pf.data_ptr())
        sync()
        h = d_pf.cpu().numpy()
        files = [h[int(p["offset"]):int(p["offset"] + p["size"])].tobytes() for p in plan]
        entries = ctx.unpack_headers(prk, files, [bytes(i) for i in ids])
        which = np.zeros(lens.size, dtype=np.int64)
        for k, p in enumerate(plan):
            which[int(p["first_blob"]):int(p["first_blob"] + p["n_blobs"])] = k
        items = np.concatenate([digests, ids[which]], axis=1)
        return d_pf, plan, ids, entries, items

    def measure(name, data, so, lens, digests, rows, ff, want):
        """rows / ff: the request; want(off) -> the expected bytes of a sample of files."""
        d_pf, plan, ids, entries, items = store(data, so, lens, digests)
        total = int(lens[rows].sum())
        d_dst = torch.empty(total + 64, dtype=torch.uint8, device=dev)
        chunks = digests[rows]
        with restore.Session(ctx, prk, d_pf.data_ptr(), ids, entries, items, slots=args.slots, plan=plan) as s:
            rc, done, off, ln, st, _ = s.files_device(chunks, ff, d_dst.data_ptr(), total)
            assert rc == 0 and done == ff.size - 1 and not st.any(), (rc, done, np.flatnonzero(st)[:8])
            want(d_dst, off, ln)
            res = dict(rate(total, timed(lambda: s.files_device(chunks, ff, d_dst.data_ptr(), total), args.reps, sync)),
                       files=int(ff.size - 1), file_bytes=total, distinct_blobs=int(lens.size), packfiles=int(len(plan)))
        out["restore_" + name] = res
        if not args.restore_only:  # the yardstick: the chain alone over the distinct blobs, 1,024 at a time
            step = 1024
            d_tmp = torch.empty(step * (3 << 20), dtype=torch.uint8, device=dev)
            do = np.arange(step, dtype=np.uint64) * np.uint64(3 << 20)

            def chain():
                for lo in range(0, len(entries), step):
                    part = entries[lo:lo + step]
                    ctx.unpack_blobs_device(prk, d_pf.data_ptr(), plan, part, d_tmp.data_ptr(), do[:len(part)])
            out["unpack_blobs_" + name] = dict(rate(int(lens.sum()), timed(chain, args.reps, sync)), blobs=int(lens.size))
            del d_tmp
        del d_dst, d_pf

    for name in args.stores.split(","):
        if name == "c2":
            n = int(args.gib * (1 << 30))
            data = splitmix_torch(42, n, dev)
            sync()
            t = ctx.submit_device(data.data_ptr(), n, np.array([0], np.uint64), np.array([n], np.uint64), make_params())
            blobs = ctx.wait(t)
            so, lens = blobs["offset"].astype(np.uint64), blobs["length"].astype(np.uint64)
            rows, ff = np.arange(lens.size), np.array([0, lens.size], dtype=np.uint64)

            def want(d_dst, off, ln, data=data, n=n):
                assert int(ln[0]) == n and torch.equal(d_dst[:n], data)
            measure(name, data, so, lens, blobs["digest"].copy(), rows, ff, want)
        elif name == "c4":
            rng = np.random.default_rng(2)
            lens = rng.integers(2048, 6144, args.small_files).astype(np.uint64)
            so = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
            n = int(lens.sum())
            data = splitmix_torch(43, n, dev)
            sync()
            dig = ctx.blake3_many_device(data.data_ptr(), n, so, lens) if hasattr(ctx, "blake3_many_device") else \
                ctx.blake3_many(data.cpu().numpy(), so, lens)
            rows, ff = np.arange(lens.size), np.arange(lens.size + 1, dtype=np.uint64)

            def want(d_dst, off, ln, data=data, n=n, so=so):
                assert np.array_equal(off, so) and torch.equal(d_dst[:n], data)
            measure(name, data, so, lens, np.asarray(dig, dtype=np.uint8).reshape(-1, 32), rows, ff, want)
        elif name == "shared":
            n = 64 << 20
            data = splitmix_torch(44, n, dev)
            sync()
            t = ctx.submit_device(data.data_ptr(), n, np.array([0], np.uint64), np.array([n], np.uint64), make_params())
            blobs = ctx.wait(t)
            so, lens = blobs["offset"].astype(np.uint64), blobs["length"].astype(np.uint64)
            rows = np.tile(np.arange(lens.size), 16)
            ff = (np.arange(17) * lens.size).astype(np.uint64)

            def want(d_dst, off, ln, data=data, n=n):
                assert (ln == n).all()
                for k in (0, 7, 15):
                    assert torch.equal(d_dst[k * n:(k + 1) * n], data), k
            measure(name, data, so, lens, blobs["digest"].copy(), rows, ff, want)
        del data
    print(json.dumps(out))


if __name__ == "__main__":
    main()
