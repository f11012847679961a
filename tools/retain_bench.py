#!/usr/bin/env python3
"""Retain on one GPU (one JSON line on stdout):

  python tools/retain_bench.py [--small-files 200000] [--snapshots 8] [--changed 0.01] [--reps 10] [--slots 0]
                               [--mark-only]

The store is tools/impact_bench.py's (build_store): --small-files files of 2-6 KiB, one chunk each, 1,000
files to a directory, --snapshots snapshots of --changed new chunks each.  Timed, each the median of --reps
runs after one warm-up with min and max beside it, in the same run:

  retain_mark    bw_retain_mark over the snapshots' roots, with n_edges and n_sweeps
  prune_mark     bw_prune_mark over the same roots: the walk without the root sets
  n_plus_1_marks bw_prune_mark over all roots and over all but one for every root: how the bytes each
                 snapshot alone holds are had without retain (the unique figures are checked to agree)
  retain_drop    bw_retain_drop for the single-root drop sets, all in one call, with and without live

--mark-only runs bw_retain_mark alone (--reps times after a warm-up): under a kernel trace of that run the
k_rt_propagate and k_rt_stats rows beside the whole give the share of the mark spent pushing and counting
the root sets.  Checked, not measured: no error, every entry reached, each drop set's live vector equal to
the prune mark over the kept roots."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from impact_bench import build_store, ms, store_arguments  # noqa: E402
from unpack_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    store_arguments(ap)
    ap.add_argument("--mark-only", action="store_true")
    args = ap.parse_args()

    from backuwup_amd import prune, restore, retain
    st = build_store(args)
    ctx, sync, roots, entries, plan0 = st["ctx"], st["sync"], st["roots"], st["entries"], st["plan0"]
    n = len(roots)
    out = {"commit": os.environ.get("BW_COMMIT"), "files": st["nf"], "snapshots": st["ns"], "changed_per_snapshot": st["n_mod"],
           "tree_blobs": st["n_trees"], "entries": int(len(entries)), "packfiles": int(len(plan0)), "slots": args.slots or 1024}
    with restore.Session(ctx, st["prk"], st["d_pf"].data_ptr(), st["ids"], entries, st["items"], slots=args.slots, plan=plan0) as s:
        masks, damaged, per_root, counts, errs = retain.mark(s, roots)
        assert not len(errs) and not damaged.any() and counts["orphan_blobs"] == 0 and counts["n_trees_expanded"] == st["n_trees"]
        out["retain_mark"] = dict(ms(timed(lambda: retain.mark(s, roots), args.reps, sync)),
                                  **{f: counts[f] for f in ("n_trees_expanded", "n_levels", "n_edges", "n_sweeps")})
        if args.mark_only:
            print(json.dumps(out))
            return
        out["prune_mark"] = ms(timed(lambda: prune.mark(s, roots), args.reps, sync))

        def n_plus_1():
            res = [prune.mark(s, roots)]
            for k in range(n):
                res.append(prune.mark(s, roots[:k] + roots[k + 1:]))
            return res
        marks = n_plus_1()
        all_bytes = marks[0][2]["live_bytes"]
        assert [all_bytes - m[2]["live_bytes"] for m in marks[1:]] == per_root["unique_bytes"].tolist()
        out["n_plus_1_marks"] = dict(ms(timed(n_plus_1, args.reps, sync)), marks=n + 1)
        out["unique_bytes"] = per_root["unique_bytes"].tolist()
        out["reached_bytes"] = per_root["reached_bytes"].tolist()

        sets = [[k] for k in range(n)]
        live, stats, freed = retain.drop(s, masks, n, sets)
        for k in range(n):
            assert live[k].tobytes() == marks[1 + k][0].tobytes() and stats[k].tobytes() == marks[1 + k][1].tobytes()
        assert freed["freed_bytes"].tolist() == per_root["unique_bytes"].tolist()
        out["retain_drop"] = dict(ms(timed(lambda: retain.drop(s, masks, n, sets), args.reps, sync)), sets=n)
        out["retain_drop_no_live"] = dict(ms(timed(lambda: retain.drop(s, masks, n, sets, want_live=False), args.reps, sync)), sets=n)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
