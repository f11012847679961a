#!/usr/bin/env python3
"""Find on one GPU (one JSON line on stdout):

  python tools/find_bench.py [--small-files 200000] [--snapshots 8] [--reps 10] [--step-seconds 900]

On the store of tools/impact_bench.py (--small-files files "f0000123" of one chunk each, 1,000 to a directory
"d0007", --snapshots roots) three queries over all roots at once, each in a process of its own under
`timeout`, the next one only when the one before ended well:

  float     "*77": a floating suffix, what *.ext is on a store with extensions
  anchored  "/d0?00/f*": leaves one directory in a hundred alive
  many      32 anchored patterns at once, each one directory and one two-digit suffix

Timed per query, the median of --reps runs after one warm-up with min and max beside it, in the same run:

  find       bw_find_paths with buffers of the right size (the walk once, not the growing)
  host_loop  one bw_restore_trees per root, the paths joined and a Python `re` per pattern over every path
             (tests/find_ref.py's translation), the median of 3

with n_opened, n_pruned, the records and the hits.  Checked, not measured: no error, and find's hits per root
equal the host loop's."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

QUERIES = {"float": ["*77"], "anchored": ["/d0?00/f*"], "many": ["/d%04d/*%02d" % (6 * k, k) for k in range(32)]}


def one(args):
    import numpy as np
    from impact_bench import build_store, ms
    from unpack_bench import timed
    import find_ref
    from backuwup_amd import find, restore
    st = build_store(args)
    ctx, sync, roots = st["ctx"], st["sync"], st["roots"]
    patterns = QUERIES[args.query]
    rx = [find_ref.to_regex(p.encode())[0] for p in patterns]
    out = {"query": args.query, "patterns": len(patterns), "files": st["nf"], "roots": len(roots), "tree_blobs": st["n_trees"]}
    with restore.Session(ctx, st["prk"], st["d_pf"].data_ptr(), st["ids"], st["entries"], st["items"], slots=args.slots,
                         plan=st["plan0"]) as s:
        recs, names, _, per_root, counts, errs = find.paths(s, roots, patterns)
        assert not len(errs), len(errs)
        caps = (counts["n_records"], counts["name_bytes"], 1, 64)
        out["find"] = dict(ms(timed(lambda: find.paths(s, roots, patterns, caps=caps), args.reps, sync)),
                           **{f: counts[f] for f in ("n_records", "n_levels", "n_opened", "n_pruned")},
                           n_hits=int(per_root["n_hits"].sum()))

        def host_loop():
            hits = []
            for r in roots:
                nodes, nm, _ = s.trees(r)
                paths = restore.walk_paths(nodes, nm)
                hits.append(sum(1 for p in paths[1:] if any(x.fullmatch(p + "/") for x in rx)))
            return hits
        want = host_loop()
        assert want == per_root["n_hits"].tolist(), (want, per_root["n_hits"].tolist())
        out["host_loop"] = dict(ms(timed(host_loop, 3, sync)), hits=int(np.sum(want)))
    print(json.dumps(out))


def main():
    from impact_bench import store_arguments
    ap = argparse.ArgumentParser()
    store_arguments(ap)
    ap.add_argument("--query", choices=sorted(QUERIES))
    ap.add_argument("--step-seconds", type=int, default=900)
    args = ap.parse_args()
    if args.query:
        return one(args)
    out = {"commit": os.environ.get("BW_COMMIT"), "queries": []}
    for q in ("float", "anchored", "many"):
        cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--query", q,
               "--small-files", str(args.small_files), "--snapshots", str(args.snapshots), "--changed", str(args.changed),
               "--reps", str(args.reps), "--slots", str(args.slots)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE)
        if p.returncode:  # a step that failed or ran out of time ends the run: nothing more is started on the GPU
            out["failed"] = {"query": q, "exit": p.returncode}
            print(json.dumps(out))
            return p.returncode
        out["queries"].append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
