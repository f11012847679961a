"""Regenerates tests/golden/cdc_windows.json: byte windows whose gear hash passes (or just misses)
the masks of avg = 1 MiB, for tests/cdc_plant.py.

    python tests/golden/make_cdc_windows.py

Found by search over seeded random bytes with the oracle's gear table and masks (about a minute):
  S     48-byte windows whose hash passes mask_s (rate 2^-21 per position)
  L     windows that pass mask_l but not mask_s (~2^-19)
  PRE   windows that pass only the scan's 16-bit prefilter (~2^-16)
  truncated_prefix_mask_s[k], k in {0, 1, 2, 45, 46}: k + 1 bytes whose hash STARTED FROM ZERO passes
        mask_s.  k = 0, 1 and 2 are searched exhaustively (256, 65,536 and 16.7 M prefixes); where
        none exists the entry is null -- tests/test_cdc_plant.py repeats the exhaustive search for
        the null entries, so a null is a checked statement about the gear table, not a gap.
Every entry is re-classified by tests/test_cdc_plant.py.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import cdc_plant as cp  # noqa: E402
from oracle import oracle  # noqa: E402

N_S, N_L, N_PRE = 16, 16, 64


def short_prefixes(gear, k):
    """Every (k + 1)-byte prefix, k <= 2, whose hash from zero passes mask_s; the first or None."""
    g = gear.g
    h = g.copy()
    for _ in range(k):
        h = ((h[:, None] << np.uint64(1)) + g[None, :]).reshape(-1)
    hit = np.nonzero((h & np.uint64(gear.mask_s)) == 0)[0]
    if not len(hit):
        return None
    return int(hit[0]).to_bytes(k + 1, "big")  # row-major: the first byte is the most significant


def long_prefix(gear, k, rng):
    while True:
        rows = rng.integers(0, 256, (1 << 22, k + 1), dtype=np.uint8)
        h = np.zeros(len(rows), dtype=np.uint64)
        for c in range(k + 1):
            h = (h << np.uint64(1)) + gear.g[rows[:, c]]
        hit = np.nonzero((h & np.uint64(gear.mask_s)) == 0)[0]
        if len(hit):
            return rows[hit[0]].tobytes()


def main():
    gear = cp.Gear.of(oracle, cp.P1)
    assert oracle.masks(*cp.P1) == oracle.masks(*cp.BK)
    found = {cp.S: [], cp.L_ONLY: [], cp.PRE_ONLY: []}
    want = {cp.S: N_S, cp.L_ONLY: N_L, cp.PRE_ONLY: N_PRE}
    seed = 1000
    while any(len(found[k]) < want[k] for k in found):
        buf = cp.filler(seed, 1 << 24)
        seed += 1
        h = gear.hash_all(buf)
        for p in np.nonzero((h & np.uint64(gear.mask_pre)) == 0)[0]:
            if p < cp.WINDOW - 1:
                continue
            kind = gear.classify_hash(h[p])
            if len(found[kind]) < want[kind]:
                found[kind].append(buf[p - cp.WINDOW + 1:p + 1].tobytes())
    rng = np.random.default_rng(2000)
    trunc = {}
    for k in (0, 1, 2):
        trunc[k] = short_prefixes(gear, k)
    for k in (45, 46):
        trunc[k] = long_prefix(gear, k, rng)
    out = {"params": list(cp.P1), "mask_s": "%#x" % gear.mask_s, "mask_l": "%#x" % gear.mask_l,
           "mask_pre": "%#x" % gear.mask_pre}
    for k in found:
        out[k] = [w.hex() for w in found[k]]
    out["truncated_prefix_mask_s"] = {str(k): (None if v is None else v.hex()) for k, v in trunc.items()}
    with open(cp.FIXTURE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print({k: len(v) for k, v in found.items()}, {k: v is not None for k, v in trunc.items()})


if __name__ == "__main__":
    main()
