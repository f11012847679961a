"""check -> impact -> restore over one store with chunk-only damage: the files impact.impact names under a
root are exactly the files restore.unpack fails on for that root.  Restore is ground truth that
tests/impact_ref.py did not write.  The store keeps one blob per packfile, so that check's bad_packfiles
(whole packfiles to fetch again, which impact.bad_from_check counts as lost) name the two damaged chunks
and nothing else."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]


def test_impact_names_the_files_restore_fails_on(ctx, oracle):
    import prune_ref
    import restore_store as rs
    from backuwup_amd import check, impact, restore
    rng = np.random.default_rng(91)
    b = rs.Builder(seed=91)
    files = {"d%d" % i: {"f%d" % j: rng.integers(0, 256, 700 + 40 * j, dtype=np.uint8).tobytes() for j in range(4)} for i in range(3)}
    shared = rng.integers(0, 256, 900, dtype=np.uint8).tobytes()
    snaps = [dict(files, top=shared), dict(files, top=shared, extra={"copy": shared}),
             dict({k: v for k, v in files.items() if k != "d0"}, d3={"f0": files["d0"]["f0"], "new": b"n" * 300})]
    roots = [b.add_dir("snap", spec) for spec in snaps]
    packs, index = b.finish(target=1)
    hd = prune_ref.headers_of(rs.PRK, packs)
    ents = prune_ref.flat_entries(hd)
    def chunk_of(data):
        _, o, n = oracle.fastcdc(data, *rs.CDC)[0]
        return oracle.blake3(data[o:o + n])

    hit = {chunk_of(shared), chunk_of(files["d0"]["f0"])}  # the first chunk of a file in every snapshot, and of one in two places
    for p, h, kind, _, length, offset in ents:
        if h in hit:
            assert kind == 0
            buf = bytearray(packs[p][1])
            buf[8 + hd[p][2] + offset + 12 + length // 2] ^= 1
            packs[p] = (packs[p][0], bytes(buf))
    data, ids = [x for _, x in packs], [i for i, _ in packs]
    entries, items = ctx.unpack_headers(rs.PRK, data, ids), rs.items_array(index)

    report = check.check(ctx, data, ids, entries, items, rs.PRK, read_data="auth")
    bad = impact.bad_from_check(report, entries)
    assert not report["ok"] and int(bad.sum()) == 2
    per_root, counts, errors = impact.impact(ctx, data, ids, entries, items, rs.PRK, roots, bad, slots=16)
    assert len(errors) == 0 and counts["n_roots_affected"] == 3
    want = [{"top", "d0/f0"}, {"top", "extra/copy", "d0/f0"}, {"d3/f0"}]
    for r, root in enumerate(roots):
        _, failed = restore.unpack(ctx, data, ids, entries, items, rs.PRK, root, slots=16)
        mine = sorted(path for path, kind, flags, n_affected, _ in per_root[r] if kind == 0 and not flags & impact.F_UNREADABLE)
        assert mine == sorted(path for path, _, _ in failed) and set(mine) == want[r]
        assert all(n_affected == 1 for _, kind, _, n_affected, _ in per_root[r] if kind == 0)
