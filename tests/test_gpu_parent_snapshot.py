"""backuwup_amd.parent.snapshot end to end: a store holds snapshot A; the scan of B (some files edited,
added, removed and touched) is matched against A, only the files that are not UNCHANGED are read, chunked
and hashed, and the new root hash must be the one a full backup of B gives (restore_store.Builder, the
oracle's write side, with the same child order)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]

DIR_MTIME = 777


def blob(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def specs():
    """A and B: {name: (bytes, mtime) | dict}."""
    rng = np.random.default_rng(77)
    a = {"docs": {"a.txt": (blob(rng, 3000), 1000), "b.txt": (blob(rng, 1500), 1001), "old": {"x": (blob(rng, 2100), 1002)}},
         "src": {"m.c": (blob(rng, 4097), 1003), "gone.c": (blob(rng, 800), 1004), "deep": {"z": (blob(rng, 1024), 1005)}},
         "top": (blob(rng, 2500), 1006), "dropped": {"y": (blob(rng, 900), 1007)}}
    b = {"docs": {"a.txt": (blob(rng, 3100), 2000),            # edited
                  "b.txt": a["docs"]["b.txt"],
                  "old": {"x": a["docs"]["old"]["x"]}},
         "src": {"m.c": (a["src"]["m.c"][0], 2001),             # touched: the same bytes, a later mtime
                 "deep": {"z": a["src"]["deep"]["z"], "fresh": (blob(rng, 1300), 2002)}},   # gone.c removed, fresh added
         "top": a["top"],
         "added": {"n": (blob(rng, 700), 2003)}}                # dropped removed, added added
    return a, b


def full_backup(b, name, v):
    """Builder.add_dir with a file's own mtime: the same calls, children in dict order."""
    if isinstance(v, dict):
        return b.add_tree(1, name, None, DIR_MTIME, None, [full_backup(b, k, x) for k, x in v.items()])
    return b.add_file(name, v[0], v[1])


def scan_of(pm_restore, spec):
    """B as a stat-only scan (nodes NODE_DTYPE, names) plus the bytes behind each File node."""
    rows, data = [("", spec)], {}
    nodes, names = [], bytearray()
    i = 0
    while i < len(rows):
        name, v = rows[i]
        nm = name.encode()
        if isinstance(v, dict):
            nodes.append((1, 2, 0, DIR_MTIME, 0, 0, len(rows), len(v), len(names), len(nm)))
            rows += list(v.items())
        else:
            nodes.append((0, 3, len(v[0]), v[1], 0, 0, 0, 0, len(names), len(nm)))
            data[i] = v[0]
        names += nm
        i += 1
    return np.array(nodes, dtype=pm_restore.NODE_DTYPE), bytes(names), data, [r[0] for r in rows]


CHUNKING = dict(min_size=64, avg_size=256, max_size=1024, small_file_threshold=0)   # restore_store.CDC, every file cut


def test_snapshot_reads_only_what_changed_and_gives_the_full_backups_root(ctx, oracle):
    import restore_store as rs
    from backuwup_amd import parent, restore
    assert rs.CDC == (64, 256, 1024)
    a, b = specs()
    builder = rs.Builder(seed=78)
    root_a = full_backup(builder, "", a)
    packs, index = builder.finish(target=11)
    want_root_b = full_backup(rs.Builder(seed=79), "", b)
    files, ids = [p for _, p in packs], [i for i, _ in packs]
    nodes, names, data, node_names = scan_of(restore, b)
    asked = []

    def read_file(i):
        asked.append(i)
        return data[i]

    with restore.Session(ctx, rs.PRK, files, ids, ctx.unpack_headers(rs.PRK, files, ids), rs.items_array(index), slots=16) as s:
        root, pieces, read = parent.snapshot(ctx, s, root_a, nodes, names, read_file, dedup=False, **CHUNKING)
        changed = sorted(i for i in data if node_names[i] in ("a.txt", "m.c", "fresh", "n"))
        assert sorted(asked) == read == changed and len(asked) == len(set(asked))
        assert root == want_root_b
        assert sum(len(p) for p in pieces) == len(changed) + 6          # one piece per File read and per Dir of B

        # B = A: no file is read and the root is A's
        nodes_a, names_a, data_a, _ = scan_of(restore, a)
        asked.clear()
        root, pieces, read = parent.snapshot(ctx, s, root_a, nodes_a, names_a, read_file, dedup=False, **CHUNKING)
        assert root == root_a and read == [] and asked == []

        # no parent: a full backup, every file read, the same root
        def read_a(i):
            return data_a[i]
        root, _, read = parent.snapshot(ctx, s, None, nodes_a, names_a, read_a, dedup=False, **CHUNKING)
        assert root == root_a and read == sorted(data_a)

        # the parent's start time at the touched file's mtime: everything at or past it is read again
        asked.clear()
        root, _, read = parent.snapshot(ctx, s, root_a, nodes_a, names_a, read_a, trust_before=1003, dedup=False, **CHUNKING)
        assert root == root_a and len(read) == 5                         # mtimes 1003 .. 1007
