"""backuwup_amd.find.restore_paths and find.find against restore.unpack and tests/find_ref.py: a partial
restore returns exactly the files of the whole restore whose paths the reference matches (a file that
matches, and everything below a directory that matches), byte for byte; for an anchored query the walk
opens fewer tree blobs than a whole walk by the reference's figure."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import find_stores  # noqa: E402
import zstd_ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]


def store_args(ctx, case):
    import restore_store
    files, ids = [b for _, b in case["packs"]], [i for i, _ in case["packs"]]
    return files, ids, ctx.unpack_headers(restore_store.PRK, files, ids), restore_store.items_array(case["index"]), restore_store.PRK


@pytest.mark.parametrize("name, patterns", [("sibling", ["/target/*.txt"]), ("sibling", ["/target", "f00?.txt"]),
                                           ("names", ["/d/K", "*.txt", "€"]), ("wide", ["/d65", "/d257/f25?"])])
def test_restore_paths_is_the_matching_part_of_unpack(ctx, oracle, tmp_path, name, patterns):
    import find_ref
    from backuwup_amd import find, restore
    case, store, hd = find_stores.case(name)
    root = case["roots"][0]
    whole, errors = restore.unpack(ctx, *store_args(ctx, case), root, slots=case["slots"])
    assert not errors
    want = find_ref.walk(store, hd, [root], [p.encode() for p in patterns], subtree=True, chunks=True, kinds=1)
    paths = find_ref.hit_paths(want["records"], 0)
    assert paths and len(paths) < len(whole)
    counts = {}
    part, errors = find.restore_paths(ctx, *store_args(ctx, case), root, patterns, slots=case["slots"], counts=counts)
    assert not errors and sorted(part) == paths and all(part[p] == whole[p] for p in paths)
    assert counts == want["counts"]
    out, errors = find.restore_paths(ctx, *store_args(ctx, case), root, patterns, destination_dir=str(tmp_path), slots=case["slots"])
    assert out is None and not errors
    on_disk = sorted(os.path.relpath(os.path.join(d, f), tmp_path) for d, _, fs in os.walk(tmp_path) for f in fs)
    assert on_disk == paths and all(open(os.path.join(tmp_path, p), "rb").read() == whole[p] for p in paths)


def test_an_anchored_query_opens_fewer_tree_blobs_by_the_references_figure(ctx, oracle):
    import find_ref
    import restore_ref
    from oracle import pack_oracle as po
    import prune_ref
    from backuwup_amd import find
    case, store, hd = find_stores.case("sibling")
    n_tree_blobs = sum(1 for e in prune_ref.flat_entries(hd) if e[2] == po.KIND_TREE)
    anchored = find_ref.walk(store, hd, case["roots"], [b"/target/*.txt"])
    floating = find_ref.walk(store, hd, case["roots"], [b"*.txt"])
    # a whole walk opens every tree blob once for its header and every Dir's once more for its rows
    assert floating["counts"]["n_opened"] == n_tree_blobs + 4 and anchored["counts"]["n_opened"] == 8
    hits, counts, errors = find.find(ctx, *store_args(ctx, case), case["roots"], ["/target/*.txt"], slots=case["slots"])
    assert [h["path"] for h in hits[0]] == ["target/a.txt"] and len(errors) == 0
    assert counts["n_opened"] == anchored["counts"]["n_opened"] and counts["n_pruned"] == anchored["counts"]["n_pruned"] == 2
    assert n_tree_blobs - counts["n_opened"] == n_tree_blobs - anchored["counts"]["n_opened"] > 290
    hits, counts, _ = find.find(ctx, *store_args(ctx, case), case["roots"], ["*.TXT"], icase=True, slots=case["slots"])
    assert counts["n_opened"] == floating["counts"]["n_opened"] and len(hits[0]) == 302


def test_restore_paths_over_a_damaged_store_reports_what_is_missing_or_short(ctx, oracle, tmp_path):
    """find_stores.damaged: restore.unpack raises on it.  restore_paths restores what can be read and names
    every item that is unreadable or cut short, with the tree error's reason: nothing goes missing in silence."""
    import find_ref
    from backuwup_amd import find, restore
    case, store, hd = find_stores.case("damaged")
    root, patterns = case["roots"][0], ["*.txt", "/cut?"]
    with pytest.raises(restore.TreeError):
        restore.unpack(ctx, *store_args(ctx, case), root, slots=case["slots"])
    want = find_ref.walk(store, hd, [root], [p.encode() for p in patterns], subtree=True, chunks=True)
    own = {h: reason for (h, _, _, reason) in want["errors"]}
    later = {by: reason for (_, by, pos, reason) in want["errors"] if pos == find_ref.NONE}
    expect = []
    for r in want["records"]:
        path = b"/".join(r["path"][:-1] + ((b"?" + r["hash"].hex().encode(),) if r["flags"] & find_ref.UNREADABLE else r["path"][-1:]))
        if r["flags"] & (find_ref.UNREADABLE | find_ref.CYCLIC):
            expect.append((path.decode(), own[r["hash"]], find_ref.NONE))
        if r["flags"] & find_ref.TRUNCATED:
            expect.append((path.decode(), later[r["hash"]], find_ref.NONE))
    assert len(expect) == 6 and all(reason for _, reason, _ in expect)  # three first pieces, two Dir chains, the File's
    tree_errors = []
    part, errors = find.restore_paths(ctx, *store_args(ctx, case), root, patterns, slots=case["slots"], tree_errors=tree_errors)
    assert sorted(errors) == sorted(expect)
    assert sorted(tree_errors) == sorted(want["errors"].elements())
    # long.txt records 80 bytes and its second piece is lost: the first piece's one chunk is what comes back
    assert part == {"ok.txt": b"O" * 40, "long.txt": b"c1" * 20, "cut1/ok.txt": b"O" * 40, "cut2/ok.txt": b"O" * 40}
    out, errors = find.restore_paths(ctx, *store_args(ctx, case), root, patterns, destination_dir=str(tmp_path / "new" / "dest"),
                                     slots=case["slots"])
    assert out is None and sorted(errors) == sorted(expect)
    dest = tmp_path / "new" / "dest"
    assert (dest / "long.txt").read_bytes() == b"c1" * 20 and (dest / "cut2" / "ok.txt").read_bytes() == b"O" * 40


def test_restore_paths_creates_matched_directories_and_sets_their_mtimes(ctx, oracle, tmp_path):
    from backuwup_amd import find
    case = find_stores.case("filtered")[0]
    # docs carries mtime 50 and is matched itself; "sub/name" is a matched Dir whose only file lies below it
    out, errors = find.restore_paths(ctx, *store_args(ctx, case), case["roots"][0], ["/docs", "name/"], destination_dir=str(tmp_path / "d"),
                                     slots=case["slots"])
    assert out is None and not errors
    assert os.path.isdir(tmp_path / "d" / "docs") and os.path.isdir(tmp_path / "d" / "sub" / "name")
    assert (tmp_path / "d" / "sub" / "name" / "in").read_bytes() == b"I" * 20 and not os.path.exists(tmp_path / "d" / "name")
    assert int(os.stat(tmp_path / "d" / "docs" / "s3").st_mtime) == 103 and int(os.stat(tmp_path / "d" / "docs").st_mtime) == 50
