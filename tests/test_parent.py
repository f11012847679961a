"""tests/parent_ref.py, the plain-Python statement of the parent match, against hand-written expectations
over the stores of tests/parent_stores.py: the reference itself is checked here, without a GPU.  Also
backuwup_amd.parent.scan_directory against os.stat."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402

pytestmark = pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")

NEW, UNCHANGED, CHANGED, RACY, DIR, TYPE_CHANGED = range(6)
NONE = 2**64 - 1
ZERO = bytes(32)


@pytest.fixture(scope="module")
def pm(oracle):
    import parent_ref
    import parent_stores
    import prune_ref
    import restore_ref
    import restore_store

    class NS:
        pass
    ns = NS()
    ns.ref, ns.stores, ns.pref, ns.rr, ns.PRK = parent_ref, parent_stores, prune_ref, restore_ref, restore_store.PRK
    return ns


def run(pm, c, root="case", trust=None):
    store = pm.rr.Store(pm.PRK, c["packs"], c["index"])
    hd = pm.pref.headers_of(pm.PRK, c["packs"])
    out = pm.ref.match(store, hd, c["root"] if root == "case" else root, c["scan"], c["trust"] if trust is None else trust)
    return out, store, hd


def status_by_path(pm, c, res, paths):
    return {p: res[pm.stores.where(c["scan"], p)][0] for p in paths}


def test_identity_every_file_unchanged_every_dir_descended(pm):
    c = pm.stores.identity()
    (res, errors, read, levels, n_unch, unch_bytes), store, hd = run(pm, c)
    assert not errors
    for sn, (st, h) in zip(c["scan"], res):
        assert st == (DIR if sn["kind"] == 1 else UNCHANGED) and h != ZERO
    files = [sn for sn in c["scan"] if sn["kind"] == 0]
    assert n_unch == len(files) == 11 and unch_bytes == sum(sn["size"] for sn in files) == 3370
    assert levels == 4                                # root; docs, src, none, etc; old, deep; deeper
    ents = pm.pref.flat_entries(hd)
    assert read == {e for e, ent in enumerate(ents) if ent[2] == 1}   # every Tree entry, and no chunk
    assert res[0][1] == c["root"]
    # the hash is the parent's child hash: the one a restore finds under that name
    t = pm.rr.fetch_tree(store, res[pm.stores.where(c["scan"], "docs")][1])
    assert t.name == "docs" and res[pm.stores.where(c["scan"], "docs/a.txt")][1] == t.children[0]


def test_one_field_off(pm):
    c = pm.stores.fields()
    (res, errors, _, levels, n_unch, unch_bytes), _, _ = run(pm, c)
    got = status_by_path(pm, c, res, c["want"])
    assert got == c["want"] and not errors and levels == 1
    assert n_unch == 2 and unch_bytes == 20 and got["no_mtime_both"] == CHANGED and got["no_size_both"] == CHANGED


def test_names_compare_whole(pm):
    c = pm.stores.names()
    (res, errors, _, _, n_unch, _), _, _ = run(pm, c)
    scan = c["scan"]
    d = scan[1]
    kids = list(range(d["child_first"], d["child_first"] + d["n_children"]))
    st = [res[k][0] for k in kids]
    assert st[:c["n_same"]] == [UNCHANGED] * c["n_same"] and st[c["n_same"]:] == [NEW] * 5 and n_unch == c["n_same"]
    assert all(res[k][1] == ZERO for k in kids[c["n_same"]:]) and not errors


def test_trust_before(pm):
    c = pm.stores.trust(pm.stores.TRUST)
    (res, _, _, _, n_unch, unch_bytes), _, _ = run(pm, c)
    assert status_by_path(pm, c, res, ["before", "at", "after", "changed"]) == \
        dict(before=UNCHANGED, at=RACY, after=RACY, changed=CHANGED)
    assert (n_unch, unch_bytes) == (1, 1)
    assert all(h != ZERO for _, h in res)             # RACY and CHANGED carry the parent's hash too
    (res, _, _, _, n_unch, unch_bytes), _, _ = run(pm, c, trust=NONE)
    assert status_by_path(pm, c, res, ["before", "at", "after", "changed"]) == \
        dict(before=UNCHANGED, at=UNCHANGED, after=UNCHANGED, changed=CHANGED)
    assert (n_unch, unch_bytes) == (3, 6)


def test_content_replaced_is_unchanged_that_is_the_heuristic(pm):
    """The parent holds other bytes under an equal name, size, mtime and ctime.  A stat-only scan cannot
    see that: the node is UNCHANGED and keeps the parent's hash.  This is the heuristic, not a defect."""
    c = pm.stores.content_replaced()
    (res, _, _, _, n_unch, _), store, _ = run(pm, c)
    i = pm.stores.where(c["scan"], "d/f")
    assert res[i][0] == UNCHANGED and n_unch == 2
    t = pm.rr.fetch_tree(store, res[i][1])
    assert pm.rr.restore_file(store, t)[0] == b"old!"


def test_duplicate_names(pm):
    c = pm.stores.duplicates()
    (res, errors, _, levels, _, _), store, _ = run(pm, c)
    scan = c["scan"]
    d = pm.stores.where(scan, "d")
    kids = list(range(scan[d]["child_first"], scan[d]["child_first"] + scan[d]["n_children"]))
    # the parent's first "dup" (size 1) answers for all three scan nodes of that name
    assert [res[k][0] for k in kids] == [UNCHANGED, UNCHANGED, UNCHANGED, CHANGED]
    assert res[kids[0]][1] == res[kids[1]][1] == res[kids[3]][1] != res[kids[2]][1]
    e = pm.stores.where(scan, "e")
    subs = list(range(scan[e]["child_first"], scan[e]["child_first"] + scan[e]["n_children"]))
    assert [res[k][0] for k in subs] == [DIR, DIR] and res[subs[0]][1] == res[subs[1]][1]
    below = [res[k][0] for s in subs for k in range(scan[s]["child_first"], scan[s]["child_first"] + scan[s]["n_children"])]
    assert below == [UNCHANGED, NEW, UNCHANGED] and levels == 3 and not errors


def test_the_item_is_part_of_the_key(pm):
    c = pm.stores.same_name_in_many_dirs()
    (res, _, _, _, n_unch, _), _, _ = run(pm, c)
    for k in range(c["n"]):
        assert res[pm.stores.where(c["scan"], "d%03d/a" % k)][0] == (UNCHANGED if k % 7 else CHANGED)
    assert n_unch == c["n"] - len(range(0, c["n"], 7))


def test_chains(pm):
    c = pm.stores.dir_chains()
    (res, errors, _, _, _, _), _, _ = run(pm, c)
    assert status_by_path(pm, c, res, ["split/k%d" % k for k in (0, 2, 3, 4, 5, 9)]) == \
        {"split/k0": 1, "split/k2": 1, "split/k3": 1, "split/k4": 2, "split/k5": 1, "split/k9": 0} and not errors
    c = pm.stores.file_chain_and_loop()
    (res, errors, read, _, _, _), _, hd = run(pm, c)
    ents = pm.pref.flat_entries(hd)
    assert res[pm.stores.where(c["scan"], "f3")][0] == UNCHANGED
    assert not {e for e in read if ents[e][1] in c["later"]}        # the File's later pieces are never opened
    assert list(errors) == [(c["loop"], c["loop"], NONE, pm.rr.EFORMAT)]
    assert status_by_path(pm, c, res, ["loop", "loop/in_loop", "loop/other"]) == {"loop": DIR, "loop/in_loop": 1, "loop/other": 0}


def test_structure(pm):
    c = pm.stores.structure()
    (res, errors, read, levels, _, _), store, hd = run(pm, c)
    want = {"kept": DIR, "kept/f": UNCHANGED, "added": NEW, "added/deep": NEW, "added/deep/g": NEW, "added/h": NEW,
            "was_file": TYPE_CHANGED, "was_file/below": NEW, "was_file/sub": NEW, "was_file/sub/x": NEW, "was_dir": TYPE_CHANGED}
    assert status_by_path(pm, c, res, want) == want and not errors and levels == 2
    ents = pm.pref.flat_entries(hd)
    names = {pm.rr.fetch_tree(store, ents[e][1]).name for e in read}
    assert names == {"", "kept", "removed", "was_file", "was_dir", "f"}   # nothing below removed or was_dir
    out, _, _ = run(pm, c, root=None)
    assert out[0] == [(NEW, ZERO)] * len(c["scan"]) and not out[1] and not out[2] and out[3:] == (0, 0, 0)
    c = pm.stores.root_is_file()
    (res, errors, read, levels, _, _), _, _ = run(pm, c)
    assert res[0] == (TYPE_CHANGED, c["root"]) and res[1] == (NEW, ZERO) and levels == 1 and len(read) == 1 and not errors
    c = pm.stores.root_unreadable()
    (res, errors, read, levels, _, _), _, _ = run(pm, c)
    assert res == [(NEW, ZERO)] * 2 and list(errors) == [(c["root"], ZERO, 0, pm.rr.ENOTFOUND)] and levels == 1 and not read


def test_damage(pm):
    c = pm.stores.damaged()
    (res, errors, _, _, n_unch, _), _, _ = run(pm, c)
    for k, name in enumerate(pm.stores.DAMAGE):
        assert errors[(c["bad"][name], c["root"], 2 * k + 1, c["reasons"][name])] == 1, name
        assert res[pm.stores.where(c["scan"], name)] == (NEW, ZERO)
    assert sum(errors.values()) == 7 and n_unch == 8
    c = pm.stores.broken_dir_chain()
    (res, errors, _, _, _, _), _, _ = run(pm, c)
    assert list(errors) == [(c["lost"], c["first"], NONE, pm.rr.ENOTFOUND)]
    assert [res[pm.stores.where(c["scan"], "d/k%d" % k)][0] for k in range(5)] == [1, 1, 0, 0, 0]


def test_scan_rules(pm):
    ok, bad = pm.stores.invalid_scans()
    assert not pm.ref.scan_invalid(ok) and len(bad) == 7
    for what, s in bad.items():
        assert pm.ref.scan_invalid(s), what


def test_scan_directory_gives_what_stat_gives(tmp_path):
    from backuwup_amd import parent
    (tmp_path / "sub" / "deeper").mkdir(parents=True)
    (tmp_path / "empty_dir").mkdir()
    (tmp_path / "b.txt").write_bytes(b"x" * 1234)
    (tmp_path / "a.bin").write_bytes(b"")
    (tmp_path / "sub" / "f").write_bytes(b"abc")
    (tmp_path / "sub" / "deeper" / "g").write_bytes(b"defgh")
    os.symlink(tmp_path / "b.txt", tmp_path / "link")            # neither a file nor a directory: left out
    os.utime(tmp_path / "b.txt", (1600000000.75, 1600000000.75))
    nodes, names = parent.scan_directory(tmp_path)
    paths = {0: ""}
    for i, n in enumerate(nodes):
        if n["kind"] == 1:
            for k in range(int(n["child_first"]), int(n["child_first"] + n["n_children"])):
                nm = names[int(nodes[k]["name_off"]):int(nodes[k]["name_off"] + nodes[k]["name_len"])].decode()
                paths[k] = (paths[i] + "/" if paths[i] else "") + nm
                assert nodes[k]["parent"] == i and k > i
        else:
            assert n["n_children"] == 0
    assert sorted(paths.values()) == ["", "a.bin", "b.txt", "empty_dir", "sub", "sub/deeper", "sub/deeper/g", "sub/f"]
    assert len(paths) == len(nodes) and nodes[0]["parent"] == NONE
    assert names[int(nodes[0]["name_off"]):int(nodes[0]["name_off"] + nodes[0]["name_len"])] == os.fsencode(tmp_path.name)
    for i, p in paths.items():
        st = os.stat(tmp_path / p)
        n = nodes[i]
        assert n["kind"] == (1 if os.path.isdir(tmp_path / p) else 0)
        assert n["size"] == st.st_size and n["mtime"] == int(st.st_mtime) and n["flags"] & 3 == 3
        birth = getattr(st, "st_birthtime", None)
        assert bool(n["flags"] & 4) == (birth is not None) and (birth is None or n["ctime"] == int(birth))
    assert nodes[[i for i, p in paths.items() if p == "b.txt"][0]]["mtime"] == 1600000000
