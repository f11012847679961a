"""The pattern language of find stated twice in tests/find_ref.py, cross-checked by enumeration, and
find_ref.walk over the stores of tests/find_stores.py: the properties the device walk is later compared
with (tests/test_gpu_find.py).  No GPU.

The enumeration: for every pattern below and every path over the alphabet {a, b, c} of up to four
components of up to three letters, the position-set simulation accepts exactly when the regex matches, and
a directory's carried state is non-empty exactly when some enumerated path below it matches.  An empty
state with a match below it fails at any depth; a live state must show a match below it wherever the
enumeration still has as many components left as the pattern has outside its '**' (every pattern's
components are of at most three letters of the alphabet, so that many always suffice)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import find_ref  # noqa: E402
import zstd_ref  # noqa: E402

NAMES = [bytes(x) for n in (1, 2, 3) for x in __import__("itertools").product(b"abc", repeat=n)]
PATTERNS = ["a", "/a", "*", "/*/b", "**/c", "/**", "a*b", "/a/**/b", "?", "/??/?", "[ab]c", "/[!a]*", "[^b]", "*a*/", "/a/b/c/a",
            "**/ab/**/c", "/*/*/*/*", "a?c/b", "/**/a/**", "\\a\\b", "[a-b][b-c]", "/ab/", "c*/**/*c", "/a*/b*/c*"]


@pytest.mark.parametrize("icase", [False, True])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_simulation_and_regex_agree_on_every_path(pattern, icase):
    pat = (pattern.upper() if icase else pattern).encode()
    rx, dir_only = find_ref.to_regex(pat, icase)
    nfa = find_ref.Nfa(pat, icase)
    assert nfa.dir_only == dir_only
    memo, seen = {}, [0, 0, 0]
    need = len([c for c in pattern.strip("/").split("/") if c != "**"])  # the components a match has at least

    def below(carried, text, depth):
        """Does any enumerated path under this directory match?  Checks every node on the way."""
        found = False
        for name in NAMES:
            key = (carried, name)
            s = memo.get(key)
            if s is None:
                s = memo[key] = (nfa.accepts(nfa.run(carried, name)), nfa.after_slash(nfa.run(carried, name)))
            child = text + name.decode() + "/"
            verdict = rx.fullmatch(child) is not None
            assert s[0] == verdict, child
            seen[0] += 1
            seen[1] += verdict
            found |= verdict
            if depth < 4:
                deeper = below(s[1], child, depth + 1)
                if not s[1]:
                    assert not deeper, child
                elif 4 - depth >= need:  # a live state is at most `need` components from a match
                    assert deeper, child
                    seen[2] += 1
                found |= deeper
        return found

    assert below(nfa.start, "", 1) and seen[0] == 39 + 39**2 + 39**3 + 39**4 and seen[1] > 0


@pytest.mark.parametrize("pattern, why", [(b"", "empty"), (b"a//b", "empty component"), (b"/", "empty component"), (b"a//", "empty component"),
                                          (b"[ab", "unterminated"), (b"a\\", "dangling"), (b"\xff", "UTF-8"), (b"\xc3", "UTF-8"),
                                          ("[é]".encode(), "ASCII"), (b"[a/b]", "slash"), (b"a\\/b", "slash"), (b"[b-a]", "backwards"),
                                          (b"/" + b"a" * 64, "65 states"), (b"a" * 63, "65 states")])
def test_refusals(pattern, why):
    with pytest.raises(ValueError, match=why):
        find_ref.Nfa(pattern)
    if "states" not in why:
        with pytest.raises(ValueError):
            find_ref.to_regex(pattern)


def test_state_counts():
    for pattern, n in ((b"/" + b"a" * 63, 64), (b"a" * 62, 64), (b"*.jpg", 7), (b"/**", 1), (b"**", 1), (b"**/**/a", 3), (b"/a***b/", 4),
                       (b"/a/**/**/b", 5)):
        assert find_ref.Nfa(pattern).n_states == n, pattern


needs_zstd = pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")


def _ref(name, qi):
    from find_stores import reference
    return reference(name, qi)


@needs_zstd
def test_the_sibling_of_an_anchored_target_is_pruned_and_none_of_its_children_is_a_record(oracle):
    _, _, out = _ref("sibling", 0)
    recs = out["records"]
    big = [r for r in recs if r["path"] == (b"big",)]
    assert len(big) == 1 and big[0]["flags"] == find_ref.PRUNED and big[0]["n_children"] == 0
    assert not [r for r in recs if r["path"][:1] == (b"big",) and len(r["path"]) > 1]
    assert find_ref.hit_paths(recs, 0) == ["target/a.txt"] and out["counts"]["n_pruned"] == 2  # big, and target/sub
    # the root and its two rows, the root's chain, target's three rows and target's chain: nothing under big
    assert out["counts"]["n_opened"] == 1 + 1 + 2 + 1 + 3
    _, _, floating = _ref("sibling", 2)
    assert len(floating["records"]) == 1 + 2 + 300 + 3 + 1 and floating["counts"]["n_pruned"] == 0


@needs_zstd
def test_seventy_levels_under_a_double_star(oracle):
    _, _, out = _ref("deep", 0)
    assert find_ref.hit_paths(out["records"], 0) == ["/".join("d%d" % k for k in range(70)) + "/leaf"]
    assert out["counts"]["n_levels"] == 72
    _, _, anchored = _ref("deep", 3)
    assert find_ref.hit_paths(anchored["records"], 0) == ["d0/d1/d2/side3"] and anchored["counts"]["n_levels"] == 5


@needs_zstd
def test_subtree_filters_and_a_trailing_slash(oracle):
    _, _, out = _ref("filtered", 0)
    assert find_ref.hit_paths(out["records"], 0) == ["docs/s3", "docs/s4", "docs/s5", "docs/s6"]
    assert all(r["patterns"] == 1 for r in out["records"] if r["path"][:1] == (b"docs",))
    assert find_ref.hit_paths(_ref("filtered", 1)[2]["records"], 0) == ["docs/s%d" % k for k in range(3, 9)]
    assert "docs/nosize" not in find_ref.hit_paths(_ref("filtered", 2)[2]["records"], 0)
    assert find_ref.hit_paths(_ref("filtered", 3)[2]["records"], 0) == ["sub/name"]
    assert find_ref.hit_paths(_ref("filtered", 4)[2]["records"], 0) == ["name", "sub/name"]


@needs_zstd
def test_two_pieces_with_and_without_chunks(oracle):
    _, _, plain = _ref("two_pieces", 0)
    _, _, rows = _ref("two_pieces", 1)
    assert plain["counts"]["n_chunks"] == 0 and rows["counts"]["n_chunks"] == 10001
    assert rows["counts"]["n_opened"] == plain["counts"]["n_opened"] + 2
    _, _, kids = _ref("two_pieces", 2)
    assert kids["counts"]["n_records"] == 1 + 2 + 10001 and kids["counts"]["n_chunks"] == 10001
    assert kids["per_root"][0]["n_hit_files"] == 10001 and kids["per_root"][0]["hit_bytes"] == 40 * 10001


@needs_zstd
def test_shared_subtrees_give_records_under_each(oracle):
    _, _, out = _ref("shared", 0)
    assert find_ref.hit_paths(out["records"], 0) == ["f.jpg", "one/f.jpg", "two/in/f.jpg"] == find_ref.hit_paths(out["records"], 2)
    assert find_ref.hit_paths(out["records"], 1) == ["one/f.jpg"]


@needs_zstd
def test_loops_and_damage(oracle):
    _, _, out = _ref("dir_contains_itself", 0)
    assert [r["flags"] for r in out["records"]] == [0, find_ref.CYCLIC, find_ref.HIT]
    c, _, out = _ref("chain_names_itself", 0)
    loop = next(r for r in out["records"] if r["name"] == b"loop")
    assert loop["flags"] == find_ref.TRUNCATED and loop["n_children"] == c["n_entries"] + 1
    _, _, out = _ref("damaged", 1)
    flags = {r["path"][-1]: r["flags"] for r in out["records"] if r["level"] == 1}
    assert flags[b"ok.txt"] == find_ref.HIT and flags[b"long.txt"] == find_ref.HIT | find_ref.TRUNCATED
    assert flags[b"cut1"] == flags[b"cut2"] == find_ref.TRUNCATED and sum(f == find_ref.UNREADABLE for f in flags.values()) == 3
    assert out["records"][1]["flags"] == find_ref.UNREADABLE and out["per_root"][1]["n_unreadable"] == 1
    assert sum(out["errors"].values()) == 1 + 3 + 2 + 1  # the second root; three first pieces; two Dir chains; the File's


@needs_zstd
def test_every_query_count_is_what_the_stores_say(oracle):
    import find_stores
    assert sorted(find_stores.N_QUERIES) == sorted(find_stores.NAMES)
    for name in find_stores.NAMES:
        assert len(find_stores.case(name)[0]["queries"]) == find_stores.N_QUERIES[name], name
    _, query, out = _ref("names", 17)
    assert len(query["patterns"]) == 32 and out["counts"]["n_pruned"] == 0
