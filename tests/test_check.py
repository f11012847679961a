"""Check without a GPU: tests/check_ref.py, the yardstick of tests/test_gpu_check.py, gives exactly the
hand-written finding for every store those tests use, and the new structs of the C ABI have the sizes
the ctypes and numpy mirrors assume."""
import ctypes
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)


@pytest.fixture(scope="module")
def cs(oracle):
    import check_ref
    import check_stores
    import prune_ref
    import restore_ref

    class NS:
        pass
    ns = NS()
    ns.cr, ns.st, ns.pref, ns.rr = check_ref, check_stores, prune_ref, restore_ref
    return ns


@pytest.fixture(scope="module")
def cases(cs):
    return cs.st.structure_cases()


def test_clean_stores_yield_nothing(cs, cases):
    for packs, index in (cases["clean"][:2], cs.st.one_packfile_of_300(), cs.st.thousand_packfiles_of_one()):
        hd = cs.pref.headers_of(cs.st.PRK, packs)
        flags, items, stats, counts = cs.cr.structure(hd, index)
        assert not any(flags) and not any(items) and all(st["tail"] == 0 for st in stats)
        assert counts["n_packfiles_clean"] == len(packs) and counts["n_items_ok"] == len(index) == counts["n_entries"]
        assert counts["claimed_bytes"] == counts["section_bytes"] == sum(len(b) - 8 - h[2] for (_, b), h in zip(packs, hd))
        assert cs.cr.bad_packfiles(hd, flags, stats) == []


NAMES = ["length past the section", "length 15", "offsets swapped", "overlap by one byte", "truncated by one byte",
         "five trailing bytes", "dropped index item", "item with an unknown id", "item naming a packfile that lacks the hash",
         "item three times", "one hash twice in a packfile", "one hash twice, indexed twice", "all together"]


@pytest.mark.parametrize("name", NAMES)
def test_each_damage_yields_exactly_its_finding(cs, cases, name):
    packs, index, finding = cases[name]
    assert finding
    hd = cs.pref.headers_of(cs.st.PRK, packs)
    flags, items, stats, counts = cs.cr.structure(hd, index)
    wf, wi, wt = cs.st.expected(hd, index, finding)
    assert flags == wf and items == wi and [st["tail"] for st in stats] == wt
    dirty = {p for p, t in enumerate(wt) if t} | {cs.pref.flat_entries(hd)[e][0] for e, f in enumerate(wf) if f}
    assert counts["n_packfiles_clean"] == len(packs) - len(dirty)
    assert cs.cr.bad_packfiles(hd, flags, stats) == sorted(dirty)
    for bit, key in ((1, "n_range"), (2, "n_order"), (4, "n_unindexed"), (8, "n_shadowed")):
        assert counts[key] == sum(1 for f in wf if f & bit)
    assert counts["n_items_duplicate"] == wi.count(cs.cr.IDUPLICATE) and counts["n_items_nopackfile"] == wi.count(cs.rr.ENOPACKFILE)
    assert counts["n_items_mismatch"] == wi.count(cs.rr.EMISMATCH) and counts["n_items_ok"] == wi.count(cs.rr.OK)


def test_data_damage_by_openssl_libzstd_and_blake3(cs):
    import zstd_ref
    if not zstd_ref.available():
        pytest.skip("system libzstd not found")
    packs, index, exp, _ = cs.st.data_store()
    hd = cs.pref.headers_of(cs.st.PRK, packs)
    hashes = [e[1] for e in cs.pref.flat_entries(hd)]
    auth, full = cs.cr.data(cs.st.PRK, packs, hd, "auth"), cs.cr.data(cs.st.PRK, packs, hd, "full")
    assert len(hashes) == 22 and set(exp) <= set(hashes)
    assert auth == [exp.get(h, (0, 0))[0] for h in hashes] and full == [exp.get(h, (0, 0))[1] for h in hashes]
    assert all((a == cs.rr.OK) == (f not in (cs.rr.ETAG, cs.rr.ERANGE)) for a, f in zip(auth, full))
    sel = [k % 3 != 1 for k in range(22)]
    part = cs.cr.data(cs.st.PRK, packs, hd, "full", sel)
    assert part == [f if s else cs.cr.SKIPPED for f, s in zip(full, sel)]
    flags, items, stats, _ = cs.cr.structure(hd, index)
    assert not any(flags) and not any(items)
    want_bad = sorted({cs.pref.flat_entries(hd)[e][0] for e, f in enumerate(full) if f})
    assert cs.cr.bad_packfiles(hd, flags, stats, full) == want_bad and len(want_bad) >= 2


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "backuwup_gpu.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %d %d %d %d\\n", sizeof(bw_check_packfile_stat),'
                   ' offsetof(bw_check_packfile_stat, tail), sizeof(bw_check_counts), offsetof(bw_check_counts, n_packfiles_clean),'
                   ' BW_CHECK_SKIPPED, BW_CHECK_IDUPLICATE, (int)BW_CHECK_AUTH, (int)BW_CHECK_FULL); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    from backuwup_amd import _lib, check
    assert vals == [ctypes.sizeof(_lib.BwCheckPackfileStat), _lib.BwCheckPackfileStat.tail.offset, ctypes.sizeof(_lib.BwCheckCounts),
                    _lib.BwCheckCounts.n_packfiles_clean.offset, _lib.BW_CHECK_SKIPPED, _lib.BW_CHECK_IDUPLICATE,
                    _lib.BW_CHECK_AUTH, _lib.BW_CHECK_FULL]
    assert check.STAT_DTYPE.itemsize == vals[0] and check.STAT_DTYPE.fields["tail"][1] == vals[1]
    assert [f for f, _ in _lib.BwCheckPackfileStat._fields_] == list(check.STAT_DTYPE.names)
    lib = _lib.load()
    for name in ("bw_auth_device", "bw_auth", "bw_check_structure", "bw_check_data"):
        assert hasattr(lib, name)
