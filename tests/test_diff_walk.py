"""The device diff walk's surface without a device: the export and its argument check, the layout of
bw_diff_record / bw_diff_counts in C against the ctypes structs and the numpy dtypes, and
diff.record_changes' path joining and sorting over a hand-made records array.  The walk itself runs in
tests/test_gpu_diff_walk.py; the C++ mirror compiles in tests/test_cpp_host_diff.py."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "backuwup_gpu.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
    printf("bw_diff_side %zu\n", sizeof(bw_diff_side));
    F(bw_diff_side, hash); F(bw_diff_side, kind); F(bw_diff_side, flags); F(bw_diff_side, size);
    F(bw_diff_side, mtime); F(bw_diff_side, ctime); F(bw_diff_side, n_children);
    printf("bw_diff_record %zu\n", sizeof(bw_diff_record));
    F(bw_diff_record, change); F(bw_diff_record, flags); F(bw_diff_record, parent); F(bw_diff_record, name_off);
    F(bw_diff_record, name_len); F(bw_diff_record, a); F(bw_diff_record, b); F(bw_diff_record, common_prefix);
    F(bw_diff_record, common_suffix); F(bw_diff_record, n_new);
    printf("bw_diff_counts %zu\n", sizeof(bw_diff_counts));
    F(bw_diff_counts, n_records); F(bw_diff_counts, name_bytes); F(bw_diff_counts, n_read);
    F(bw_diff_counts, n_levels); F(bw_diff_counts, n_errors);
    printf("consts %d %d %d %d %u %u\n", BW_DIFF_ADDED, BW_DIFF_REMOVED, BW_DIFF_MODIFIED, BW_DIFF_TYPE_CHANGED,
           BW_DIFF_UNREADABLE, BW_DIFF_TRUNCATED);
    return 0;
}
"""


def test_the_library_exports_bw_diff_trees_and_refuses_null_arguments():
    from backuwup_amd import _lib
    L = _lib.load()
    assert "bw_diff_trees" in [s[0] for s in _lib.SIGNATURES]
    cnt = _lib.BwDiffCounts()
    assert L.bw_diff_trees(None, None, None, 0, None, 0, None, 0, None, None, None, 0) == _lib.BW_EINVAL
    assert L.bw_diff_trees(None, None, None, 0, None, 0, None, 0, None, ctypes.byref(cnt), None, 0) == _lib.BW_EINVAL


def test_record_and_counts_layout_in_c_ctypes_and_numpy(tmp_path):
    from backuwup_amd import _lib, diff
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        key, *vals = line.split()
        got[key] = [int(v) for v in vals]
    structs = {"bw_diff_side": (_lib.BwDiffSide, diff.SIDE_DTYPE), "bw_diff_record": (_lib.BwDiffRecord, diff.RECORD_DTYPE),
               "bw_diff_counts": (_lib.BwDiffCounts, None)}
    n_fields = 0
    for name, (ct, dt) in structs.items():
        assert got[name] == [ctypes.sizeof(ct)]
        assert dt is None or dt.itemsize == ctypes.sizeof(ct)
        for f, _ in ct._fields_:
            assert got["%s.%s" % (name, f)] == [getattr(ct, f).offset], (name, f)
            assert dt is None or dt.fields[f][1] == getattr(ct, f).offset, (name, f)
            n_fields += 1
    assert n_fields == 7 + 10 + 5 and (got["bw_diff_side"], got["bw_diff_record"], got["bw_diff_counts"]) == ([72], [200], [40])
    assert got["consts"] == [diff.ADDED, diff.REMOVED, diff.MODIFIED, diff.TYPE_CHANGED, diff.F_UNREADABLE, diff.F_TRUNCATED]


SIZING_CPP = r"""
#include <cstdio>
#include "bw_diff_host.h"
int main() {
    const unsigned long long ns[] = {0, 1, 32, 33, 300, (1ull << 30) - 1, 1ull << 30, (1ull << 30) + 1, (1ull << 31) - 1,
                                     1ull << 40};
    for (unsigned long long n : ns) std::printf("%llu %u\n", n, bw::df_table_cap(n));
    std::printf("max %llu\n", (unsigned long long)bw::DF_MAX_ROWS);
    return 0;
}
"""


def test_table_capacity_is_a_power_of_two_that_ends_within_32_bits(tmp_path):
    """The name and row tables hold twice their keys.  Up to the level limit of 2^30 keys the capacity is
    a power of two >= 2 n that fits 32 bits; past it the count still ends (a u32 doubled past 2^31 is 0,
    and a loop on it would not)."""
    src = tmp_path / "sizing.cpp"
    src.write_text(SIZING_CPP)
    exe = tmp_path / "sizing"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "backuwup_amd", "csrc"), str(src), "-o", str(exe)],
                          timeout=120)
    lines = subprocess.check_output([str(exe)], timeout=20).decode().splitlines()
    assert lines[-1] == "max %d" % (1 << 30)
    got = {int(a): int(b) for a, b in (ln.split() for ln in lines[:-1])}
    assert got[0] == got[1] == got[32] == 64 and got[33] == 128 and got[300] == 1024
    for n, cap in got.items():
        assert cap & (cap - 1) == 0 and 64 <= cap <= 1 << 31
        if n <= 1 << 30:
            assert cap >= 2 * n and (cap == 64 or cap < 4 * n)
    assert got[(1 << 30) - 1] == got[1 << 30] == 1 << 31 and got[1 << 40] == 1 << 31


def test_record_changes_joins_paths_through_parent_and_sorts_them():
    from backuwup_amd import diff
    NONE = 2**64 - 1
    names = b"zeta" + b"alpha" + b"in" + b"\xff\xfe"
    # (change, flags, parent, name_off, name_len); records of a level in no particular order
    rows = [(diff.MODIFIED, 0, NONE, 0, 0),                 # 0: the root, path ''
            (diff.MODIFIED, 0, 0, 0, 4),                    # 1: zeta
            (diff.TYPE_CHANGED, diff.F_TRUNCATED, 0, 4, 5),  # 2: alpha
            (diff.ADDED, 0, 1, 9, 2),                       # 3: zeta/in
            (diff.REMOVED, 0, 2, 9, 2),                     # 4: alpha/in
            (diff.ADDED, diff.F_UNREADABLE, 2, 0, 0),       # 5: alpha/?<hash of B>
            (diff.ADDED, 0, 2, 11, 2),                      # 6: a name that is not UTF-8
            (diff.ADDED, 0, 2, 9, 2)]                       # 7: alpha/in again, ADDED: sorts before the REMOVED one
    rec = np.zeros(len(rows), dtype=diff.RECORD_DTYPE)
    for i, (change, flags, parent, off, ln) in enumerate(rows):
        rec[i]["change"], rec[i]["flags"], rec[i]["parent"], rec[i]["name_off"], rec[i]["name_len"] = change, flags, parent, off, ln
        rec[i]["a"]["hash"], rec[i]["b"]["hash"] = 0xA0 + i, 0xB0 + i
        rec[i]["b"]["size"], rec[i]["a"]["n_children"] = 100 + i, i
        rec[i]["common_prefix"], rec[i]["common_suffix"], rec[i]["n_new"] = i, 2 * i, 3 * i
    out = diff.record_changes(rec, names)
    bad = b"\xff\xfe".decode("utf-8", "surrogateescape")
    assert [(c["path"], c["change"]) for c in out] == [
        ("", diff.MODIFIED), ("alpha", diff.TYPE_CHANGED), ("alpha/?" + (bytes([0xB5]) * 32).hex(), diff.ADDED),
        ("alpha/in", diff.ADDED), ("alpha/in", diff.REMOVED), ("alpha/" + bad, diff.ADDED), ("zeta", diff.MODIFIED),
        ("zeta/in", diff.ADDED)]
    alpha, added, removed = out[1], out[3], out[4]
    assert alpha["flags"] == diff.F_TRUNCATED and alpha["hash_a"] == bytes([0xA2]) * 32 and alpha["hash_b"] == bytes([0xB2]) * 32
    assert alpha["a"] == dict(kind=0, flags=0, size=0, mtime=0, ctime=0, n_children=2) and alpha["b"]["size"] == 102
    assert (alpha["common_prefix"], alpha["common_suffix"], alpha["n_new"]) == (2, 4, 6)
    assert added["a"] is None and added["hash_a"] is None and added["b"]["size"] == 107
    assert removed["b"] is None and removed["hash_b"] is None and removed["hash_a"] == bytes([0xA4]) * 32
    assert diff.record_changes(rec[:0], b"") == []
