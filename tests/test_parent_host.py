"""The parent match's host-only rules (backuwup_amd/csrc/bw_parent_host.h) in a stand-alone C++ program: the
scan validation, every refused form and the valid edge forms, and the table sizing.  Also the export's
argument check and the layout of bw_parent_result / bw_parent_counts in C against ctypes and numpy.  The
walk itself runs in tests/test_gpu_parent_match.py."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

HOST_CPP = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "bw_parent_host.h"
using namespace bw;
static bw_restore_node node(uint32_t kind, uint64_t first, uint64_t count, uint64_t off, uint64_t len) {
    bw_restore_node n;
    memset(&n, 0, sizeof(n));
    n.kind = kind; n.child_first = first; n.n_children = count; n.name_off = off; n.name_len = len;
    return n;
}
// root {d {f, g}, e {h}, top}: names "" d e top f g h
static std::vector<bw_restore_node> good() {
    return {node(1, 1, 3, 0, 0), node(1, 4, 2, 0, 1), node(1, 6, 1, 1, 1), node(0, 0, 0, 2, 3),
            node(0, 0, 0, 5, 1), node(0, 0, 0, 6, 1), node(0, 0, 0, 7, 1)};
}
static void say(const char* what, const std::vector<bw_restore_node>& s, uint64_t names_len) {
    std::printf("%s %llu\n", what, (unsigned long long)pm_scan_invalid(s.data(), s.size(), names_len));
}
int main() {
    std::vector<bw_restore_node> s = good();
    say("good", s, 8);
    s = good(); s[3].kind = 2; say("kind", s, 8);
    s = good(); s[3].n_children = 1; say("file_with_children", s, 8);
    s = good(); s[1].child_first = 1; say("child_first_is_itself", s, 8);
    s = good(); s[2].child_first = 0; say("child_first_before", s, 8);
    s = good(); s[2].n_children = 2; say("range_past_end", s, 8);
    s = good(); s[2].child_first = 8; say("first_past_end", s, 8);
    s = good(); s[2].child_first = 5; say("overlap", s, 8);
    s = good(); s[1].child_first = 6; s[1].n_children = 1; s[2].child_first = 4; s[2].n_children = 2; say("descending_ranges", s, 8);
    s = good(); s[0].child_first = 0; say("root_names_itself", s, 8);
    s = good(); s[6].name_len = 2; say("name_past_arena", s, 8);
    s = good(); s[6].name_off = 9; s[6].name_len = 0; say("name_off_past_arena", s, 8);
    s = good(); s[6].name_off = ~0ull; s[6].name_len = 2; say("name_wraps", s, 8);
    s = good(); s[2].n_children = ~0ull; say("count_wraps", s, 8);
    // the valid edge forms
    s = {node(1, 0, 0, 0, 0)}; say("single_dir", s, 0);
    s = {node(0, 0, 0, 0, 0)}; say("single_file", s, 0);
    s = {node(1, 1, 1, 0, 0), node(1, 77, 0, 0, 0)}; say("empty_dir", s, 0);
    s = {node(1, 1, 2, 0, 0), node(0, 0, 0, 0, 0), node(0, 0, 0, 0, 0)}; say("empty_names", s, 0);
    s = good(); s[6].name_off = 8; s[6].name_len = 0; say("empty_name_at_the_end", s, 8);
    s = good(); s[3].child_first = 5; say("file_child_first_ignored", s, 8);
    s = good(); s.push_back(node(0, 0, 0, 0, 0)); say("unnamed_node", s, 8);
    const unsigned long long ns[] = {0, 1, 32, 33, 300, 10001, 1ull << 30, (1ull << 30) + 1};
    for (unsigned long long n : ns) std::printf("cap %llu %u\n", n, pm_table_cap(n));
    std::printf("max %llu\n", (unsigned long long)PM_MAX_ROWS);
    return 0;
}
"""

INVALID = {"kind": 4, "file_with_children": 4, "child_first_is_itself": 2, "child_first_before": 3, "range_past_end": 3,
           "first_past_end": 3, "overlap": 3, "root_names_itself": 1, "name_past_arena": 7, "name_off_past_arena": 7,
           "name_wraps": 7, "count_wraps": 3}
VALID = ("good", "descending_ranges", "single_dir", "single_file", "empty_dir", "empty_names", "empty_name_at_the_end",
         "file_child_first_ignored", "unnamed_node")


def run_host(tmp_path, extra=()):
    src = tmp_path / "parent_host.cpp"
    src.write_text(HOST_CPP)
    exe = tmp_path / ("parent_host" + ("_san" if extra else ""))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-g", *extra, "-I", os.path.join(ROOT, "backuwup_amd", "csrc"), str(src),
                           "-o", str(exe)], timeout=180)
    return subprocess.check_output([str(exe)], timeout=60).decode().splitlines()


def check_lines(lines):
    got = {ln.split()[0]: int(ln.split()[1]) for ln in lines if not ln.startswith("cap ")}
    for what, at in INVALID.items():            # 1 + the node that breaks the rule
        assert got[what] == at, what
    for what in VALID:
        assert got[what] == 0, what
    assert got["max"] == 1 << 30
    caps = {int(ln.split()[1]): int(ln.split()[2]) for ln in lines if ln.startswith("cap ")}
    assert caps[0] == caps[1] == caps[32] == 64 and caps[33] == 128 and caps[300] == 1024 and caps[10001] == 32768
    assert caps[1 << 30] == caps[(1 << 30) + 1] == 1 << 31
    for n, cap in caps.items():
        assert cap & (cap - 1) == 0 and (n > 1 << 30 or cap >= 2 * n)


def test_scan_validation_and_table_sizing(tmp_path):
    check_lines(run_host(tmp_path))


def test_the_same_program_under_the_address_and_undefined_sanitizers(tmp_path):
    check_lines(run_host(tmp_path, extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all")))


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "backuwup_gpu.h"
#include "backuwup_gpu_pack.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
    printf("bw_parent_result %zu\n", sizeof(bw_parent_result));
    F(bw_parent_result, hash); F(bw_parent_result, status); F(bw_parent_result, pad);
    printf("bw_parent_counts %zu\n", sizeof(bw_parent_counts));
    F(bw_parent_counts, n_read); F(bw_parent_counts, n_levels); F(bw_parent_counts, n_errors);
    F(bw_parent_counts, n_unchanged); F(bw_parent_counts, unchanged_bytes);
    printf("consts %d %d %d %d %d %d\n", BW_PARENT_NEW, BW_PARENT_UNCHANGED, BW_PARENT_CHANGED, BW_PARENT_RACY,
           BW_PARENT_DIR, BW_PARENT_TYPE_CHANGED);
    return 0;
}
"""


def test_result_and_counts_layout_in_c_ctypes_and_numpy(tmp_path):
    from backuwup_amd import _lib, parent
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        key, *vals = line.split()
        got[key] = [int(v) for v in vals]
    for name, ct, dt in (("bw_parent_result", _lib.BwParentResult, parent.RESULT_DTYPE), ("bw_parent_counts", _lib.BwParentCounts, None)):
        assert got[name] == [ctypes.sizeof(ct)]
        for f, _ in ct._fields_:
            assert got["%s.%s" % (name, f)] == [getattr(ct, f).offset], (name, f)
            assert dt is None or dt.fields[f][1] == getattr(ct, f).offset
    assert got["consts"] == [parent.NEW, parent.UNCHANGED, parent.CHANGED, parent.RACY, parent.DIR, parent.TYPE_CHANGED]


def test_the_library_exports_bw_parent_match_and_refuses_null_arguments():
    from backuwup_amd import _lib
    L = _lib.load()
    assert "bw_parent_match" in [s[0] for s in _lib.SIGNATURES]
    cnt = _lib.BwParentCounts()
    assert L.bw_parent_match(None, None, 0, 0, None, 0, None, 0, None, None, ctypes.byref(cnt), None, 0) == _lib.BW_EINVAL
