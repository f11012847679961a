"""The find side of the C++ host mirror (backuwup_amd/host/backuwup.hpp: Find) compiled against the C ABI
and run on the GPU (tests/cpp/host_find.cpp).  The expected lines are worked out by hand from the program's
store, which is host_impact.cpp's: root A holds a.bin (2037 bytes) and sub/b.bin (1074), root B the same a.bin,
sub/b.bin (2185) and new.bin (1074, one chunk).  Records come level after level: the roots 0-1, A's two and
B's three children 2-6, the two b.bin 7-8."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(tmp_path):
    exe = tmp_path / "host_find"
    libdir = os.path.join(ROOT, "backuwup_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "cpp", "host_find.cpp"), "-L", libdir, "-lbackuwup_amd",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cpp_find_mirror_compiles(tmp_path):
    assert build(tmp_path).exists()


@pytest.mark.gpu
def test_cpp_find_mirror_matches(tmp_path):
    out = subprocess.check_output([str(build(tmp_path))], timeout=120).decode().splitlines()
    # rec: root 'path' kind patterns flags child_first n_children
    assert [ln for ln in out if ln.startswith("float rec")] == [
        "float rec 0 '' 1 0 0 2 2", "float rec 1 '' 1 0 0 4 3", "float rec 0 'a.bin' 0 1 1 0 0", "float rec 0 'sub' 1 0 0 7 1",
        "float rec 1 'a.bin' 0 1 1 0 0", "float rec 1 'sub' 1 0 0 8 1", "float rec 1 'new.bin' 0 1 1 0 0",
        "float rec 0 'sub/b.bin' 0 1 1 0 0", "float rec 1 'sub/b.bin' 0 1 1 0 0"]
    # root: records, hits, hit files, hit bytes, unreadable; counts: records, levels, opened, pruned, chunk rows, errors
    assert "float root 0 4 2 2 3111 0" in out and "float root 1 5 3 3 5296 0" in out
    assert "float counts 9 3 13 0 0 0" in out  # 9 first pieces, and the chains of the two roots and the two subs
    # anchored: both subs are PRUNED (16) and never descended; new.bin's one chunk row comes back
    assert [ln for ln in out if ln.startswith("anchored rec")] == [
        "anchored rec 0 '' 1 0 0 2 2", "anchored rec 1 '' 1 0 0 4 3", "anchored rec 0 'a.bin' 0 0 0 0 0",
        "anchored rec 0 'sub' 1 0 16 0 0", "anchored rec 1 'a.bin' 0 0 0 0 0", "anchored rec 1 'sub' 1 0 16 0 0",
        "anchored rec 1 'new.bin' 0 1 1 0 1"]
    assert "anchored root 0 3 0 0 0 0" in out and "anchored root 1 4 1 1 1074 0" in out
    assert "anchored counts 7 2 10 2 1 0" in out and "anchored chunk 1" in out
    # "/SUB/" folded, directories only, with SUBTREE: the subs and what lies below them
    assert [ln for ln in out if ln.startswith("icase rec")] == [
        "icase rec 0 '' 1 0 0 2 2", "icase rec 1 '' 1 0 0 4 3", "icase rec 0 'a.bin' 0 0 0 0 0", "icase rec 0 'sub' 1 1 1 7 1",
        "icase rec 1 'a.bin' 0 0 0 0 0", "icase rec 1 'sub' 1 1 1 8 1", "icase rec 1 'new.bin' 0 0 0 0 0",
        "icase rec 0 'sub/b.bin' 0 1 1 0 0", "icase rec 1 'sub/b.bin' 0 1 1 0 0"]
    assert "icase root 0 4 2 1 1074 0" in out and "icase root 1 5 2 1 2185 0" in out and "icase counts 9 3 13 0 0 0" in out
