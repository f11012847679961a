"""The diff side of the C++ host mirror (backuwup_amd/host/backuwup.hpp: Diff) compiled against the
C ABI and run on the GPU (tests/cpp/host_diff.cpp)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(tmp_path):
    exe = tmp_path / "host_diff"
    libdir = os.path.join(ROOT, "backuwup_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "cpp", "host_diff.cpp"), "-L", libdir, "-lbackuwup_amd",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cpp_diff_mirror_compiles(tmp_path):
    assert build(tmp_path).exists()


@pytest.mark.gpu
def test_cpp_diff_mirror_walks(tmp_path):
    out = subprocess.check_output([str(build(tmp_path))], timeout=120).decode().splitlines()
    assert "diff 4 3 7 0 1" in out          # "", sub, sub/b.bin, new.bin; both roots, both subs, both b.bin, new.bin read
    assert "at '' 3 1 0 2" in out           # the root: a.bin stays in front, sub and new.bin are new rows
    assert "at 'sub' 3 0 0 1" in out
    assert "at 'sub/b.bin' 3 1 0 1" in out  # one chunk appended
    assert "at 'new.bin' 1 0 0 0" in out
    assert "same 0 0 0 0" in out
    assert "lost 5 1 4 1 16" in out         # the absent root: ENOTFOUND, an unreadable ADDED record, A's four nodes REMOVED
