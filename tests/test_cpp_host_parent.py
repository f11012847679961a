"""The parent match side of the C++ host mirror (backuwup_amd/host/backuwup.hpp: ParentMatch) compiled
against the C ABI and run on the GPU (tests/cpp/host_parent.cpp)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(tmp_path):
    exe = tmp_path / "host_parent"
    libdir = os.path.join(ROOT, "backuwup_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "cpp", "host_parent.cpp"), "-L", libdir, "-lbackuwup_amd",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cpp_parent_mirror_compiles(tmp_path):
    assert build(tmp_path).exists()


@pytest.mark.gpu
def test_cpp_parent_mirror_matches(tmp_path):
    out = subprocess.check_output([str(build(tmp_path))], timeout=120).decode().splitlines()
    # scan nodes: "", a.bin, sub, new.bin, sub/b.bin; statuses NEW 0, UNCHANGED 1, CHANGED 2, RACY 3, DIR 4
    assert "same 4 1 4 1 1 | 2 5 3 5296 0 1" in out     # B against itself: both Dirs and the three Files read
    assert "hash 1 1" in out                            # the root's hash, and a.bin's tree blob's
    assert "racy 4 1 4 3 3 | 2 5 1 2037 0 1" in out     # mtimes at or past trust_before are not trusted
    assert "older 4 1 4 0 2 | 2 4 1 2037 0 1" in out    # against A: new.bin is new, b.bin changed
    assert "none 0 0 0 0 0 | 0 0 0 0 0 1" in out
    assert "lost 0 0 0 0 0 | 1 0 0 0 1 1" in out and "reason 16" in out
