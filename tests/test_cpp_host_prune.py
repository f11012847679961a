"""The prune side of the C++ host mirror (backuwup_amd/host/backuwup.hpp: Prune) compiled against the
C ABI and run on the GPU (tests/cpp/host_prune.cpp)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(tmp_path):
    exe = tmp_path / "host_prune"
    libdir = os.path.join(ROOT, "backuwup_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "cpp", "host_prune.cpp"), "-L", libdir, "-lbackuwup_amd",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cpp_prune_mirror_compiles(tmp_path):
    assert build(tmp_path).exists()


@pytest.mark.gpu
def test_cpp_prune_mirror_round_trip(tmp_path):
    out = subprocess.check_output([str(build(tmp_path))], timeout=120).decode().splitlines()
    assert "mark 0 7 8 4 1 16 1" in out    # no root: nothing live; 7 of 8 live, 4 trees, the absent root ENOTFOUND, the spare chunk dead
    assert "plan 7 1 1" in out
    assert "pruned 7 2 1 1 0 16" in out    # the kept root restores byte for byte; the dropped chunk is ENOTFOUND
    assert "again 0 0" in out              # no dead byte left, nothing to move
