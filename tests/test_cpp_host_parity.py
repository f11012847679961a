"""The parity side of the C++ host mirror (backuwup_amd/host/backuwup.hpp: Parity) compiled against the
C ABI and run on the GPU (tests/cpp/host_parity_shards.cpp; tests/cpp/host_parity.cpp is the older
program of tests/test_cpp_host.py, about agreement with the oracle)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(tmp_path):
    exe = tmp_path / "host_parity_shards"
    libdir = os.path.join(ROOT, "backuwup_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "cpp", "host_parity_shards.cpp"), "-L", libdir, "-lbackuwup_amd",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cpp_parity_mirror_compiles(tmp_path):
    assert build(tmp_path).exists()


@pytest.mark.gpu
def test_cpp_parity_mirror_protects_and_repairs(tmp_path):
    out = subprocess.check_output([str(build(tmp_path))], timeout=120).decode().splitlines()
    assert "plan 2 14240 2 2 5008" in out   # groups of 3 and 2; shard lengths 5008 and 2112, two parity shards each
    assert "digests 1" in out
    assert "repair 2 0 1 0 0  1 1" in out   # packfile 0 rebuilt, packfile 2 damaged and rebuilt, both equal to the originals
    assert "nodigest 2 1" in out            # without digests the flipped byte goes through: one byte of packfile 0 differs
    assert "lost 4 4 4 4 0  1" in out       # two gone and the damaged one: nothing to rebuild from, and solve says BW_ETOOFEW
    assert "solve 1 2 3  0 4  6" in out
    assert "matmul 1" in out
