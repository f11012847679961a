"""The check side of the C++ host mirror (backuwup_amd/host/backuwup.hpp: Check) compiled against the
C ABI and run on the GPU (tests/cpp/host_check.cpp)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(tmp_path):
    exe = tmp_path / "host_check"
    libdir = os.path.join(ROOT, "backuwup_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "cpp", "host_check.cpp"), "-L", libdir, "-lbackuwup_amd",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cpp_check_mirror_compiles(tmp_path):
    assert build(tmp_path).exists()


@pytest.mark.gpu
def test_cpp_check_mirror_round_trip(tmp_path):
    out = subprocess.check_output([str(build(tmp_path))], timeout=120).decode().splitlines()
    assert "structure 7 0 0 0 0 7 1 0" in out   # seven entries, no flag, seven items OK, the packfile clean, no tail
    assert "data 7 7" in out                    # every tag verifies; every blob decodes, hashes to its name and parses
    # entry 0 lost its item (BW_CHECK_E_UNINDEXED = 4); the flipped tag byte is BW_UNPACK_ETAG (1) in both modes, at
    # the last entry; the unselected entry is skipped
    assert "damaged 4 1 6 1 1 1 1 1" in out
    assert "auth 1 0 1" in out                  # the flipped ciphertext bit fails; the empty item verifies
