"""The rekey side of the C++ host mirror (backuwup_amd/host/backuwup.hpp: Rekey) compiled against the
C ABI and run on the GPU (tests/cpp/host_rekey.cpp)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(tmp_path):
    exe = tmp_path / "host_rekey"
    libdir = os.path.join(ROOT, "backuwup_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "cpp", "host_rekey.cpp"), "-L", libdir, "-lbackuwup_amd",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cpp_rekey_mirror_compiles(tmp_path):
    assert build(tmp_path).exists()


@pytest.mark.gpu
def test_cpp_rekey_mirror_round_trip(tmp_path):
    out = subprocess.check_output([str(build(tmp_path))], timeout=120).decode().splitlines()
    assert "store 7 7 1 1" in out        # seven entries and the header authentic; the bytes are the store packed under the new PRK
    assert "after 7 7 7 0" in out        # under the new PRK every tag verifies and every blob decodes; under the old one none
    assert "damaged 1 1 1 1" in out      # the damaged blob is BW_UNPACK_ETAG (1) when rekeyed and when authenticated afterwards
    assert "reseal 1 0 1  1 0 1  1" in out
