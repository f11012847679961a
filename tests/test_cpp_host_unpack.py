"""The read side of the C++ host mirror (backuwup_amd/host/backuwup.hpp: unpack_headers, unpack_blobs,
zstd_decompress) compiled against the C ABI and run on the GPU (tests/cpp/host_unpack.cpp)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(tmp_path):
    exe = tmp_path / "host_unpack"
    libdir = os.path.join(ROOT, "backuwup_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "cpp", "host_unpack.cpp"), "-L", libdir, "-lbackuwup_amd",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cpp_unpack_mirror_compiles(tmp_path):
    assert build(tmp_path).exists()


@pytest.mark.gpu
def test_cpp_unpack_mirror_round_trip(tmp_path):
    out = subprocess.check_output([str(build(tmp_path))], timeout=120).decode().splitlines()
    unpack = [l.split() for l in out if l.startswith("unpack ")][0]
    assert int(unpack[1]) >= 1 and unpack[2:] == ["5", "5", "5"]
    assert "damaged 0 1 0 0 0" in out      # BW_UNPACK_ETAG for the damaged blob alone
    assert "frames 1 0 hello" in out
