"""The restore side of the C++ host mirror (backuwup_amd/host/backuwup.hpp: Restore) compiled against the
C ABI and run on the GPU (tests/cpp/host_restore.cpp)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(tmp_path):
    exe = tmp_path / "host_restore"
    libdir = os.path.join(ROOT, "backuwup_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "cpp", "host_restore.cpp"), "-L", libdir, "-lbackuwup_amd",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cpp_restore_mirror_compiles(tmp_path):
    assert build(tmp_path).exists()


@pytest.mark.gpu
def test_cpp_restore_mirror_round_trip(tmp_path):
    out = subprocess.check_output([str(build(tmp_path))], timeout=120).decode().splitlines()
    assert "locate 0 16" in out                                   # BW_RESTORE_OK, BW_RESTORE_ENOTFOUND
    assert "walk 4 a.bin sub b.bin" in out                        # the root, its children, then sub's
    assert out.count("files 2 a.bin 1 1 1500000000 sub/b.bin 1") == 2  # a large window and one below a file's size
    assert "refused 19 1" in out                                  # BW_RESTORE_ENOTTREE for a chunk's hash
