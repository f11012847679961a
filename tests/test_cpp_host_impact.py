"""The impact side of the C++ host mirror (backuwup_amd/host/backuwup.hpp: Impact) compiled against the
C ABI and run on the GPU (tests/cpp/host_impact.cpp).  The expected lines are worked out by hand from the
program's store: entries are chunks 0-3, a.bin 4 (chunks 0, 1), A's b.bin 5 (chunk 2), B's b.bin 6 (chunks
2, 3), new.bin 7 (chunk 2), A's sub 8, B's sub 9, root A 10 (a.bin, sub), root B 11 (a.bin, sub, new.bin)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(tmp_path):
    exe = tmp_path / "host_impact"
    libdir = os.path.join(ROOT, "backuwup_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "cpp", "host_impact.cpp"), "-L", libdir, "-lbackuwup_amd",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cpp_impact_mirror_compiles(tmp_path):
    assert build(tmp_path).exists()


@pytest.mark.gpu
def test_cpp_impact_mirror_matches(tmp_path):
    out = subprocess.check_output([str(build(tmp_path))], timeout=120).decode().splitlines()
    # mark: taint per entry | trees expanded, levels, edges, tainted, roots affected, errors | root_affected
    assert "clean mark 0 0 0 0 0 0 0 0 0 0 0 0 | 8 3 7 0 0 0 | 0 0" in out and "clean counts 0 0 0" in out
    assert not [ln for ln in out if ln.startswith("clean rec")] and "clean sweeps 1" in out
    # chunk 2 lost: the three files that name it, both subs and both roots are BELOW
    assert "chunk mark 0 0 1 0 0 2 2 2 2 2 2 2 | 8 3 7 8 2 0 | 1 1" in out
    # rec: root 'path' kind n_affected n_children first_affected flags
    assert sorted(ln for ln in out if ln.startswith("chunk rec")) == sorted([
        "chunk rec 0 '' 1 1 2 1 0", "chunk rec 0 'sub' 1 1 1 0 0", "chunk rec 0 'sub/b.bin' 0 1 1 0 0",
        "chunk rec 1 '' 1 2 3 1 0", "chunk rec 1 'sub' 1 1 1 0 0", "chunk rec 1 'new.bin' 0 1 1 0 0",
        "chunk rec 1 'sub/b.bin' 0 1 2 0 0"])
    assert "chunk root 0 3 1 0 1" in out and "chunk root 1 4 2 0 2" in out and "chunk counts 7 3 0" in out
    # B's sub lost: it is never opened, so its b.bin (6) and chunk 3 are reached by nobody; root A is sound
    assert "dir mark 0 0 0 0 0 0 0 0 0 1 0 2 | 6 3 6 2 1 0 | 0 1" in out
    assert sorted(ln for ln in out if ln.startswith("dir rec")) == ["dir rec 1 '' 1 1 3 1 0", "dir rec 1 '?' 0 0 0 -1 1"]
    assert "dir root 0 0 0 0 0" in out and "dir root 1 2 0 1 0" in out and "dir counts 2 2 0" in out
    # the one packfile lost: both roots are unreadable, nothing is opened
    assert "packfile 12" in out and "all mark 0 0 0 0 0 0 0 0 0 0 1 1 | 0 0 0 2 2 0 | 1 1" in out
    assert sorted(ln for ln in out if ln.startswith("all rec")) == ["all rec 0 '?' 0 0 0 -1 1", "all rec 1 '?' 0 0 0 -1 1"]
