"""The retain side of the C++ host mirror (backuwup_amd/host/backuwup.hpp: Retain) compiled against the C
ABI and run on the GPU (tests/cpp/host_retain.cpp).  The expected lines are worked out by hand from the
program's store: entries are chunks 0-3, a.bin 4 (chunks 0, 1), A's b.bin 5 (chunk 2), B's b.bin 6 (chunks
2, 3), new.bin 7 (chunk 2), A's sub 8, B's sub 9, root A 10 (a.bin, sub), root B 11 (a.bin, sub, new.bin)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(tmp_path):
    exe = tmp_path / "host_retain"
    libdir = os.path.join(ROOT, "backuwup_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "cpp", "host_retain.cpp"), "-L", libdir, "-lbackuwup_amd",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cpp_retain_mirror_compiles(tmp_path):
    assert build(tmp_path).exists()


@pytest.mark.gpu
def test_cpp_retain_mirror_matches(tmp_path):
    out = subprocess.check_output([str(build(tmp_path))], timeout=120).decode().splitlines()
    # masks per entry | trees expanded, levels, edges (2 + 3 of the roots, 2 of a.bin, 1 + 1 of the subs, 1 + 2 of the
    # b.bins, 1 of new.bin), sweeps >= 1, errors | reached, orphans
    assert "ab masks 3 3 3 2 3 1 2 2 1 2 1 2 | 8 3 13 1 0 | 12 0" in out
    # root: reached, unique, damaged, status, complete, the bytes add up
    assert "ab root 0 7 3 0 0 1 1" in out and "ab root 1 9 5 0 0 1 1" in out
    # drop: freed, live, the bytes add up, live and stats are bw_prune_mark's over the kept roots
    assert [ln for ln in out if ln.startswith("ab drop")] == [
        "ab drop 0 freed 0 live 12 bytes 1 prune 1", "ab drop 1 freed 3 live 9 bytes 1 prune 1",
        "ab drop 2 freed 5 live 7 bytes 1 prune 1", "ab drop 3 freed 12 live 0 bytes 1 prune 1"]
    # B twice: each of its bits alone frees nothing, and nothing is B's alone
    assert "bab masks 7 7 7 5 7 2 5 5 2 5 2 5 | 8 3 13 1 0 | 12 0" in out
    assert "bab root 0 9 0 0 0 1 1" in out and "bab root 1 7 3 0 0 1 1" in out and "bab root 2 9 0 0 0 1 1" in out
    assert [ln for ln in out if ln.startswith("bab drop")] == [
        "bab drop 0 freed 0 live 12 bytes 1 prune 1", "bab drop 1 freed 5 live 7 bytes 1 prune 1",
        "bab drop 2 freed 3 live 9 bytes 1 prune 1"]
