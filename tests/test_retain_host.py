"""The host arithmetic of retain (backuwup_amd/csrc/bw_retain_host.h) in a stand-alone C++ program
(tests/cpp/retain_selftest.cpp), plain and under the address and undefined sanitizers: W, the place of a
root's bit, the valid bits of a word, the refusal of a bit of a root that was not given, the drop predicate
and the forward order of a sweep; then rt_valid and rt_foreign at 63, 64, 65, 4095 and 4096 roots (line G: n,
W, the last word's valid bits, the valid bits past it, then rt_foreign over three clean rows, with the top bit
of the last row's last word set, and with its lowest bit that no root has: where the word is full no bit is
foreign).  Every expected value below is worked out by hand.  The walk itself runs
in tests/test_gpu_retain.py."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

WANT = """
A 1 1 1 2 2 3 64
B 15 16 17 1 8000000000000000 2
C 0 1 7fffffffffffffff ffffffffffffffff 1 ffffffffffffffff
D -1 1 -1 0 1 2 -1
E 1 0 1 0 0 1 0
F empty 0
F range 0 5
F range 5 12
F range 12 13
F backward first 12
G 63 1 7fffffffffffffff 0 -1 2 2
G 64 1 ffffffffffffffff 0 -1 -1 -1
G 65 2 1 0 -1 2 2
G 4095 64 7fffffffffffffff 0 -1 2 2
G 4096 64 ffffffffffffffff 0 -1 -1 -1
""".strip().splitlines()


def run_host(tmp_path, extra=()):
    exe = tmp_path / ("retain_selftest" + ("_san" if extra else ""))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-g", *extra, "-I", os.path.join(ROOT, "backuwup_amd", "csrc"),
                           os.path.join(HERE, "cpp", "retain_selftest.cpp"), "-o", str(exe)], timeout=180)
    return [ln.rstrip() for ln in subprocess.check_output([str(exe)], timeout=60).decode().splitlines()]


def test_words_bits_foreign_check_predicate_and_sweep_order(tmp_path):
    assert run_host(tmp_path) == WANT


def test_the_same_program_under_the_address_and_undefined_sanitizers(tmp_path):
    assert run_host(tmp_path, extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all")) == WANT
