"""The pattern compiler and the per-byte rule of find (backuwup_amd/csrc/bw_find_host.h) in the stand-alone
program tests/cpp/find_selftest.cpp, plain and under the address and undefined sanitizers.  Every expected
line below is worked out by hand from the header's state layout: a state per literal byte, '?', class and
run of '*', one per component end, one per run of '**' components, one in front of a floating pattern;
bit k of a state set is state k.  The kernel runs the same fd_step (tests/test_gpu_find.py)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

WANT = [
    # "*.jpg" floats: ** * . j p g end = 7 states; at a component start the '**', the '*' and the '.' are live
    "A jpg states=7 init=7 acc=40 star=2 dstar=1 cont=0 dir=0",
    "A 64 states=64 init=1 acc=8000000000000000 star=0 dstar=0 cont=0 dir=0",
    "A 65 refused: a pattern that needs 65 states (at most 64)",
    "A float64 states=64 init=3 acc=8000000000000000 star=0 dstar=1 cont=0 dir=0",
    "A float65 refused: a pattern that needs 65 states (at most 64)",
    # a * b end | ** | c end: the runs of '*' and of '**' are one state each
    "A runs states=7 init=1 acc=40 star=2 dstar=10 cont=0 dir=1",
    "A all states=1 init=1 acc=1 star=0 dstar=1 cont=0 dir=0",
    "R empty refused: an empty pattern",
    "R slash refused: an empty component",
    "R component refused: an empty component",
    "R class refused: an unterminated class",
    "R backslash refused: a dangling backslash",
    "R utf8 refused: a pattern that is not valid UTF-8",
    "R overlong refused: a pattern that is not valid UTF-8",
    "R member refused: a class member that is not ASCII",
    "R classslash refused: a '/' inside a class",
    "R escslash refused: an escaped '/'",
    "R range refused: a class range that runs backwards",
    # a ? end: the '?' takes the lead byte, the state behind it stays over the continuation bytes
    "T two 2 4 4 match=1 down=0",
    "T three 2 4 4 4 match=1 down=0",
    "T four 2 4 4 4 4 match=1 down=0",
    "T twice 2 4 4 0 0 match=0 down=0",
    "T neg 2 2 2 4 match=1 down=0",
    # a end ** b end: the '/' behind a enters the '**' (4) and passes it (8): zero components
    "T zero 2 c 14 match=1 down=c",
    "T one 2 c 4 c 14 match=1 down=c",
    "T mid 2 c 4 4 match=0 down=c",
    "T icase 2 4 match=1 down=0",
    "T case 0 0 match=0 down=0",
    "T float 7 7 7 f 17 27 47 match=1 down=7",
    "T last " + " ".join("%x" % (1 << k) for k in range(1, 64)) + " match=1 down=0",
    # a end **: the end of a accepts through the closing '**', which is what its children start in
    "T tail 2 match=1 down=4",
]


def run_selftest(tmp_path, extra=()):
    exe = tmp_path / ("find_selftest" + ("_san" if extra else ""))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-g", *extra, "-I", os.path.join(ROOT, "backuwup_amd", "csrc"),
                           os.path.join(HERE, "cpp", "find_selftest.cpp"), "-o", str(exe)], timeout=180)
    return [ln.rstrip() for ln in subprocess.check_output([str(exe)], timeout=60).decode().splitlines()]


def test_state_counts_refusals_and_step_traces(tmp_path):
    assert run_selftest(tmp_path) == WANT


def test_the_same_program_under_the_address_and_undefined_sanitizers(tmp_path):
    assert run_selftest(tmp_path, extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all")) == WANT
