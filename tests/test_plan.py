"""The batch plan (backuwup_amd/csrc/bw_plan.h) without a device.

tests/cpp/plan_selftest.cpp includes only that header and compares its two-pass, 64-range tables and
every plan field with one serial walk; it is built once with ASan + UBSan and once with TSan (the
parallel fill is the only threaded code on the submit path) and run as a program of its own.  Its
`model` mode prints the geometry of a file list, which pins tests/cdc_chain_plant.py's seg_len_for
and segment model to the C++ plan at both segment lengths.
"""
import os
import subprocess

import numpy as np
import pytest

import cdc_chain_plant as cc
import cdc_plant as cp

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "plan_selftest.cpp")
# the sanitizer runtimes are linked statically: the programs run in whatever environment the suite has
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
TSAN = ["-fsanitize=thread", "-static-libtsan"]


def build(tmp_path, name, san):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fno-omit-frame-pointer", "-g", "-O1"] + san +
                          [SRC, "-lpthread", "-o", str(exe)])
    return str(exe)


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("plan"), "plan_selftest_asan", ASAN)


def test_plan_under_asan_ubsan(asan_exe):
    assert "plan selftest ok" in run(asan_exe)


def test_plan_under_tsan(tmp_path):
    assert "plan selftest ok" in run(build(tmp_path, "plan_selftest_tsan", TSAN))


@pytest.mark.parametrize("params", [cp.P1, cp.P3, cc.PF], ids=["P1", "P3", "PF"])
@pytest.mark.parametrize("small_batch", [True, False], ids=["small", "large"])
def test_python_model_matches_the_plan(oracle, asan_exe, params, small_batch):
    """seg_bytes, segments and cdc_files of the same file list from the C++ plan and from the Python
    model (Model.resolve over files of one constant byte that passes no mask: only the geometry is
    of interest here)."""
    L = cc.seg_len_for(params, small_batch)
    threshold = 300
    lens = [0, threshold, threshold + 1, L - 1, 5, L + 1]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    gear = cp.Gear.of(oracle, params)
    data = np.full(sum(lens), cc.constant_byte(gear), dtype=np.uint8)
    want = cc.Model(gear, data, params).resolve(offs, lens, threshold, small_batch)
    out = run(asan_exe, "model", *params, threshold, int(small_batch), *lens).split()
    got = dict(zip(out[0::2], (int(x) for x in out[1::2])))
    assert got == dict(seg_bytes=L, segments=want["segments"], cdc_files=want["cdc_files"])
    assert want["seg_bytes"] == L and want["cdc_files"] == 3 and want["segments"] == 1 + 1 + 2
