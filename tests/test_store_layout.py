"""The store's layout rules (backuwup_amd/csrc/bw_store_layout.h) without a device.

tests/cpp/store_layout_selftest.cpp includes only that header: blob_place, section_base and
store_extent against literals, rekey's items and gaps painted into a per-byte counter over seeded
small stores, and repack's tables against a serial restatement.  It is built with ASan + UBSan, as
tests/test_plan.py builds its program, and run as a program of its own (nothing here is threaded, so
there is no TSan build).
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "store_layout_selftest.cpp")
# the sanitizer runtimes are linked statically: the program runs in whatever environment the suite has
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("store_layout") / "store_layout_selftest_asan"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fno-omit-frame-pointer", "-g", "-O1"] + ASAN +
                          [SRC, "-lpthread", "-o", str(exe)])
    return str(exe)


def test_store_layout_under_asan_ubsan(asan_exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([asan_exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "store layout selftest ok" in r.stdout
