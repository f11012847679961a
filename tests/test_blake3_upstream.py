"""BLAKE3 pinned to upstream: tests/golden/blake3_upstream.json holds the digests that the upstream C
implementation (tests/blake3_upstream.py: llvm_blake3_* inside ROCm's LLVM, written by nobody here)
gives for the cases of tests/blake3_cases.py.  The oracle (scalar and SIMD), the pure-Python
restatement and every BLAKE3 digest committed earlier are checked against it here; the device paths
in tests/test_gpu_blake3_upstream.py.  Where the library is present (a build host) the fixture is
also recomputed; only the tests that need the live library skip without it."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

import blake3_cases as cases
import blake3_upstream as up
from backuwup_amd.synth import splitmix_bytes, tree_corpus

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "blake3_upstream.json")))
A5_DIGEST = "288bba07c57e7334145f6905c58d864d9ce21618c6dadef35a7a25bb48c1c3a7"


def _live():
    if not up.available():
        pytest.skip("no library exporting llvm_blake3_hasher_init under the ROCm root")
    return up


@pytest.fixture(scope="module")
def groups():
    """(source, [(off, n)], [digest]) per group; the sources are what the generator hashed."""
    out = {}
    for g, src, cs in (("small", cases.small_source(), cases.small_cases()),
                       ("tree", cases.tree_source(), cases.tree_cases())):
        assert hashlib.sha256(src.tobytes()).hexdigest() == FIX["sources"][g]["sha256"], g
        assert FIX["sources"][g]["cases"] == len(cs), g
        src.setflags(write=False)
        out[g] = (src, cs, cases.digests(FIX, g))
    return out


def test_fixture_shape():
    assert os.path.getsize(os.path.join(HERE, "golden", "blake3_upstream.json")) < 160 << 10
    assert len(cases.SMALL_LENS) == 410 and len(cases.small_cases()) == 1640
    assert cases.small_cases()[:410] == [(0, n) for n in cases.SMALL_LENS]  # the offset-0 cases lead
    assert cases.tree_cases()[-1] == (3, (3 << 20) + 1)
    assert bytes.fromhex(FIX["small"][:64]).hex() == up.KAT[b""]  # case 0 is the empty message


def test_fixture_is_what_upstream_computes(groups):
    u = _live()
    assert FIX["blake3_version"] == u.version()
    for g, (src, cs, want) in groups.items():
        for (off, n), d in zip(cs, want):
            assert u.hash(src[off:off + n]) == d, (g, off, n)
    print("upstream BLAKE3 %s (%s)" % (u.version(), u.path()))


@pytest.mark.parametrize("impl", ["scalar", "simd"])
def test_oracle_equals_fixture(oracle, groups, impl):
    if impl == "simd" and not oracle.simd_available():
        pytest.skip("no AVX-512 on this host (the baseline falls back to the scalar restatement)")
    fn = oracle.blake3 if impl == "scalar" else oracle.blake3_fast
    for g, (src, cs, want) in groups.items():
        for (off, n), d in zip(cs, want):
            assert fn(src[off:off + n]) == d, (g, off, n)


def test_python_restatement_equals_fixture(groups):
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    src, cs, want = groups["small"]
    raw = src.tobytes()
    assert mg.splitmix(cases.SMALL_SEED, 4200) == raw[:4200]  # its own generator gives the same source
    ran = 0
    for (off, n), d in zip(cs, want):
        if off == 0 and n <= 4097:
            assert mg.blake3_py(raw[:n]) == d, n
            ran += 1
    assert ran == sum(1 for n in cases.SMALL_LENS if n <= 4097) > 150


def test_committed_digests_are_upstream():
    u = _live()
    vec = json.load(open(os.path.join(HERE, "golden", "vectors.json")))
    assert len(vec["blake3"]) == 25
    for v in vec["blake3"]:
        msg = (np.arange(v["len"]) % 251).astype(np.uint8)
        assert u.hash(msg).hex() == v["digest"], v["len"]
    assert len(vec["blake3_kat"]) == 3
    for m, d in vec["blake3_kat"].items():
        assert u.hash(bytes.fromhex(m)).hex() == d, m
    firsts = 0
    for v in vec["fastcdc"]:
        if v["first_chunk_blake3"]:
            d = splitmix_bytes(v["seed"], v["len"])
            assert hashlib.sha256(d.tobytes()).hexdigest() == v["sha256"]
            _, o, n = v["chunks"][0]
            assert u.hash(d[o:o + n]).hex() == v["first_chunk_blake3"], (v["seed"], v["len"])
            firsts += 1
    assert firsts >= 10
    d = splitmix_bytes(0, 8_400_953)  # the first chunk of the cross-check vector
    assert u.hash(d[:1560056]).hex() == A5_DIGEST
    fx = json.load(open(os.path.join(HERE, "golden", "blake3_prefix_collision.json")))
    assert u.hash(bytes.fromhex(fx["m1"])).hex() == fx["digest1"]
    assert u.hash(bytes.fromhex(fx["m2"])).hex() == fx["digest2"]


def test_oracle_large_and_batch_driver(oracle):
    u = _live()
    data = splitmix_bytes(99, (40 << 20) + 777)
    simd = oracle.simd_available()
    for n in [15 << 10, 16 << 10, (16 << 10) + 1, 17 << 10, 256 << 10, 1 << 20, (1 << 20) + 1, (3 << 20) - 1, 3 << 20,
              40 << 20]:
        for off in (0, 3):
            m = data[off:off + n]
            want = u.hash(m)
            assert oracle.blake3(m) == want, (n, off)
            if simd:
                assert oracle.blake3_fast(m) == want, (n, off)
    # the batch driver hashes the slices it reports
    data, offs, lens = tree_corpus(24 << 20, seed=3, max_file=6 << 20)
    blobs = oracle.process_files(data, offs, lens)
    assert len(blobs) > len(offs)  # some files are cut into several blobs
    for b in blobs:  # a blob's offset counts from its file's start (bw_oracle.h)
        o, n = int(offs[int(b["file"])]) + int(b["offset"]), int(b["length"])
        assert bytes(b["digest"]) == u.hash(data[o:o + n]), (int(b["file"]), o, n)
    per_file = np.bincount(blobs["file"].astype(np.int64), weights=blobs["length"].astype(np.float64))
    assert [int(x) for x in per_file] == [int(x) for x in lens]  # and the slices tile every file
