"""Parity without a GPU: tests/parity_ref.py (the yardstick of tests/test_gpu_gf_matmul.py and
tests/test_gpu_parity_shards.py) pinned to constants worked out by hand, and the library's two host-only
entry points, bw_parity_plan and bw_parity_solve, against it."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import parity_ref as pr  # noqa: E402

KM = [(1, 1), (2, 2), (5, 3), (6, 4), (3, 5)]


def test_field_constants():
    assert pr.EXP[8] == 29 and pr.EXP[12] == 205
    assert (pr.LOG[3], pr.LOG[5], pr.LOG[7]) == (25, 50, 198)
    assert len(set(pr.EXP[:255].tolist())) == 255 and pr.EXP[255] == 1  # the generator has order 255
    assert pr.cauchy(3, 2).tolist() == [[142, 244, 71], [244, 142, 167]]
    assert pr.cauchy(4, 1).tolist() == [[1, 142, 244, 71]]
    assert pr.cauchy(253, 3).all()
    # C[i][j] does not depend on k: a short last group uses the leading columns
    assert np.array_equal(pr.cauchy(8, 2)[:, :3], pr.cauchy(3, 2))


def test_every_nonzero_element_has_its_inverse():
    for a in range(1, 256):
        assert pr.mul(a, pr.inv(a)) == 1


def test_multiplication_commutes_and_distributes_over_all_pairs():
    m = pr.MUL
    assert np.array_equal(m, m.T)
    assert all(m[a, b] == pr.mul(a, b) for a in range(256) for b in (0, 1, 2, 3, 0x1d, 0x80, 0xff))
    a = np.arange(256)
    for c in range(256):  # (a ^ b) * c == a * c ^ b * c for all 65,536 pairs (a, b), every c
        assert np.array_equal(m[c][a[:, None] ^ a[None, :]], m[c][a][:, None] ^ m[c][a][None, :])
    assert np.array_equal(m[2], np.array([pr.xtime(x) for x in range(256)], dtype=np.uint8))


def test_packed_doubling_equals_the_bytewise_one():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 1 << 32, 10000, dtype=np.uint64)
    hi = x & 0x80808080
    y = (((x ^ hi) << 1) & 0xffffffff) ^ ((hi - (hi >> 7)) & 0x1d1d1d1d)
    for b in range(4):
        assert np.array_equal((y >> (8 * b)) & 0xff, pr.MUL[2][((x >> (8 * b)) & 0xff).astype(np.int64)])


@pytest.mark.parametrize("k,m", KM)
def test_every_k_subset_of_the_generator_is_invertible(k, m):
    g = pr.generator(k, m)
    for rows in itertools.combinations(range(k + m), k):
        ainv = pr.gauss_inverse(g[list(rows)])
        assert ainv is not None, rows
        assert np.array_equal(pr.small_matmul(ainv, g[list(rows)]), np.eye(k, dtype=np.uint8))


def test_the_reference_recovers_what_it_encoded():
    rng = np.random.default_rng(9)
    packs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (100, 37, 64, 1, 99)]
    shards, groups = pr.encode(packs, 5, 3)
    assert groups == [(0, 5, 3, 112, 0)] and [len(s) for s in shards] == [112] * 3
    full = [p + bytes(112 - len(p)) for p in packs] + shards
    present = [1, 0, 1, 0, 1, 1, 0, 1]
    used, missing, mat = pr.solve(5, 3, present)
    assert used == [0, 2, 4, 5, 7] and missing == [1, 3, 6]
    out = pr.matmul(mat, [full[s] for s in used], 112)
    assert [o.tobytes() for o in out] == [full[s] for s in missing]


# ---------------------------------------------------------------- the library's host-only entry points
@pytest.fixture(scope="module")
def par():
    from backuwup_amd import parity
    return parity


def _plan_tuples(groups):
    return [(int(g["first_packfile"]), int(g["k"]), int(g["m"]), int(g["shard_len"]), int(g["out_offset"])) for g in groups]


@pytest.mark.parametrize("sizes,k,m", [([100, 37, 64, 1, 99], 5, 3), ([16, 17, 15, 4096, 1, 33, 3000000], 3, 2),
                                       ([5] * 9, 8, 1), ([7], 8, 2), (list(range(1, 41)), 4, 4), ([1] * 255, 255, 1)])
def test_plan_equals_the_reference(par, sizes, k, m):
    groups, total = par.plan(sizes, k, m)
    want, want_total = pr.plan(sizes, k, m)
    assert _plan_tuples(groups) == want and total == want_total
    assert all(g[4] % 16 == 0 and g[3] % 16 == 0 for g in want)
    assert want[-1][1] == (len(sizes) - 1) % k + 1  # the short last group takes the remainder


def test_plan_refusals(par):
    from backuwup_amd import _lib
    for sizes, k, m in [([5, 0, 7], 2, 1), ([5], 0, 1), ([5], 1, 0), ([5], 255, 2), ([5], 256, 1)]:
        with pytest.raises(_lib.BwError) as x:
            par.plan(sizes, k, m)
        assert x.value.rc == _lib.BW_EINVAL, (sizes, k, m)
    assert par.plan([5], 255, 1)[1] == 16 and par.plan([5], 1, 255)[1] == 255 * 16
    # a table too small: BW_ENOSPC with both totals set
    import ctypes
    L = _lib.load()
    sz = np.array([10, 20, 30], dtype=np.uint64)
    ng, total = ctypes.c_uint64(), ctypes.c_uint64()
    one = (_lib.BwParityGroup * 1)()
    assert L.bw_parity_plan(sz.ctypes.data_as(_lib.u64p), 3, 1, 2, one, 1, ctypes.byref(ng), ctypes.byref(total)) == _lib.BW_ENOSPC
    assert (ng.value, total.value) == (3, 2 * (16 + 32 + 32))
    assert _lib.load().bw_strerror(_lib.BW_ETOOFEW) == b"fewer shards present than the parity group has data shards"


def _check_solve(par, k, m, present):
    from backuwup_amd import _lib
    try:
        want = pr.solve(k, m, present)
    except pr.TooFew as e:
        with pytest.raises(_lib.BwError) as x:
            par.solve(k, m, present)
        assert x.value.rc == _lib.BW_ETOOFEW
        return e
    used, missing, mat = par.solve(k, m, present)
    assert used == want[0] and missing == want[1], present
    assert np.array_equal(mat, want[2]), present
    return None


@pytest.mark.parametrize("k,m", [(5, 3), (2, 2)])
def test_solve_every_erasure_pattern(par, k, m):
    few = 0
    for bits in itertools.product((0, 1), repeat=k + m):
        few += _check_solve(par, k, m, bits) is not None
    assert few == sum(1 for bits in itertools.product((0, 1), repeat=k + m) if sum(bits) < k)


def test_solve_a_full_field(par):
    """k + m = 256: every element of the field is a row or a column of the Cauchy matrix."""
    rng = np.random.default_rng(11)
    for k, m in [(253, 3), (128, 128), (1, 255), (255, 1)]:
        present = np.ones(k + m, dtype=np.uint8)
        present[rng.choice(k + m, size=min(m, 3), replace=False)] = 0
        assert _check_solve(par, k, m, present) is None
    assert _check_solve(par, 253, 3, [1] * 250 + [0] * 4 + [1] * 2) is not None


def test_solve_refusals(par):
    from backuwup_amd import _lib
    import ctypes
    L = _lib.load()
    u = (ctypes.c_uint32 * 8)()
    n = ctypes.c_uint32()
    b = (ctypes.c_uint8 * 64)()
    for k, m in [(0, 1), (1, 0), (200, 57)]:
        assert L.bw_parity_solve(k, m, b, u, u, ctypes.byref(n), b) == _lib.BW_EINVAL
    assert L.bw_parity_solve(2, 2, None, u, u, ctypes.byref(n), b) == _lib.BW_EINVAL


# ---------------------------------------------------------------- the manifest codec
def _manifest():
    rng = np.random.default_rng(13)
    groups = []
    for k, m in [(3, 2), (1, 1)]:
        groups.append(dict(k=k, m=m, shard_len=4096 + 16 * k, ids=[rng.bytes(12) for _ in range(k)],
                           sizes=[int(rng.integers(1, 4096)) for _ in range(k)], data_digests=[rng.bytes(32) for _ in range(k)],
                           parity_digests=[rng.bytes(32) for _ in range(m)]))
    return groups


def test_manifest_round_trip_and_layout(par):
    groups = _manifest()
    buf = pr.manifest_encode(groups)
    assert len(buf) == 8 + (16 + 3 * 56 + 2 * 32) + (16 + 56 + 32)
    assert buf[:8] == bytes([1, 0, 0, 0, 2, 0, 0, 0]) and buf[8:16] == bytes([3, 0, 0, 0, 2, 0, 0, 0])
    assert int.from_bytes(buf[16:24], "little") == 4096 + 48 and buf[24:36] == groups[0]["ids"][0] and buf[36:40] == bytes(4)
    assert pr.manifest_decode(buf) == groups
    # the package's codec is the same one
    assert par.manifest_encode(groups) == buf and par.manifest_decode(buf) == groups
    assert par.MANIFEST_INFO_TEXT == pr.MANIFEST_INFO_TEXT == b"backuwup parity manifest v1"


def test_manifest_refusals(par):
    buf = bytearray(pr.manifest_encode(_manifest()))
    for codec in (pr, par):
        wrong = bytearray(buf)
        wrong[0] = 2
        with pytest.raises(ValueError):
            codec.manifest_decode(bytes(wrong))
        with pytest.raises(ValueError):
            codec.manifest_decode(bytes(buf) + b"\0")
        pad = bytearray(buf)
        pad[36] = 1
        with pytest.raises(ValueError):
            codec.manifest_decode(bytes(pad))


def test_the_library_exports_parity():
    from backuwup_amd import _lib, parity
    lib = _lib.load()
    for name in ("bw_gf_matmul_device", "bw_gf_matmul", "bw_parity_plan", "bw_parity_build_device", "bw_parity_build",
                 "bw_parity_solve", "bw_parity_repair_device", "bw_parity_repair"):
        assert hasattr(lib, name)
    for name in ("matmul", "plan", "build", "solve", "repair", "protect", "repair_store"):
        assert callable(getattr(parity, name))
