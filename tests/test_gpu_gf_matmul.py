"""bw_gf_matmul_device / bw_gf_matmul (k_gf_matmul: dst_r = XOR_c M[r][c] * src_c over GF(2^8), sources at
any alignment and zero beyond their length) against tests/parity_ref.py, byte for byte: the outputs, 0xC3
canaries around every destination, and the sources, which must come back untouched.  Every case runs
through the device and the host form."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import parity_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

T = 8                  # bw_internal.h GF_ROW_TILE: destination rows per pass over the sources
W = 2048               # GF_WAVE_BYTES: bytes of every row one wave task covers (two steps of 64 lanes x 16)
G = 1024 * 4 * W       # GF_GRID_BLOCKS blocks of 4 waves: bytes per row of one grid pass
CANARY = 0xC3


def test_constants_match_the_binding():
    from backuwup_amd import _lib
    assert (_lib.GF_ROW_TILE, _lib.GF_WAVE_BYTES, _lib.GF_GRID_BYTES) == (T, W, G)


def _layout(sizes, align, gap):
    off, pos = [], gap
    for i, n in enumerate(sizes):
        pos += (int(align[i]) - pos) % 16
        off.append(pos)
        pos += int(n) + gap
    return np.array(off, dtype=np.uint64), pos + 16


def _run(ctx, matrix, srcs, src_len, length, src_align=None, want=None):
    """srcs: the bytes placed at each source's offset (they may be longer than src_len: what lies beyond
    must not count).  Both forms against the reference; returns the rows."""
    import torch
    from backuwup_amd import parity
    matrix = np.asarray(matrix, dtype=np.uint8)
    rows, cols = matrix.shape
    src_len = [int(x) for x in src_len]
    if src_align is None:
        src_align = [(5 * c + 3) % 16 for c in range(cols)]
    soff, stotal = _layout([len(s) for s in srcs], src_align, gap=7)
    buf = np.full(stotal, CANARY, dtype=np.uint8)
    for o, s in zip(soff, srcs):
        buf[int(o):int(o) + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    doff, dtotal = _layout([length] * rows, [0] * rows, gap=16)
    if want is None:
        want = pr.matmul(matrix, [bytes(s)[:n] for s, n in zip(srcs, src_len)], length)
    expect = np.full(dtotal, CANARY, dtype=np.uint8)
    for r in range(rows):
        expect[int(doff[r]):int(doff[r]) + length] = want[r]
    before = buf.copy()
    out = np.full(dtotal, CANARY, dtype=np.uint8)
    parity.matmul(ctx, matrix, buf, soff, src_len, doff, length, dst_size=dtotal, out=out)
    assert np.array_equal(buf, before), "bw_gf_matmul wrote the host source"
    d_src = torch.from_numpy(buf).cuda()
    d_dst = torch.full((dtotal,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch's stream is not the context's
    parity.matmul_device(ctx, matrix, d_src.data_ptr(), soff, src_len, d_dst.data_ptr(), doff, length)
    torch.cuda.synchronize()
    assert np.array_equal(d_src.cpu().numpy(), before), "bw_gf_matmul_device wrote the source buffer"
    for name, o in (("bw_gf_matmul", out), ("bw_gf_matmul_device", d_dst.cpu().numpy())):
        bad = np.flatnonzero(o != expect)
        assert not bad.size, (name, "first differing byte", int(bad[0]), "row",
                              int(np.searchsorted(doff, bad[0], side="right")) - 1, "of", rows, "len", length)
    return want


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, W - 1, W, W + 1])
def test_lengths_around_every_boundary(ctx, length):
    rng = np.random.default_rng(500 + length)
    matrix = rng.integers(1, 256, (2, 3), dtype=np.uint8)
    srcs = [rng.bytes(length) for _ in range(3)]
    _run(ctx, matrix, srcs, [length] * 3, length)


def test_more_than_one_grid_pass(ctx):
    length = G + 16
    src = np.random.default_rng(501).integers(0, 256, length, dtype=np.uint8)
    want = pr.MUL[0x53][src][None, :]
    _run(ctx, [[0x53]], [src.tobytes()], [length], length, src_align=[9], want=want)


def test_every_source_alignment(ctx):
    rng = np.random.default_rng(502)
    length = W + 37
    matrix = rng.integers(0, 256, (3, 16), dtype=np.uint8)
    srcs = [rng.bytes(length) for _ in range(16)]
    _run(ctx, matrix, srcs, [length] * 16, length, src_align=list(range(16)))


def test_zero_extension(ctx):
    """A source ends anywhere: nowhere, after one byte, one byte short, inside a lane's 16 bytes, either side
    of a wave task's border.  The bytes that lie beyond it in the buffer are not zero and must not count."""
    rng = np.random.default_rng(503)
    length = 2 * W + 100
    ends = [0, 1, length - 1, length, 16 * 5 + 7, 1024 - 1, 1024 + 9, W - 3, W, W + 5, 2 * W + 99 - 16]
    matrix = rng.integers(1, 256, (T + 1, len(ends)), dtype=np.uint8)
    srcs = [rng.integers(1, 256, length, dtype=np.uint8).tobytes() for _ in ends]
    _run(ctx, matrix, srcs, ends, length)
    # and a source that is longer than the rows: only the first `length` bytes count
    _run(ctx, matrix[:, :2], [rng.bytes(length + 50)] * 2, [length + 50, length + 1], length)


@pytest.mark.parametrize("cols", [1, 2, 8, 255])
def test_matrix_shapes(ctx, cols):
    rng = np.random.default_rng(504 + cols)
    length = 1024 + 13
    srcs = [rng.bytes(length) for _ in range(cols)]
    for rows in (1, T, T + 1, 2 * T + 1):
        matrix = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
        _run(ctx, matrix, srcs, [length] * cols, length)


def test_matrix_values(ctx):
    rng = np.random.default_rng(505)
    length = W + 300
    cols, rows = 7, T + 3
    matrix = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    matrix[0, :] = [0, 1, 2, 0x80, 0xff, 3, 0x1d]
    matrix[1, :] = [1, 0, 0, 0, 0, 0, 0]      # a copy of source 0
    matrix[4, :] = 0                           # a zero row: written as zeros
    matrix[T + 1, :] = 0xff
    matrix[:, 5] = 0                           # a zero column: source 5 must not matter
    srcs = [rng.bytes(length) for _ in range(cols)]
    a = _run(ctx, matrix, srcs, [length] * cols, length)
    assert not a[4].any() and a[1].tobytes() == srcs[0]
    srcs[5] = bytes([0x5a]) * length
    b = _run(ctx, matrix, srcs, [length] * cols, length)
    assert np.array_equal(a, b)
    # the field's own table through the kernel: every coefficient times every byte
    every = bytes(range(256))
    full = _run(ctx, np.arange(256, dtype=np.uint8).reshape(256, 1), [every], [256], 256)
    assert np.array_equal(full, pr.MUL)


def test_refusals(ctx):
    import torch
    from backuwup_amd import _lib, parity
    d = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    host = np.zeros(1024, dtype=np.uint8)
    torch.cuda.synchronize()
    for doff in ([8], [16, 1031], [1024 + 1]):
        m = np.ones((len(doff), 2), dtype=np.uint8)
        with pytest.raises(_lib.BwError) as x:
            parity.matmul_device(ctx, m, d.data_ptr(), [0, 100], [64, 64], d.data_ptr() + 2048, doff, 64)
        assert x.value.rc == _lib.BW_EINVAL
        with pytest.raises(_lib.BwError) as x:
            parity.matmul(ctx, m, host, [0, 100], [64, 64], doff, 64, dst_size=2048)
        assert x.value.rc == _lib.BW_EINVAL
    with pytest.raises(_lib.BwError) as x:   # destinations that overlap
        parity.matmul_device(ctx, np.ones((2, 1), np.uint8), d.data_ptr(), [0], [64], d.data_ptr() + 2048, [0, 48], 64)
    assert x.value.rc == _lib.BW_EINVAL
    with pytest.raises(_lib.BwError) as x:   # a destination over a source
        parity.matmul_device(ctx, np.ones((1, 1), np.uint8), d.data_ptr(), [40], [64], d.data_ptr(), [96], 64)
    assert x.value.rc == _lib.BW_EINVAL
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == CANARY).all(), "a refused call wrote device memory"
