"""bw_zstd_decompress(_device) on the GPU (k_zd_frame, backuwup_amd/csrc/bw_zstd_dec.hip): frames of
the system libzstd at levels 1, 3, 7, 13 and 19 and of the device encoder, as ragged batches.  The
frame sets are those of tests/test_zstd_decode_host.py, which runs the same decoder core on the CPU
under ASan/UBSan; the mutated frames go to the device only in test_gpu_mutated_frames."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_corpus  # noqa: E402
import zstd_decode_cases as zc  # noqa: E402
import zstd_ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]
CANARY = 64


def _decode_device(ctx, frames, caps, pad=3):
    """One ragged batch through bw_zstd_decompress_device: frames at offsets that are no multiple
    of anything, each output range followed by a canary.  -> (blobs or None, out_len, canaries ok)."""
    import torch
    n = len(frames)
    so, at = [], 1
    for f in frames:
        so.append(at)
        at += len(f) + pad
    src = np.full(at + 16, 0x5A, dtype=np.uint8)
    for o, f in zip(so, frames):
        src[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    do, at = [], 5
    for c in caps:
        do.append(at)
        at += c + CANARY
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    ol, ok = ctx.zstd_decompress_device(d_src.data_ptr(), so, [len(f) for f in frames], d_dst.data_ptr(), do, caps)
    out = d_dst.cpu().numpy()
    assert out[:5].tobytes() == b"\xa5" * 5
    blobs, canaries = [], True
    for i in range(n):
        canaries &= out[do[i] + caps[i]:do[i] + caps[i] + CANARY].tobytes() == b"\xa5" * CANARY
        blobs.append(out[do[i]:do[i] + int(ol[i])].tobytes() if ok[i] else None)
    return blobs, ol, canaries


def test_gpu_census_corpus_one_ragged_batch(ctx):
    frames = zc.frames()
    blobs, ol, canaries = _decode_device(ctx, [f for _, _, _, f in frames], [len(s) for _, _, s, _ in frames])
    assert canaries
    for (name, lv, src, _), b, n in zip(frames, blobs, ol):
        assert b is not None and int(n) == len(src), (name, lv)
        assert b == src, (name, lv)


def test_gpu_census_corpus_host_form(ctx):
    frames = zc.frames()
    got = ctx.zstd_decompress([f for _, _, _, f in frames])
    for (name, lv, src, _), b in zip(frames, got):
        assert b == src, (name, lv)


def test_gpu_edges_in_one_batch(ctx):
    from backuwup_amd import _lib
    L = _lib.load()
    text = zstd_corpus.blob("text", 3 << 20, 5)
    blobs = [b"", b"x", zstd_corpus.blob("text", 131072, 1), zstd_corpus.blob("text", 131073, 2), text]
    frames = [zstd_ref.compress(b, 3) for b in blobs]
    assert frames[0][2:] == b"\x01\x00\x00"  # the empty blob: one raw block of size 0
    raw = zstd_corpus.blob("random", 300000, 3)
    store = bytearray([0, (max(10, (len(raw) - 1).bit_length()) - 10) << 3])  # bw_zstd_store_size's layout
    for k in range(0, len(raw), 131072):
        store += zc.block(0, raw[k:k + 131072], k + 131072 >= len(raw))
    assert len(store) == L.bw_zstd_store_size(len(raw))
    blobs.append(raw)
    frames.append(bytes(store))
    got, ol, canaries = _decode_device(ctx, frames, [len(b) for b in blobs])
    assert canaries
    assert got == blobs and [int(x) for x in ol] == [len(b) for b in blobs]


def test_gpu_round_trip_on_the_device(ctx):
    """bw_zstd_compress_device then bw_zstd_decompress_device, without leaving the device."""
    import torch
    from backuwup_amd import _lib
    L = _lib.load()
    blobs = [b for _, _, b in zstd_corpus.corpus([5000, 400000])] + [b for _, _, _, b in zstd_corpus.edge_corpus()]
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    so = np.concatenate([[0], np.cumsum(lens[:-1] + np.uint64(7))]).astype(np.uint64)
    host = np.zeros(int(so[-1] + lens[-1]) + 16, dtype=np.uint8)
    for o, b in zip(so, blobs):
        host[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    cap = np.array([L.bw_zstd_store_size(int(x)) for x in lens], dtype=np.uint64)
    fo = np.concatenate([[0], np.cumsum(cap[:-1])]).astype(np.uint64)
    d_src = torch.from_numpy(host).cuda()
    d_frames = torch.zeros(int(cap.sum()), dtype=torch.uint8, device="cuda")
    fl = ctx.zstd_compress_device(d_src.data_ptr(), so, lens, d_frames.data_ptr(), fo)
    d_back = torch.zeros(host.size, dtype=torch.uint8, device="cuda")
    ol, ok = ctx.zstd_decompress_device(d_frames.data_ptr(), fo, fl, d_back.data_ptr(), so, lens)
    assert ok.all() and np.array_equal(ol, lens)
    back = d_back.cpu().numpy()
    for o, b in zip(so, blobs):
        assert back[int(o):int(o) + len(b)].tobytes() == b


def test_gpu_mutated_frames(ctx, tmp_path):
    """The host test's mutated frames on the device, with its four requirements; the canary behind
    every output range is checked by a copy back.  The decoder core runs over them on the host
    first (a plain build here; under the sanitizers in tests/test_zstd_decode_host.py::
    test_mutated_frames, a CPU test), and only a green host run lets them go to the device."""
    from test_zstd_decode_host import check_mutations
    muts = [m for _, _, m in zc.mutations()]
    # 928 ranges of 3 MiB would be 2.9 GB: every frame libzstd decodes gets what it regenerates
    # plus slack, every other one 470,000 bytes, so capacity is never why a frame is refused
    caps = [min(zc.CAP, (len(v) if v is not None else 400000) + 70000) for v in zc.libzstd_verdicts()]
    ref = zc.run_host(zc.build_host(tmp_path, sanitize=False), list(zip(muts, caps)), tmp_path, "gpu_mut", sanitized=False)
    check_mutations(ref)
    blobs, ol, canaries = _decode_device(ctx, muts, caps)
    assert canaries
    # ok[] says decoded or not; the cause of a refusal is the core's, from the host run
    for i, (b, (e, hb, _)) in enumerate(zip(blobs, ref)):
        assert (b is not None) == (e == 0), (i, e)
        assert b is None or b == hb, i
    check_mutations([(e, b or b"", True) for b, (e, _, _) in zip(blobs, ref)])


def test_gpu_capacity_and_empty_batch(ctx):
    import torch
    from backuwup_amd import _lib
    from backuwup_amd._lib import BwError
    f = zstd_ref.compress(b"abc", 3)
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(BwError) as e:
        ctx.zstd_decompress_device(d.data_ptr(), [0], [len(f)], d.data_ptr(), [0], [(3 << 20) + 1])
    assert e.value.rc == _lib.BW_EINVAL
    L = _lib.load()
    assert L.bw_zstd_decompress_device(ctx.h, None, None, None, 0, None, None, None, None, None) == _lib.BW_OK
    assert L.bw_zstd_decompress(ctx.h, None, None, None, 0, None, None, None, None, None) == _lib.BW_OK
    assert ctx.zstd_decompress([]) == []
    # dst_cap one byte short: refused, and the byte after dst_cap untouched
    src = b"hello, hello, hello, hello, world" * 40
    blobs, ol, canaries = _decode_device(ctx, [zstd_ref.compress(src, 3)] * 2, [len(src), len(src) - 1])
    assert canaries and blobs == [src, None] and int(ol[1]) == 0
