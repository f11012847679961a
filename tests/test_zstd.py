"""Per-blob zstd level 3 (pack.rs:58-64).

CPU part: the oracle's restatement (oracle/bw_oracle_zstd.c) against the system libzstd
(tests/zstd_ref.py, the reference's Compressor settings) byte for byte, and its level-3
parameters against ZSTD_getCParams.  The image's libzstd is 1.4.8; the reference links 1.5.5
(zstd-sys, Cargo.lock:2760), which is absent: equality with 1.5.5 output is "parity unpinned".
GPU part: bw_zstd_compress(_device) against the oracle on the same corpus, and every frame
decoded by libzstd (the reference reader's Decompressor, unpack.rs:66-68).

Frame-mode census (test_corpus_reaches_every_encoder_class; classes from tests/zstd_frames.py).
Frames that reach each class: the edge corpus (zstd_corpus.EDGE_CASES, 49 blobs, asserted), the fixed
corpus of test_gpu_zstd_equals_oracle (6 kinds x SIZES_GPU, 162 blobs) and the blobs of the seeded
random tests (many-mixed, lanes, layouts, test_gpu_fuzz.test_zstd_random_blobs; 2,746 blobs) -- the
last two printed with BW_ZSTD_SIDE_CENSUS=1, not asserted:

    class (frames that reach it)             edge  fixed  random
    block_compressed                           49     90    1740
    block_raw                                  22     82    1011
    block_rle                                  10      4      36
    huf_weights_fse                            21     28     458
    huf_weights_direct                         12      0       5
    lit_raw                                    18     67    1281
    lit_rle                                     2      0       0
    lit_huffman                                33     28     463
    lit_huffman_repeat                          9      4      26
    huffman_repeat_1stream                      3      1       2
    lit_header3_1stream                         5      6      69
    lit_header3_4stream                        10      6     221
    lit_header4                                 6     18     189
    lit_header5                                21      0       0
    ll_predefined                              33     51    1075
    ll_rle                                      6      1       0
    ll_fse                                     17     39     671
    ll_repeat                                   0      0       0
    of_predefined                              29     47     957
    of_rle                                      8      2      28
    of_fse                                     19     42     760
    of_repeat                                   0      0       0
    ml_predefined                              31     52    1074
    ml_rle                                      7      1       1
    ml_fse                                     18     39     671
    ml_repeat                                   0      0       0
    nseq_0                                      8      1       7
    nseq_lt128                                 39     59    1234
    nseq_lt7f00                                15     30     500
    nseq_ge7f00                                 2      0       0
    uncompressed_then_compressed               25      5       6
    raw_then_compressed                        18      2       5
    rle_then_compressed                         7      3       1
    huffman_table_reused_after_raw_block        9      0       0
    literal_count_at_255                        2      0       1
    literal_count_at_256                        2      0       0
    literal_count_at_1023                       2      0       1
    literal_count_at_1024                       2      0       1
    literal_count_at_16383                      4      0       0
    literal_count_at_16384                      4      0       0
    long_offset                                 0      0       0
    of_code_ge20                                2      8       0
    ll_code_35                                  2      1       7
    ml_code_52                                  2     12      53
    rep1                                       20     70    1196
    rep2_at_ll0                                14     35     398
    rep2                                        0      0       0
    rep3_at_ll0                                 0      0       0
    rep3                                        0      0       0
    rep1_minus_1                                0      0       0
"""
import ctypes

import numpy as np
import pytest

import zstd_corpus

SIZES_CPU = [0, 1, 6, 7, 63, 64, 200, 1000, 4096, 16384, 16385, 70000, 131072, 131073,
             262144, 262145, 700000, 2 * 1024 * 1024 + 4096, 3 * 1024 * 1024]


def _zstd():
    import zstd_ref
    if not zstd_ref.available():
        pytest.skip("libzstd not available")
    return zstd_ref


def test_level3_params_match_libzstd(oracle):
    z = _zstd()
    L = z.lib()

    class CP(ctypes.Structure):
        _fields_ = [(f, ctypes.c_uint) for f in
                    ("windowLog", "chainLog", "hashLog", "searchLog", "minMatch", "targetLength", "strategy")]
    L.ZSTD_getCParams.restype = CP
    L.ZSTD_getCParams.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_size_t]
    sizes = set(range(1, 200)) | {(1 << k) + d for k in range(6, 23) for d in (-1, 0, 1)} | {3 << 20}
    for n in sorted(sizes):
        c = L.ZSTD_getCParams(3, n, 0)
        assert c.strategy == 2  # ZSTD_dfast
        assert oracle.zstd3_params(n) == (c.windowLog, c.chainLog, c.hashLog, c.minMatch), n


@pytest.mark.parametrize("kind", zstd_corpus.KINDS)
def test_oracle_equals_libzstd_level3(oracle, kind):
    z = _zstd()
    for i, n in enumerate(SIZES_CPU):
        data = zstd_corpus.blob(kind, n, i)
        frame = oracle.zstd3_compress(data)
        assert frame == z.compress(data), (kind, n)
        assert z.decompress(frame) == data


def test_oracle_random_sizes_equal_libzstd(oracle):
    z = _zstd()
    rng = np.random.default_rng(5)
    for i in range(60):
        kind = zstd_corpus.KINDS[i % len(zstd_corpus.KINDS)]
        n = int(rng.integers(0, 400000)) if i % 3 else int(rng.integers(0, 3000))
        data = zstd_corpus.blob(kind, n, 100 + i)
        assert oracle.zstd3_compress(data) == z.compress(data), (kind, n)


def test_random_data_gives_the_store_frame(oracle):
    """Incompressible blobs: level 3 writes raw blocks, i.e. the store frame the packer's fused
    path emits (oracle/pack_oracle.py zstd_store)."""
    from oracle import pack_oracle as po
    for n in (0, 1, 100, 131072, 131073, 1 << 20, 3 << 20):
        data = zstd_corpus.blob("random", n, n)
        assert oracle.zstd3_compress(data) == po.zstd_store(data)


# ------------------------------------------------------------------ GPU (bw_zstd.hip) vs the oracle
SIZES_GPU = [0, 1, 6, 7, 8, 63, 64, 65, 200, 255, 256, 1000, 1023, 1024, 4096, 16383, 16384, 16385, 70000,
             131071, 131072, 131073, 262144, 262145, 700000, 2 * 1024 * 1024 + 4096, 3 * 1024 * 1024]


def _check_frames(oracle, blobs, frames, z=None):
    for i, (d, f) in enumerate(zip(blobs, frames)):
        want = oracle.zstd3_compress(d)
        assert f == want, (i, len(d), len(f), len(want))
        if z is not None:
            assert z.decompress(f) == bytes(d)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", zstd_corpus.KINDS)
def test_gpu_zstd_equals_oracle(ctx, oracle, kind):
    blobs = [zstd_corpus.blob(kind, n, i) for i, n in enumerate(SIZES_GPU)]
    frames = ctx.zstd_compress(blobs)
    import zstd_ref
    _check_frames(oracle, blobs, frames, zstd_ref if zstd_ref.available() else None)


def _mixed_blobs():
    rng = np.random.default_rng(11)
    blobs = []
    for i in range(240):
        kind = zstd_corpus.KINDS[int(rng.integers(len(zstd_corpus.KINDS)))]
        n = int(rng.choice([rng.integers(0, 300), rng.integers(300, 20000), rng.integers(20000, 300000)]))
        blobs.append(zstd_corpus.blob(kind, n, 1000 + i))
    return blobs


def _lane_blobs(lanes):
    rng = np.random.default_rng(23)
    return [[zstd_corpus.blob(zstd_corpus.KINDS[(b + i) % len(zstd_corpus.KINDS)],
                              int(rng.choice([rng.integers(0, 500), rng.integers(500, 200000)])), 3000 + 100 * b + i)
             for i in range(40)] for b in range(lanes)]


def _layout_blobs():
    rng = np.random.default_rng(29)
    many = [zstd_corpus.blob(zstd_corpus.KINDS[i % len(zstd_corpus.KINDS)], int(rng.integers(0, 3000)), 5000 + i)
            for i in range(2100)]
    few = [zstd_corpus.blob(zstd_corpus.KINDS[i % len(zstd_corpus.KINDS)], int(rng.integers(1000, 300000)), 9000 + i)
           for i in range(30)]
    return many, few


@pytest.mark.gpu
def test_gpu_zstd_many_mixed_blobs_small_batches(oracle):
    """Hundreds of blobs of every kind in one call, split into internal batches of at most 7 blobs
    / 1 MiB (hash-table slots reused across batches through their index bases)."""
    from backuwup_amd import Context, _lib
    blobs = _mixed_blobs()
    with Context(0) as c:
        c.set_option(_lib.BW_OPT_ZSTD_SLOTS, 7)
        c.set_option(_lib.BW_OPT_ZSTD_BATCH_BYTES, 1 << 20)
        f1 = c.zstd_compress(blobs)
        f2 = c.zstd_compress(blobs[::-1])  # the same slots again, at higher index bases
    _check_frames(oracle, blobs, f1)
    _check_frames(oracle, blobs[::-1], f2)


@pytest.mark.gpu
def test_gpu_zstd_device_buffers(ctx, oracle):
    import torch
    blobs = [zstd_corpus.blob(k, 3 * 1024 * 1024 - 5 * i, 77 + i) for i, k in enumerate(zstd_corpus.KINDS)]
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    so = np.concatenate([[0], np.cumsum(lens + 16)[:-1]]).astype(np.uint64)
    host = np.zeros(int(so[-1] + lens[-1]), dtype=np.uint8)
    for o, b in zip(so, blobs):
        host[int(o):int(o) + len(b)] = np.frombuffer(b, np.uint8)
    d_src = torch.from_numpy(host).cuda()
    cap = np.array([ctx._L.bw_zstd_store_size(int(x)) for x in lens], dtype=np.uint64)
    do = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.uint64)
    d_dst = torch.zeros(int(cap.sum()), dtype=torch.uint8, device="cuda")
    fl = ctx.zstd_compress_device(d_src.data_ptr(), so, lens, d_dst.data_ptr(), do)
    out = d_dst.cpu().numpy()
    frames = [out[int(do[i]):int(do[i] + fl[i])].tobytes() for i in range(len(blobs))]
    _check_frames(oracle, blobs, frames)


@pytest.mark.gpu
def test_gpu_zstd_rejects_blob_over_3mib(ctx):
    from backuwup_amd._lib import BwError
    with pytest.raises(BwError):
        ctx.zstd_compress([bytes(3 * 1024 * 1024 + 1)])


@pytest.mark.gpu
def test_gpu_zstd_async_lanes_equal_oracle(oracle):
    """bw_zstd_submit_device / bw_zstd_wait: BW_ZSTD_LANES batches in flight on one context (each
    lane its own stream and hash tables, one with small slot limits so its tables are reused),
    waited out of order; every frame equals the oracle's; a submit with every lane busy and a
    wait on an unknown ticket are BW_ESTATE."""
    import torch
    from backuwup_amd import Context, _lib
    from backuwup_amd._lib import BwError
    batches = []
    for blobs in _lane_blobs(_lib.BW_ZSTD_LANES):
        lens = np.array([len(x) for x in blobs], dtype=np.uint64)
        so = np.concatenate([[0], np.cumsum(lens + 16)[:-1]]).astype(np.uint64)
        host = np.zeros(int(so[-1] + lens[-1]) + 16, dtype=np.uint8)
        for o, x in zip(so, blobs):
            host[int(o):int(o) + len(x)] = np.frombuffer(x, np.uint8)
        cap = np.array([_lib.load().bw_zstd_store_size(int(x)) for x in lens], dtype=np.uint64)
        do = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.uint64)
        batches.append((blobs, so, lens, do, torch.from_numpy(host).cuda(),
                        torch.zeros(int(cap.sum()), dtype=torch.uint8, device="cuda")))
    with Context(0) as c:
        c.set_option(_lib.BW_OPT_ZSTD_SLOTS, 5)  # copied to the lanes: internal batches of 5 blobs
        tickets = [c.zstd_submit_device(src.data_ptr(), so, lens, dst.data_ptr(), do)
                   for blobs, so, lens, do, src, dst in batches]
        with pytest.raises(BwError):
            c.zstd_submit_device(batches[0][4].data_ptr(), batches[0][1], batches[0][2], batches[0][5].data_ptr(),
                                 batches[0][3])
        fls = {t: c.zstd_wait(t) for t in reversed(tickets)}
        with pytest.raises(BwError):
            c.zstd_wait(tickets[0])
        again = c.zstd_submit_device(batches[1][4].data_ptr(), batches[1][1], batches[1][2], batches[1][5].data_ptr(),
                                     batches[1][3])  # a lane is free again
        fl_again = c.zstd_wait(again)
    for t, (blobs, so, lens, do, src, dst) in zip(tickets, batches):
        out = dst.cpu().numpy()
        frames = [out[int(do[i]):int(do[i] + fls[t][i])].tobytes() for i in range(len(blobs))]
        _check_frames(oracle, blobs, frames)
    assert np.array_equal(fl_again, fls[tickets[1]])


@pytest.mark.gpu
def test_gpu_zstd_table_layouts_and_switches(oracle):
    """Sub-batches of more than 2,048 blobs parse with narrow (libzstd u32) tables, smaller ones with
    wide entries that carry their bytes; a slot that changes layout is cleared first.  One context:
    narrow, wide, narrow again over the same slots; every frame equals the oracle's."""
    from backuwup_amd import Context
    many, few = _layout_blobs()
    with Context(0) as c:
        f_many = c.zstd_compress(many)
        f_few = c.zstd_compress(few)
        f_many2 = c.zstd_compress(many[::-1])
    _check_frames(oracle, many, f_many)
    _check_frames(oracle, few, f_few)
    _check_frames(oracle, many[::-1], f_many2)


# ------------------------------------------------------------------ the frame-mode census
# Every mode of the frame format that the level-3 encoder chooses between, and the number of
# distinct blobs of zstd_corpus.EDGE_CASES that must reach it (classes: tests/zstd_frames.py).
# A class at 0 cannot be produced by this encoder; its argument is in UNREACHABLE, and the census
# asserts that nothing reaches it (an input that does makes the argument, and this table, wrong).
UNREACHABLE = {
    "fse_repeat":
        "Table mode 'repeat' (LL, OF, ML).  Below the lazy strategies ZSTD_selectEncodingType returns "
        "set_repeat only when the previous block's table is marked valid, and only a dictionary marks it "
        "so; a table written by a block is marked 'check', which strategies below lazy (dfast is 2) never "
        "act on.  The reference compresses every blob with a fresh, dictionary-less compressor, and the "
        "oracle's select_encoding and bw_zstd.hip's section_tables have no such branch.  The fse_follow "
        "blobs (an FSE-coded block, then under 1,000 sequences of the same statistics) are where it "
        "would appear; libzstd writes fresh tables there.",
    "offset_values_2_3":
        "Offset values 2 and 3 (repeat offsets 2 and 3 after literals, repeat offset 3 and 'repeat 1 minus "
        "1' at ll == 0).  ZSTD_compressBlock_doubleFast stores a sequence in three places: the repeat "
        "probe at ip + 1 and the immediate-repeat loop (offset code 0, offset value 1), and a hash match "
        "(offset + 2, offset value >= 4).  Offset value 1 is repeat offset 1 after literals and repeat "
        "offset 2 at ll == 0, and both are required below.",
    "long_offset":
        "Offset codes above 25 (the decoders' long-offset mode; above 28 the predefined OF table is "
        "disallowed).  Blobs are at most 3 MiB, so level 3's window log is min(21, ceil(log2 n)) <= 21 "
        "(oracle.zstd3_params); an offset is below the window size, its value at most 2^21 + 2, its code "
        "at most 21.  Codes of 20 and more (offsets past 1 MiB) are required below instead.",
}
assert len(UNREACHABLE) <= 3
# The 3-byte sequence count is NOT excused: it needs 0x7F00 = 32,512 sequences in a 128 KiB block,
# level 3's shortest match is 4 bytes whatever minMatch says (the finder confirms candidates with a
# 4-byte compare), and 131,072 / 4 = 32,768 >= 32,512 -- possible only with almost no literals, which
# is what the immediate-repeat loop emits when two offsets alternate (the seqflood blobs).
REQUIRED = {
    "block_compressed": 2, "block_raw": 2, "block_rle": 2,
    "huf_weights_fse": 2, "huf_weights_direct": 2,
    "lit_raw": 2, "lit_rle": 2, "lit_huffman": 2, "lit_huffman_repeat": 2, "huffman_repeat_1stream": 2,
    "lit_header3_1stream": 2, "lit_header3_4stream": 2, "lit_header4": 2, "lit_header5": 2,
    "ll_predefined": 2, "ll_rle": 2, "ll_fse": 2, "ll_repeat": (0, "fse_repeat"),
    "of_predefined": 2, "of_rle": 2, "of_fse": 2, "of_repeat": (0, "fse_repeat"),
    "ml_predefined": 2, "ml_rle": 2, "ml_fse": 2, "ml_repeat": (0, "fse_repeat"),
    "nseq_0": 2, "nseq_lt128": 2, "nseq_lt7f00": 2, "nseq_ge7f00": 2,
    "uncompressed_then_compressed": 2, "raw_then_compressed": 2, "rle_then_compressed": 2,
    "huffman_table_reused_after_raw_block": 2,
    "literal_count_at_255": 2, "literal_count_at_256": 2, "literal_count_at_1023": 2, "literal_count_at_1024": 2,
    "literal_count_at_16383": 2, "literal_count_at_16384": 2,
    "long_offset": (0, "long_offset"), "of_code_ge20": 2, "ll_code_35": 2, "ml_code_52": 2,
    "rep1": 2, "rep2_at_ll0": 2,
    "rep2": (0, "offset_values_2_3"), "rep3_at_ll0": (0, "offset_values_2_3"), "rep3": (0, "offset_values_2_3"),
    "rep1_minus_1": (0, "offset_values_2_3"),
}

_edge = {}


def _edge_corpus(oracle):
    """[(name, blob, oracle frame, classes)] of the edge corpus, computed once per session."""
    import zstd_frames
    if not _edge:
        rows = []
        for kind, n, seed, data in zstd_corpus.edge_corpus():
            frame = oracle.zstd3_compress(data)
            blocks = zstd_frames.classify(frame)  # raises unless it consumes the frame exactly
            assert sum(b["regen"] for b in blocks) == len(data), (kind, n, seed)
            rows.append(("%s-%d-%d" % (kind, n, seed), data, frame, frozenset(zstd_frames.frame_classes(blocks))))
        _edge["rows"] = rows
    return _edge["rows"]


def _print_census(title, count):
    print("\n%s" % title)
    for k in REQUIRED:
        print("  %-40s %5d" % (k, count[k]))


def test_corpus_reaches_every_encoder_class(oracle):
    """The census: every class of REQUIRED is reached by at least its minimum of distinct edge
    blobs, on the oracle's frames; every frame is consumed exactly by the classifier, its blocks'
    regenerated sizes add up to the blob, and (libzstd present) it equals libzstd 1.4.8's frame and
    decodes to the blob.  The sequence-level classes (offset codes, repeat codes, largest LL / ML
    codes) come from the classifier's own decode of the sequences bitstream, not from the oracle.
    BW_ZSTD_SIDE_CENSUS=1 also prints the census of the fixed corpus and of the seeded random tests'
    blobs (half a minute of pure-Python decoding; the module docstring's table is one such run)."""
    import os
    import zstd_frames
    import zstd_ref
    assert set(REQUIRED) == set(zstd_frames.FORMAT_CLASSES)
    rows = _edge_corpus(oracle)
    assert len({d for _, d, _, _ in rows}) == len(rows), "edge blobs are not distinct"
    assert sum(len(d) for _, d, _, _ in rows) < 48 << 20 and max((len(d) for _, d, _, _ in rows), default=0) <= 3 << 20
    if zstd_ref.available():
        for name, data, frame, _ in rows:
            assert frame == zstd_ref.compress(data), name
            assert zstd_ref.decompress(frame) == data, name
    count = dict.fromkeys(REQUIRED, 0)
    for _, _, _, classes in rows:
        for k in classes:
            count[k] += 1
    _print_census("edge corpus (%d blobs)" % len(rows), count)
    short = {k: (count[k], v) for k, v in REQUIRED.items() if not isinstance(v, tuple) and count[k] < v}
    assert not short, "classes reached by too few edge blobs (have, need): %r" % short
    stale = {k: count[k] for k, v in REQUIRED.items() if isinstance(v, tuple) and (count[k] or v[1] not in UNREACHABLE)}
    assert not stale, "classes excused as unreachable that are reached, or excused without an argument: %r" % stale
    if os.environ.get("BW_ZSTD_SIDE_CENSUS"):
        import test_gpu_fuzz
        from backuwup_amd import _lib
        fixed = [zstd_corpus.blob(kind, n, i) for kind in zstd_corpus.KINDS for i, n in enumerate(SIZES_GPU)]
        many, few = _layout_blobs()
        rand = (_mixed_blobs() + [b for lane in _lane_blobs(_lib.BW_ZSTD_LANES) for b in lane] + many + few +
                [b for case in range(6) for b in test_gpu_fuzz.zstd_random_blobs(case)])
        for title, blobs in (("fixed corpus", fixed), ("seeded random tests", rand)):
            _print_census("%s (%d blobs)" % (title, len(blobs)),
                          zstd_frames.census(oracle.zstd3_compress(b) for b in blobs))


def _pack_device(L, blobs):
    """The blobs in one device buffer, 16 bytes apart, and a frame buffer of their store sizes."""
    import torch
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    so = np.concatenate([[0], np.cumsum(lens + 16)[:-1]]).astype(np.uint64)
    host = np.zeros(int(so[-1] + lens[-1]) + 16, dtype=np.uint8)
    for o, b in zip(so, blobs):
        host[int(o):int(o) + len(b)] = np.frombuffer(b, np.uint8)
    cap = np.array([L.bw_zstd_store_size(int(x)) for x in lens], dtype=np.uint64)
    do = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.uint64)
    return so, lens, do, torch.from_numpy(host).cuda(), torch.zeros(int(cap.sum()), dtype=torch.uint8, device="cuda")


def _frames_of(dst, do, fl):
    out = dst.cpu().numpy()
    return [out[int(do[i]):int(do[i] + fl[i])].tobytes() for i in range(len(fl))]


def _check_edge(rows, frames, how, z=None):
    """Byte equality with the oracle's frames; a mismatch names the blob and the classes it reaches."""
    assert len(frames) == len(rows)
    for (name, data, want, classes), f in zip(rows, frames):
        assert f == want, "%s: %s differs from the oracle (%d vs %d bytes); the blob reaches %s" % (
            how, name, len(f), len(want), sorted(classes))
        if z is not None:
            assert z.decompress(f) == data, (how, name)


@pytest.mark.gpu
def test_gpu_zstd_edge_classes_equal_oracle(ctx, oracle):
    """Every blob of the edge corpus (one per frame mode the fixed corpus misses, see the census)
    in one bw_zstd_compress call and again through bw_zstd_compress_device."""
    import zstd_ref
    rows = _edge_corpus(oracle)
    blobs = [d for _, d, _, _ in rows]
    z = zstd_ref if zstd_ref.available() else None
    _check_edge(rows, ctx.zstd_compress(blobs), "zstd_compress", z)
    so, lens, do, src, dst = _pack_device(ctx._L, blobs)
    fl = ctx.zstd_compress_device(src.data_ptr(), so, lens, dst.data_ptr(), do)
    _check_edge(rows, _frames_of(dst, do, fl), "zstd_compress_device", z)


@pytest.mark.gpu
def test_gpu_zstd_edge_classes_three_slots(oracle):
    """A fresh context with three hash-table slots: the edge blobs share and reuse slots across
    internal batches, forward and reversed, so a blob rerun after a wrong guess about its
    uncompressed blocks (a fresh index range in its slot) is followed by the slot's next use."""
    from backuwup_amd import Context, _lib
    rows = _edge_corpus(oracle)
    blobs = [d for _, d, _, _ in rows]
    with Context(0) as c:
        c.set_option(_lib.BW_OPT_ZSTD_SLOTS, 3)
        f1 = c.zstd_compress(blobs)
        f2 = c.zstd_compress(blobs[::-1])
    _check_edge(rows, f1, "3 slots, forward")
    _check_edge(rows[::-1], f2, "3 slots, reversed")


@pytest.mark.gpu
def test_gpu_zstd_edge_classes_async_lanes(oracle):
    """One bw_zstd_submit_device per lane, each carrying the blobs with an uncompressed block before
    a compressed one (the rerun path) in a different rotation, waited in reverse order."""
    from backuwup_amd import Context, _lib
    rows = [r for r in _edge_corpus(oracle) if "uncompressed_then_compressed" in r[3]]
    assert len(rows) >= 4
    lanes = []
    for b in range(_lib.BW_ZSTD_LANES):
        k = b * len(rows) // _lib.BW_ZSTD_LANES
        lanes.append(rows[k:] + rows[:k])
    with Context(0) as c:
        packed = [_pack_device(c._L, [d for _, d, _, _ in lane]) for lane in lanes]
        tickets = [c.zstd_submit_device(src.data_ptr(), so, lens, dst.data_ptr(), do) for so, lens, do, src, dst in packed]
        fls = {t: c.zstd_wait(t) for t in reversed(tickets)}
    for b, (t, lane, (so, lens, do, src, dst)) in enumerate(zip(tickets, lanes, packed)):
        _check_edge(lane, _frames_of(dst, do, fls[t]), "lane %d" % b)
