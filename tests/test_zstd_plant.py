"""The planted frames (tests/zstd_plant_cases.py, written with tests/zstd_plant.py) pinned on the
CPU before any of them goes to a device (tests/test_gpu_zstd_planted.py):

- three readings agree on every frame: the system libzstd, zstd_plant.replay (the RFC's rules over
  the planted literals and sequences) and tests/zstd_frames.py (which must consume every accepted
  frame exactly and find the classes the case was built for);
- the decoder core (backuwup_amd/csrc/bw_zstd_dec_core.h) as the stand-alone host program under
  ASan/UBSan gives the same verdict and bytes, keeps its canary and raises no report;
- the planted frames and the libzstd corpus frames together reach every name of
  zstd_frames.DECODER_CLASSES.

replay states RFC 8878 as the decoder reads it.  Where libzstd is laxer than that and the decoder
is not, by decision, the frame is named in DIVERGENCES with the zd::Err expected; every frame
outside that table has libzstd and replay agreeing, on the verdict and on the bytes.

The image has libzstd 1.4.8; the reference links zstd 1.5.5.  LIBZSTD_1_4_8 records what 1.4.8 says
about the frames on which releases may differ; the decoder's verdict on them does not depend on it."""
import ctypes
import os
import struct
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_decode_cases as zc  # noqa: E402
import zstd_frames  # noqa: E402
import zstd_plant  # noqa: E402
import zstd_plant_cases as pc  # noqa: E402
import zstd_ref  # noqa: E402

pytestmark = pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")

from zstd_plant_cases import E_BLOCK_SIZE, E_CHECKSUM, E_LITERALS, E_OFFSET, E_SEQ_HEADER, want_err  # noqa: E402

# The one table of frames the decoder refuses although libzstd decodes them:
# name -> (the rule replay names or None for a frame that is not planted, zd::Err, why).
DIVERGENCES = {
    "B_ml_longest_plus_1": ("block_size", E_BLOCK_SIZE,
                            "3.1.1.2.4: a block regenerates at most 128 KiB; libzstd's one-shot path bounds only the capacity"),
    "D_rep1_minus_1_is_zero": ("offset_zero", E_OFFSET,
                               "3.1.1.5: repeat offset 1 minus 1 is 0, which the RFC calls corrupt; libzstd makes it 1"),
    "D_nseq_zero_in_two_bytes": ("zero_sequences_wide", E_SEQ_HEADER,
                                 "3.1.1.3.2.1: no sequences is the single byte 0; libzstd reads 0x80 0x00 as zero too and goes on"),
    "libzstd_checksum_frame": (None, E_CHECKSUM,
                               "3.1.1.1.1.4: the checksum flag is refused outright (the reference's Compressor never sets it)"),
    "huffman_literals_of_size_0": (None, E_LITERALS,
                                   "3.1.1.3.1.1: Huffman literals of Regenerated_Size 0 code nothing; libzstd 1.4.8 decodes a "
                                   "1-stream one"),
}

# What libzstd 1.4.8 (version number 10408) answers; True: it decodes the frame.
LIBZSTD_1_4_8 = {
    "D_nseq_zero_in_two_bytes": True,   # 0x80 0x00 as a sequence count
    "E_window_above_bound": False,      # a window descriptor above 2^31
    "E_window_at_bound": True,
    "D_offset_beyond_window": True,     # an offset beyond the window but inside the output (one-shot decoding keeps no window)
}

HUFFMAN_CLASSES = ("lit_header3_1stream", "lit_header3_4stream", "lit_header4", "lit_header5", "huf_weights_direct",
                   "huf_weights_fse", "lit_huffman_repeat")

HUF_SIZE_0 = b"\x00\x00" + zc.block(2, b"\x02\xc0\x00\x80\x10\x01\x00", True)  # of tests/test_zstd_decode_host.py


def libzstd_checksum_frame(data):
    """A magicless libzstd frame with the content checksum."""
    L = zstd_ref.lib()
    c = L.ZSTD_createCCtx()
    try:
        for p, v in [(zstd_ref.ZSTD_c_contentSizeFlag, 0), (zstd_ref.ZSTD_c_checksumFlag, 1),
                     (zstd_ref.ZSTD_c_format, zstd_ref.ZSTD_f_zstd1_magicless)]:
            assert not L.ZSTD_isError(L.ZSTD_CCtx_setParameter(c, p, v))
        cap = L.ZSTD_compressBound(len(data))
        out = ctypes.create_string_buffer(cap)
        n = L.ZSTD_compress2(c, out, cap, data, len(data))
        assert not L.ZSTD_isError(n)
        return out.raw[:n]
    finally:
        L.ZSTD_freeCCtx(c)


def libzstd(frame, cap):
    try:
        return zstd_ref.decompress(frame, cap)
    except ValueError:
        return None


@pytest.fixture(scope="module")
def verdicts():
    """libzstd's answer per planted case: bytes or None.  DIVERGENCES and LIBZSTD_1_4_8 record where
    release 1.4.8 is laxer than the RFC, so every test that compares with libzstd holds that release."""
    assert zstd_ref.version() == 10408, ("the system libzstd is %d, not 1.4.8 (10408): record DIVERGENCES and LIBZSTD_1_4_8 "
                                         "of tests/test_zstd_plant.py anew for it" % zstd_ref.version())
    return {c.name: libzstd(c.frame, c.cap) for c in pc.all_cases()}


def test_writer_reads_back():
    """The FSE table descriptions and bitstreams the writer emits are read back by zstd_frames."""
    for counts, log in (((8, 8, 8, 8), 5), ((4,) * 8, 5), ((8, 8, 8, 4, -1, 1, 2), 5), ((30, 0, 0, 0, 0, 0, 0, 1, -1), 5),
                        ((1, 0, 60, 0, 0, 0, 2, -1), 6), (zstd_frames.LL_DEFAULT, 6), (zstd_frames.OF_DEFAULT, 5)):
        b = zstd_plant.write_ncount(log, counts)
        assert zstd_frames._read_ncount(b + b"\xff", 0, len(b) + 1, 255, 9) == (log, list(counts), len(b))
    assert zstd_plant.header_bytes(zstd_plant.header(), 0) == b"\x00\x00"
    assert zstd_plant.header_bytes(zstd_plant.header(single=True, fcs_width=2, did=b"\0\0"), 300) == b"\x62\0\0\x2c\x00"


def test_libzstd_and_replay_agree(verdicts):
    disagree = set()
    for c in pc.all_cases():
        lz = verdicts[c.name]
        if (lz is not None) != c.ok:
            disagree.add(c.name)
            assert lz is not None, (c.name, "replay accepts what libzstd refuses")
        elif c.ok:
            assert lz == c.want, (c.name, "libzstd and replay regenerate different bytes")
    planted = {k for k, v in DIVERGENCES.items() if v[0] is not None}
    assert disagree == planted, (sorted(disagree - planted), sorted(planted - disagree))
    for k in planted:
        assert {c.name: c.want for c in pc.all_cases()}[k] == DIVERGENCES[k][0]
    assert sum(c.ok for c in pc.all_cases()) >= 300 and sum(not c.ok for c in pc.all_cases()) >= 25


def test_libzstd_1_4_8_verdicts(verdicts):
    assert {k: verdicts[k] is not None for k in LIBZSTD_1_4_8} == LIBZSTD_1_4_8


def test_classifier_reads_every_accepted_frame():
    for c in pc.all_cases():
        if not c.ok and not c.classes:
            continue
        # raises unless it consumes the frame exactly; a refused case that names classes is refused for
        # what it regenerates (an offset, a size), not for its form, and must be read too
        blocks = zstd_frames.classify(c.frame, any_header=True)
        assert not c.ok or sum(b["regen"] for b in blocks) == len(c.want), c.name
        got = zstd_frames.decoder_classes(blocks)
        assert c.classes <= got, (c.name, sorted(c.classes - got))
        assert got <= set(zstd_frames.DECODER_CLASSES), (c.name, sorted(got - set(zstd_frames.DECODER_CLASSES)))
    # the header's own refusals
    for name in ("E_reserved_bit", "E_checksum_flag", "E_window_above_bound", "E_dict_id2", "E_wrong_fcs2_+256"):
        c = {c.name: c for c in pc.all_cases()}[name]
        with pytest.raises(ValueError):
            zstd_frames.classify(c.frame, any_header=True)
    # the default reading is unchanged: only descriptor 0x00
    with pytest.raises(ValueError):
        zstd_frames.classify(b"\x20\x05" + zc.block(0, b"hello", True))
    assert zstd_frames.classify(b"\x20\x05" + zc.block(0, b"hello", True), any_header=True)[0]["header"]["fcs"] == 5


def test_host_run_under_sanitizers(tmp_path, verdicts):
    """Every planted frame through the decoder core under ASan/UBSan (a stand-alone program; a
    report fails run_host): the verdict and bytes of libzstd, except the rows of DIVERGENCES."""
    exe = zc.build_host(tmp_path)
    cases = pc.all_cases()
    extra = [("libzstd_checksum_frame", libzstd_checksum_frame(b"hello, hello, hello" * 9), 256, b"hello, hello, hello" * 9),
             ("huffman_literals_of_size_0", HUF_SIZE_0, 16, b"")]
    res = zc.run_host(exe, [(c.frame, c.cap) for c in cases] + [(f, cap) for _, f, cap, _ in extra], tmp_path, "plant")
    for c, (e, out, canary) in zip(cases, res):
        assert canary, c.name
        assert e == want_err(c), (c.name, e, c.want if not c.ok else "ok")
        lz = verdicts[c.name]
        if c.name in DIVERGENCES:
            assert lz is not None and e == DIVERGENCES[c.name][1], (c.name, e)
        else:
            assert (e == 0) == (lz is not None), (c.name, e)
            assert e != 0 or out == lz == c.want, c.name
    for (name, f, cap, data), (e, out, canary) in zip(extra, res[len(cases):]):
        assert canary and e == DIVERGENCES[name][1], (name, e)
        assert libzstd(f, cap) == data, name
    assert len(DIVERGENCES) == 5


def test_census_reaches_every_decoder_class():
    """Planted frames + libzstd's corpus frames reach every class name; the Huffman classes, which
    the writer cannot plant, are all reached by libzstd's frames alone."""
    count = dict.fromkeys(zstd_frames.DECODER_CLASSES, 0)
    corpus = dict(count)
    for c in pc.all_cases():
        try:  # a refused frame counts where it is refused for what it regenerates (an offset, a size), not for its form
            blocks = zstd_frames.classify(c.frame, any_header=True)
        except ValueError:
            assert not c.ok
            continue
        for k in zstd_frames.decoder_classes(blocks):
            count[k] += 1
    for _, _, _, f in zc.frames():
        for k in zstd_frames.decoder_classes(zstd_frames.classify(f, any_header=True)):
            corpus[k] += 1
    assert [k for k in HUFFMAN_CLASSES if corpus[k] == 0] == []
    assert [k for k in count if count[k] + corpus[k] == 0] == []
    # and what only planting reaches
    only_planted = sorted(k for k in count if corpus[k] == 0)
    print("classes the libzstd corpus does not reach:", only_planted)
    assert "long_offset" in only_planted and "single_segment" in only_planted


# ------------------------------------------------------------------ the barrier rule
# matches that wait, per frame of group C (the first sequence of each waits once)
C_WAITS = {"C_ends_at_dirty": 1, "C_one_before_dirty": 1, "C_one_past_dirty": 2, "C_own_literals": 2,
           "C_own_literals_overlap": 2, "C_ll0_reads_first_match": 2, "C_far_back_after_many_stores": 2, "C_chain_200": 200}


def run_hazard(tmp_path, cases):
    """tests/cpp/zstd_dec_hazard.cpp under ASan/UBSan over [(frame, cap)] ->
    [(error, bytes, waits, unsynced reads, needless waits)]"""
    exe = os.path.join(str(tmp_path), "zstd_dec_hazard")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + zc.SAN + [os.path.join(HERE, "cpp", "zstd_dec_hazard.cpp"), "-o", exe])
    inp, outp = os.path.join(str(tmp_path), "hazard.in"), os.path.join(str(tmp_path), "hazard.out")
    with open(inp, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for frame, cap in cases:
            f.write(struct.pack("<II", len(frame), cap) + frame)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe, inp, outp], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    raw, out, at = open(outp, "rb").read(), [], 0
    for _ in cases:
        e, n, waits, unsynced, needless = struct.unpack_from("<iIIII", raw, at)
        at += 20
        out.append((e, raw[at:at + n], waits, unsynced, needless))
        at += n
    assert at == len(raw)
    return out


def test_barrier_rule_on_the_host(tmp_path):
    """zd::Hazard is the rule WaveExec::match asks before it reads (bw_zstd_dec.hip).  A device run
    cannot show that a wait is needed: a chip may make a wave's stores visible to its later loads
    anyway.  So the rule itself is held, on the host, to what was really stored: over every planted
    frame and a part of the libzstd corpus no match reads a byte stored since the last barrier
    without waiting, none waits without such a byte in its source, and the frames of group C --
    built on either side of the comparison -- wait exactly where their docstring
    (tests/test_gpu_zstd_planted.py, C) says."""
    cases = pc.all_cases()
    corpus = zc.frames()[::9]
    res = run_hazard(tmp_path, [(c.frame, c.cap) for c in cases] + [(f, len(src)) for _, _, src, f in corpus])
    for c, (e, out, waits, unsynced, needless) in zip(cases, res):
        assert e == want_err(c) and (e != 0 or out == c.want), (c.name, e)
        assert (unsynced, needless) == (0, 0), (c.name, unsynced, needless)
        if c.name in C_WAITS:
            assert waits == C_WAITS[c.name], (c.name, waits)
    assert set(C_WAITS) == {c.name for c in pc.group_c()}
    for (name, lv, src, _), (e, out, waits, unsynced, needless) in zip(corpus, res[len(cases):]):
        assert e == 0 and out == src and (unsynced, needless) == (0, 0), (name, lv, e, unsynced, needless)
    assert sum(r[2] for r in res[len(cases):]) > 1000  # the corpus does make matches wait
