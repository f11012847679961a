"""The zstd decoder core (backuwup_amd/csrc/bw_zstd_dec_core.h) on the CPU, as a stand-alone program
under AddressSanitizer and UndefinedBehaviorSanitizer (tests/cpp/zstd_dec_host.cpp; a child
process, nothing preloaded): the code the kernel runs, over valid frames of every format class and
over damaged ones, before any damaged frame goes to a GPU.

Frames come from the system libzstd (1.4.8 here) at levels 1, 3, 7, 13 and 19; modes are counted
with tests/zstd_frames.py."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_decode_cases as zc  # noqa: E402
import zstd_frames  # noqa: E402
import zstd_ref  # noqa: E402

pytestmark = pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")

# Where the decoder may refuse a frame libzstd 1.4.8 decodes (error names of zd::Err), each with
# the clause of RFC 8878 the frame breaks.  Anything else refused is a failure.
STRICTER_THAN_LIBZSTD = {
    3: "E_CHECKSUM: 3.1.1.1.1.4 Content_Checksum_Flag -- refused outright (the reference never sets it)",
    4: "E_BLOCK: 3.1.1.2.3 Block_Size above Block_Maximum_Size (libzstd's one-shot path does not bound raw/RLE blocks)",
    5: "E_TRAILING: concatenated frames are out of scope (3.1 allows them; the reference writes one frame per blob)",
    6: "E_LITERALS: 3.1.1.3.1.1 a Huffman-coded literals section of Regenerated_Size 0 codes nothing; libzstd 1.4.8 "
       "decodes a 1-stream one, its 4-stream path and tests/zstd_frames.py refuse it",
    7: "E_HUF_TABLE: 4.2.1 Max_Number_of_Bits is 11 (libzstd builds 12-bit tables); 4.2.1.2 the weights' FSE "
       "stream must hold its two initial states",
    8: "E_HUF_STREAM: 4.2.2 the fourth stream holds the remainder of the regenerated size; 4.2.2 / 4.1 every "
       "stream is consumed exactly (libzstd 1.4.8 decodes some streams that are not)",
    9: "E_SEQ_HEADER: 3.1.1.3.2.1 reserved bits of Symbol_Compression_Modes; zero sequences in a two-byte count",
    11: "E_SEQ_STREAM: 4.1 / 3.1.1.3.2.1.2 the bitstream is consumed exactly (libzstd 1.4.8 lets it run past its start)",
    13: "E_OFFSET: 3.1.1.5 an offset of 0 (repeat offset 1 minus 1) is corrupt (libzstd forces it to 1)",
    14: "E_BLOCK_SIZE: 3.1.1.2.4 a block regenerates at most Block_Maximum_Size",
}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("zd_host")
    return zc.build_host(d), d


def test_census_corpus_decodes_and_reaches_every_class(host):
    exe, d = host
    frames = zc.frames()
    assert len(zc.blobs()) == 73
    count = zstd_frames.census(f for _, _, _, f in frames)
    missing = sorted(k for k, v in count.items() if v == 0)
    assert missing == ["long_offset"], missing  # needs an offset above 32 MiB: unreachable for 3 MiB blobs
    res = zc.run_host(exe, [(f, zc.CAP) for _, _, _, f in frames], d, "census")
    for (name, lv, src, _), (e, out, canary) in zip(frames, res):
        assert e == 0 and canary, (name, lv, e)
        assert out == src, (name, lv)
    # exact capacity is enough
    res = zc.run_host(exe, [(f, len(src)) for _, _, src, f in frames[::7]], d, "exact")
    for (name, lv, src, _), (e, out, canary) in zip(frames[::7], res):
        assert e == 0 and canary and out == src, (name, lv, e)


def check_mutations(results):
    """The four requirements over decoder results [(error, bytes, canary)] of zc.mutations()."""
    muts, verdicts = zc.mutations(), zc.libzstd_verdicts()
    assert len(muts) == len(results) == len(verdicts)
    rejected = sum(v is None for v in verdicts)
    accepted = len(verdicts) - rejected
    assert rejected >= 50 and accepted >= 50, (rejected, accepted)
    stricter = []
    for (name, kind, _), ref, (e, out, canary) in zip(muts, verdicts, results):
        assert canary, (name, kind)
        if ref is None:
            assert e != 0, (name, kind, "libzstd rejects, the decoder accepts")
        elif e == 0:
            assert out == ref, (name, kind, "decoded bytes differ from libzstd's")
        else:
            assert e in STRICTER_THAN_LIBZSTD, (name, kind, e, "refused for a cause that is not listed")
            stricter.append((name, e))
    print("mutations: %d, libzstd rejects %d, accepts %d; refused although libzstd accepts: %d %s"
          % (len(muts), rejected, accepted, len(stricter), stricter))
    assert len(stricter) <= 0.05 * accepted, (len(stricter), accepted, stricter)


def test_mutated_frames(host):
    exe, d = host
    muts = zc.mutations()
    assert len(muts) == 928  # 58 blobs under 300,000 bytes x 2 levels x 8
    check_mutations(zc.run_host(exe, [(m, zc.CAP) for _, _, m in muts], d, "mut"))


def test_hand_made_frames(host):
    exe, d = host
    cap = zc.CAP
    a3 = b"a" * cap
    full = zc.frame_3mib_plus_1()
    # 3 MiB exactly (the same frame without its last byte-long block) decodes; one more byte does not
    ok3 = bytearray(b"\x00\x58")
    for k in range(24):
        ok3 += zc.block(1, b"a", k == 23, 128 * 1024)
    short = zstd_ref.compress(b"hello, hello, hello, hello, world" * 40, 3)
    n_short = 33 * 40
    cases = [(bytes(ok3), cap), (full, cap), (zc.offset_at_output_frame(), 64), (zc.offset_past_output_frame(), 64),
             (zc.offset_code_31_frame(), 64), (short, n_short), (short, n_short - 1),
             (b"\x01\x00\x00\x01\x00\x00", 16),                  # dictionary id 0 in a 1-byte field: fine
             (b"\x01\x00\x07\x01\x00\x00", 16),                  # dictionary id 7
             (b"\x04\x00\x01\x00\x00", 16),                      # checksum flag
             (b"\x00\x00\x07\x00\x00", 16),                      # reserved block type
             (b"\x00\x00\x01\x00\x00\x00", 16),                  # a byte after the last block
             (b"\x20\x05" + zc.block(0, b"hello", True), 16),    # single segment, content size 5
             (b"\x20\x06" + zc.block(0, b"hello", True), 16),    # content size 6, 5 regenerated
             (b"", 16), (b"\x00", 16),
             # one Huffman stream (a two-symbol tree, then only the end mark) that regenerates 0 literals
             (b"\x00\x00" + zc.block(2, b"\x02\xc0\x00\x80\x10\x01\x00", True), 16)]
    r = zc.run_host(exe, cases, d, "hand")
    assert all(c for _, _, c in r)
    assert r[0][0] == 0 and r[0][1] == a3
    assert r[1][0] == 15                                         # E_DST: 3 MiB + 1
    assert r[2][0] == 0 and r[2][1] == b"abcdefghabcd"
    assert r[3][0] == 13 and r[4][0] == 13                       # E_OFFSET
    assert r[5][0] == 0 and r[5][1] == b"hello, hello, hello, hello, world" * 40
    assert r[6][0] == 15                                         # dst_cap one byte short (canary checked above)
    assert r[7][0] == 0 and r[7][1] == b""
    assert r[8][0] == 2 and r[9][0] == 3 and r[10][0] == 4 and r[11][0] == 5
    assert r[12][0] == 0 and r[12][1] == b"hello"
    assert r[13][0] == 16
    assert r[14][0] == 0 and r[14][1] == b""                    # no bytes: libzstd returns 0, and so does the reference
    assert zstd_ref.decompress(b"", 16) == b""
    assert r[15][0] == 1
    assert r[16][0] == 6                                         # E_LITERALS (listed above: libzstd 1.4.8 decodes it)
    assert zstd_ref.decompress(cases[16][0], 16) == b""
    # libzstd agrees on the ones it can be asked about
    assert zstd_ref.decompress(zc.offset_at_output_frame(), 64) == b"abcdefghabcd"
    for bad in (zc.offset_past_output_frame(), zc.offset_code_31_frame(), full):
        with pytest.raises(ValueError):
            zstd_ref.decompress(bad, cap)
