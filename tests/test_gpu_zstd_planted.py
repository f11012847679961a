"""k_zd_frame (backuwup_amd/csrc/bw_zstd_dec.hip) over planted frames: the device-only code of
WaveExec -- copy's head, vector body and tail, fill, the two forms of match and the `dirty` rule that
decides whether a match waits at a barrier -- the header and block forms no compressor here emits,
and the state a wave carries from one frame to the next.  Every frame was pinned on the CPU first
(tests/test_zstd_plant.py: libzstd, replay and the sanitized host run of the same core agree on
it); here the bytes expected are replay's, ok[] must be the host run's verdict, and a canary lies
behind every output range.  All comparisons are exact."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_corpus  # noqa: E402
import zstd_decode_cases as zc  # noqa: E402
import zstd_frames  # noqa: E402
import zstd_plant as zp  # noqa: E402
import zstd_plant_cases as pc  # noqa: E402
import zstd_ref  # noqa: E402
from zstd_plant_cases import E_LITERALS, E_SEQ_HEADER, want_err  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")]
CANARY = 64


def decode_placed(ctx, items):
    """One ragged batch through bw_zstd_decompress_device, laid out like _decode_device of
    tests/test_gpu_zstd_decode.py (frames at odd source offsets, a canary behind every output
    range), with the residue mod 16 of a frame's source and destination address chosen where asked.
    items: [(frame, cap, src residue or None, dst residue or None)] -> [bytes or None]; every byte
    of the destination outside the ranges written must be untouched."""
    import torch
    so, at = [], 1
    for f, _, sr, _ in items:
        if sr is not None:
            at += (sr - at) % 16
        so.append(at)
        at += len(f) + 3
    src = np.full(at + 16, 0x5A, dtype=np.uint8)
    for o, (f, _, _, _) in zip(so, items):
        src[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    do, at = [], 5
    for _, cap, _, dr in items:
        if dr is not None:
            at += (dr - at) % 16
        do.append(at)
        at += cap + CANARY
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0  # the residues above are those of the addresses
    caps = [c for _, c, _, _ in items]
    ol, ok = ctx.zstd_decompress_device(d_src.data_ptr(), so, [len(f) for f, _, _, _ in items], d_dst.data_ptr(), do, caps)
    out = d_dst.cpu().numpy()
    clean = out != 0xA5  # -> where a byte outside every capacity was written
    for o, c in zip(do, caps):
        clean[o:o + c] = False
    assert not clean.any(), "a byte outside an output range was written (first at %d)" % int(np.argmax(clean))
    res = []
    for i in range(len(items)):
        assert ok[i] or int(ol[i]) == 0, i
        res.append(out[do[i]:do[i] + int(ol[i])].tobytes() if ok[i] else None)
    return res


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The decoder core's verdict per planted case from a plain host build (the sanitized run is the
    CPU test's): {name: (zd::Err, bytes)}."""
    d = tmp_path_factory.mktemp("zd_plant_host")
    exe = zc.build_host(d, sanitize=False)
    cases = pc.all_cases()
    res = zc.run_host(exe, [(c.frame, c.cap) for c in cases], d, "plant", sanitized=False)
    for c, (e, out, canary) in zip(cases, res):
        assert canary and e == want_err(c) and (e != 0 or out == c.want), (c.name, e)
    return exe, d, {c.name: (e, out) for c, (e, out, _) in zip(cases, res)}


def check(ctx, host, placed):
    """placed: [(case, src residue, dst residue)]: the device's ok[] is the host run's verdict and
    the bytes are replay's."""
    got = decode_placed(ctx, [(c.frame, c.cap, sr, dr) for c, sr, dr in placed])
    for (c, sr, dr), b in zip(placed, got):
        e, _ = host[2][c.name]
        assert (b is not None) == (e == 0) == c.ok, (c.name, sr, dr, e)
        assert b is None or b == c.want, (c.name, sr, dr, "bytes differ from replay's")


def test_gpu_a_copy_geometry(ctx, host):
    """A.  Every frame of group A (raw and RLE literals of 43 lengths behind a 17-byte raw block)
    at every destination residue mod 16, so that WaveExec::copy -- which aligns the destination --
    runs with a head of every length 0..15 and, by the 32 lengths from 1024, with every tail 0..15
    at every head; lengths 255 / 256 / 257 take both sides of n >= 256, 256..1023 give some lanes
    one vector and the others none, 1024 + k give some lanes a second.  The literals are read from
    the frame: for each frame the source residue runs through all 16 as well (5 * residue + case).
    (The head only chooses where the 16-byte stores start, and Vec16 is packed: a head taken from
    the source instead is slower, not wrong, and passes.  What fails here is a head, body or tail
    that drops, repeats or misplaces a byte.)"""
    placed = [(c, (5 * dr + i) % 16, dr) for i, c in enumerate(pc.group_a()) for dr in range(16)]
    # the geometry reached, from the layout alone: the literals land at dst_off + 17
    raw = [(c, dr) for c, _, dr in placed if c.name.startswith("A_raw")]
    lens = {c.name: len(c.blocks[1][1]["lits"]) - 5 for c, _ in raw}
    reached = {((-(dr + 17)) & 15, (lens[c.name] - ((-(dr + 17)) & 15)) & 15) for c, dr in raw if lens[c.name] >= 256}
    assert reached == {(h, t) for h in range(16) for t in range(16)}
    assert {lens[c.name] for c, _ in raw} >= {0, 1, 15, 16, 17, 255, 256, 257, 271, 272, 1023, 1024}
    assert {sr for _, sr, _ in placed} == set(range(16))
    check(ctx, host, placed)


def test_gpu_b_match_forms(ctx, host):
    """B.  off x ml over pc.B_OFF x pc.B_ML with off <= ll: off < ml is the overlapped s[i % o]
    loop, off >= ml goes through copy (from ml 256 on its vector path, with a source in the output
    at any alignment); the furthest valid offset and one past it; the longest match length code with
    extra bits up to where it fills a 128 KiB block, and one byte more (E_BLOCK_SIZE with room, E_DST
    where the capacity is the bound).  Each frame at three destination residues."""
    placed = [(c, None, (7 * i + k) % 16) for i, c in enumerate(pc.group_b()) for k in (0, 5, 11)]
    assert {c.name for c in pc.group_b() if not c.ok} == {"B_one_past_furthest", "B_ml_longest_plus_1",
                                                         "B_ml_longest_plus_1_cap", "B_offset_code_26"}
    assert (host[2]["B_ml_longest_plus_1"][0], host[2]["B_ml_longest_plus_1_cap"][0]) == (14, 15)
    check(ctx, host, placed)


def test_gpu_c_barrier_decision(ctx, host):
    """C.  WaveExec::match waits for the wave's earlier stores iff `dirty && s + span > dirty`
    (dirty: the first address stored since the last barrier; span = min(off, ml)).  In every frame
    of group C the first sequence (64 literals, a match of 8 at offset 64) waits and then stores
    [64, 72), so dirty = 64 when the second sequence's match (at 80, after 8 literals) decides:
      C_ends_at_dirty       source [48, 64): s + span == dirty, the last byte synchronized -- no wait
      C_one_before_dirty    source [48, 63): below it
      C_one_past_dirty      source [48, 65): s + span == dirty + 1, one unsynchronized byte
      C_own_literals        source [74, 78): the literals this sequence just stored
      C_own_literals_overlap  off 5 < ml 40: span = off, the source ends where the match starts
      C_ll0_reads_first_match  ll 0: the source is exactly the first match's bytes
      C_far_back_after_many_stores  100 sequences whose sources end at or below 64 (every fifth
                            exactly at it) pile up stores without a wait, then a match from [3, 33),
                            then one from the three newest bytes
      C_chain_200           200 short sequences that each read what the one before stored
    A wrong decision reads stale bytes, so the exact comparison is the check.  Every frame at every
    destination residue: the 128-byte lines the stale bytes would sit in move with it.
    (A chip may make a wave's stores visible to its own later loads without any wait, and then a
    match that never waits passes here.  The rule itself -- zd::Hazard -- is held to what was really
    stored by tests/test_zstd_plant.py::test_barrier_rule_on_the_host, over these same frames.)"""
    check(ctx, host, [(c, None, dr) for c in pc.group_c() for dr in range(16)])


def test_gpu_d_state_carried_in_a_frame(ctx, host):
    """D.  Multi-block frames: every repeat-offset index, offsets kept over raw and RLE blocks,
    Repeat_Mode after predefined, RLE and FSE tables (and refused in a first block), sequence counts
    of 127, 128, 0x7EFF and 0x7F00, literal headers wider than needed."""
    names = {c.name for c in pc.group_d()}
    assert {"D_every_repeat_index", "D_rep1_minus_1_is_zero", "D_offsets_over_raw_and_rle", "D_repeat_after_predefined",
            "D_repeat_after_rle", "D_repeat_after_fse", "D_repeat_in_first_block_ll", "D_nseq_127", "D_nseq_128",
            "D_nseq_0x7EFF", "D_nseq_0x7F00"} <= names
    check(ctx, host, [(c, None, None) for c in pc.group_d()])


def test_gpu_e_header_forms(ctx, host):
    """E.  Single-segment or window x content-size width x dictionary-id width, wrong content
    sizes (the 2-byte field's +256 among them), a dictionary id, the reserved bit, the window at
    its bound and above it.  The errors expected are the host run's."""
    assert sum(c.ok for c in pc.group_e()) == 33 and host[2]["E_wrong_fcs2_+256"][0] == 16
    check(ctx, host, [(c, None, None) for c in pc.group_e()])


# ------------------------------------------------------------------ F
def _max_waves():
    text = open(os.path.join(zc.ROOT, "backuwup_amd", "csrc", "bw_unpack.h")).read()
    return int(re.search(r"constexpr uint32_t ZD_MAX_WAVES = (\d+);", text).group(1))


def carried_state_frames():
    """The three leaders and their probes.  A leader runs on a wave first, its probe 2048 frames on.
    -> [(leader frame, leader blob, probe frame, what the probe must give: bytes, or None = refused)]"""
    out = []
    # 1. treeless literals: two blocks of i.i.d. skewed bytes; libzstd at level 1 writes the second with the
    # first's Huffman tree and no sequences.  Lifted into a frame of its own it has no tree: refused
    # -- and decoded in full by a wave that kept huf_valid and the tree from the leader.
    blob = zstd_corpus.edge_blob("skew_mid", 128 * 1024 + 20000, 3)
    lead = zstd_ref.compress(blob, 1)
    b = zstd_frames.classify(lead)
    assert len(b) == 2 and b[0]["lit_type"] == "huffman" and b[1]["lit_type"] == "huffman_repeat" and b[1]["nseq"] == 0
    at = 2 + 3 + b[0]["body"] + 3
    out.append((lead, blob, lead[:2] + zc.block(2, lead[at:at + b[1]["body"]], True), None))
    # 2. Repeat_Mode tables in a first block.  The leader is planted: its compressed block uses the
    # predefined tables, which sets the three valid flags and leaves those tables in LDS -- the
    # tables the writer codes the probe's bitstream with.  So a wave that kept the flags decodes the
    # probe in full (ok = 1, not another refusal): the leader's blocks followed by the probe's are a
    # frame libzstd decodes, which is what that wave would be reading.
    seqs = [(2, 4, pc.off(7)), (1, 5, pc.off(100)), (0, 3, pc.off(30))]
    lead2 = pc.Case("F_predefined_leader", [zp.raw(bytes(range(50, 250))), pc._comp(seqs)])
    probe_blocks = [zp.raw(bytes(range(200))), pc._comp([(2, 4, pc.off(7)), (1, 5, pc.off(100))], ll="repeat", of="repeat",
                                                         ml="repeat")]
    probe = pc.Case("F_repeat_mode", probe_blocks)
    assert lead2.ok and probe.want == "repeat_without_table"
    joined = pc.Case("F_leader_then_probe", lead2.blocks + probe_blocks)
    assert joined.ok and joined.frame.endswith(probe.frame[2:]) and zstd_ref.decompress(joined.frame, 4096) == joined.want
    out.append((lead2.frame, lead2.want, probe.frame, None))
    blob = zstd_corpus.blob("text", 6000, 11)
    lead = zstd_ref.compress(blob, 3)
    c = zstd_frames.frame_classes(zstd_frames.classify(lead))
    assert {"lit_huffman", "ll_fse", "of_fse", "ml_fse"} <= c, sorted(c)
    # 3. repeat codes on the initial offsets 1, 4, 8, behind a libzstd frame that built a Huffman tree and all
    # three FSE tables and whose matches moved the offsets
    probe = pc.Case("F_initial_offsets", [zp.comp(b"abcdefghijklmnop", [(4, 5, pc.CODE1), (1, 6, pc.CODE2), (3, 7, pc.CODE3),
                                                                       (0, 3, pc.CODE1)])])
    assert probe.ok
    out.append((lead, blob, probe.frame, probe.want))
    return out


def test_gpu_f_state_carried_between_frames_of_a_wave(ctx, host):
    """F.  zd_run (bw_capi_pack.hip) launches waves = min(n, ZD_MAX_WAVES) and frame i runs on wave
    i % waves, so in a batch of 2048 + 64 frames, frame 2048 + k is decoded in the LDS State and
    literals buffer that frame k left.  Frames 0..63 are the leaders (libzstd frames that build a
    Huffman tree and FSE tables and move the repeat offsets, and a planted one that leaves the
    predefined tables valid), 64..2047 tiny raw frames, and 2048 + k is the probe
    of frame k: treeless literals and Repeat_Mode tables in a first block (refused: the host run's
    verdict on the frame alone), or repeat codes that must find the offsets 1, 4, 8 (replay's bytes).
    The test rests on ZD_MAX_WAVES = 2048, read from bw_unpack.h."""
    waves = _max_waves()
    assert waves == 2048
    trio = carried_state_frames()
    exe, d, _ = host
    for k, (lead, blob, probe, want) in enumerate(trio):  # each probe alone on the host: a fresh State
        (e, out, canary), = zc.run_host(exe, [(probe, 4096)], d, "f%d" % k, sanitized=False)
        assert canary and (e, out) == ((0, want) if want is not None else ((E_LITERALS, E_SEQ_HEADER)[k], b"")), (k, e)
        if want is None:
            with pytest.raises(ValueError):
                zstd_ref.decompress(probe, 1 << 20)
        else:
            assert zstd_ref.decompress(probe, 4096) == want
    tiny = b"\x00\x00" + zc.block(0, b"tiny", True)
    items = [(trio[k % 3][0], len(trio[k % 3][1]), None, None) for k in range(64)]
    items += [(tiny, 4, None, None)] * (waves - 64)
    items += [(trio[k % 3][2], 160 * 1024 if k % 3 == 0 else 4096, None, None) for k in range(64)]
    assert len(items) == waves + 64
    got = decode_placed(ctx, items)
    for k in range(64):
        assert got[k] == trio[k % 3][1], k
        assert got[waves + k] == trio[k % 3][3], (k, "a probe saw the state of the frame before it on its wave")
    assert all(g == b"tiny" for g in got[64:waves])
