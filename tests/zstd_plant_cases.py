"""The planted frames of tests/test_zstd_plant.py (CPU) and tests/test_gpu_zstd_planted.py (device),
built with tests/zstd_plant.py.  Groups follow the device tests: A copy geometry, B match forms,
C the barrier decision of WaveExec::match, D state carried inside a frame, E header forms.
(F, state carried between frames of one wave, is a batch layout and lives in the device test.)"""
import functools
import random

import zstd_plant as zp

CODE1, CODE2, CODE3 = 1, 2, 3  # offset_value: the repeat codes

# zd::Err (backuwup_amd/csrc/bw_zstd_dec_core.h), and the one the decoder gives for each rule replay names
E_HEADER, E_DICT, E_CHECKSUM, E_LITERALS, E_SEQ_HEADER, E_LIT_OVERRUN, E_OFFSET, E_BLOCK_SIZE, E_DST, E_CONTENT_SIZE = \
    1, 2, 3, 6, 9, 12, 13, 14, 15, 16
RULE_ERR = {"reserved_bit": E_HEADER, "window_too_large": E_HEADER, "dict_id": E_DICT, "checksum": E_CHECKSUM,
            "content_size": E_CONTENT_SIZE, "repeat_without_table": E_SEQ_HEADER, "zero_sequences_wide": E_SEQ_HEADER,
            "literals": E_LIT_OVERRUN, "offset_zero": E_OFFSET, "offset_past_output": E_OFFSET, "block_size": E_BLOCK_SIZE}


def _bytes(seed, n):
    return random.Random(seed).randbytes(n)


def off(o):
    """offset_value of a real offset"""
    return o + 3


class Case:
    def __init__(self, name, blocks, header=None, cap=None, classes=()):
        self.name, self.blocks = name, blocks
        self.header = header or zp.header(window=0x38)  # a 128 KiB window
        self.frame = zp.frame(self.header, blocks)
        self.want = zp.replay(blocks, self.header)  # bytes, or the rule broken
        self.cap = cap if cap is not None else (len(self.want) + 37 if isinstance(self.want, bytes) else 4096)
        self.classes = frozenset(classes)  # class names of zstd_frames.DECODER_CLASSES the case is built to reach

    @property
    def ok(self):
        return isinstance(self.want, bytes)

    def __repr__(self):
        return "Case(%s)" % self.name


def want_err(c):
    """The zd::Err the decoder must give for a planted case."""
    if c.ok:
        return 0
    if c.want == "block_size" and c.cap <= zp.BLOCK_MAX:
        return E_DST  # the capacity is the nearer bound
    return RULE_ERR[c.want]


def one_seq(name, ll, ml, ov, prefix=0, tail=5, rle=False, **kw):
    """[a raw block of `prefix` bytes,] one compressed block: ll + tail literals, one sequence."""
    seed = hash((ll, ml, ov, prefix)) & 0xFFFFFF
    blocks = [zp.raw(_bytes(seed, prefix))] if prefix else []
    if rle:
        blocks.append(zp.comp(lit_rle=(0xC3, ll + tail), seqs=[(ll, ml, ov)]))
    else:
        blocks.append(zp.comp(_bytes(seed + 1, ll + tail), [(ll, ml, ov)]))
    return Case(name, blocks, **kw)


# ------------------------------------------------------------------ A
A_LL = (0, 1, 15, 16, 17, 255, 256, 257, 271, 272, 1023) + tuple(1024 + k for k in range(32))


@functools.lru_cache(maxsize=None)
def group_a():
    """Raw and RLE literals of every length of A_LL behind a 17-byte raw block, one sequence whose
    match (4 bytes at offset 7) keeps out of the way.  The device test places each frame at every
    destination residue mod 16, which sweeps WaveExec::copy's head over 0..15; the 32 lengths from
    1024 sweep its tail over 0..15 at every head, and give some lanes a second vector."""
    out = []
    for ll in A_LL:
        out.append(one_seq("A_raw_ll%d" % ll, ll, 4, off(7), prefix=17))
        out.append(one_seq("A_rle_ll%d" % ll, ll, 4, off(7), prefix=17, rle=True))
    return out


# ------------------------------------------------------------------ B
B_OFF = (1, 2, 3, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257)
B_ML = (3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4099)
ML_LONGEST = zp.BLOCK_MAX - 1  # code 52 (base 65,539) + 65,532 of the 65,535 its extra bits hold: with one literal the block is full


@functools.lru_cache(maxsize=None)
def group_b():
    out = []
    for o in B_OFF:
        for ml in B_ML:
            ll = o + (o + ml) % 3  # off <= ll
            out.append(one_seq("B_off%d_ml%d" % (o, ml), ll, ml, off(o), tail=2))
    out.append(one_seq("B_furthest", 6, 5, off(16), prefix=10))          # off == o + ll
    out.append(one_seq("B_one_past_furthest", 6, 5, off(17), prefix=10))  # refused
    out.append(one_seq("B_ml_longest", 1, ML_LONGEST, off(1), tail=0, classes=["ml_code_52"]))
    out.append(one_seq("B_ml_longest_plus_1", 1, ML_LONGEST + 1, off(1), tail=0, cap=200000))
    out.append(one_seq("B_ml_longest_plus_1_cap", 1, ML_LONGEST + 1, off(1), tail=0, cap=zp.BLOCK_MAX))
    out.append(one_seq("B_offset_code_26", 8, 3, (1 << 26) + 5, classes=["long_offset", "of_code_ge20"]))
    return out


# ------------------------------------------------------------------ C
def seq_frame(name, seqs, tail=3, **kw):
    n = sum(s[0] for s in seqs) + tail
    return Case(name, [zp.comp(_bytes(len(seqs) * 131 + n, n), seqs)], **kw)


# The first sequence of every C frame: 64 literals at [0, 64) (dirty = 0), a match of 8 from offset
# 64, whose source [0, 8) was stored since the last barrier: it waits, then stores [64, 72), so
# dirty = 64 for the second sequence.
C_FIRST = (64, 8, off(64))


@functools.lru_cache(maxsize=None)
def group_c():
    out = [
        # second sequence: 8 literals at [72, 80), the match at 80
        seq_frame("C_ends_at_dirty", [C_FIRST, (8, 16, off(32))]),        # source [48, 64): s + span == dirty
        seq_frame("C_one_past_dirty", [C_FIRST, (8, 17, off(32))]),       # source [48, 65): s + span == dirty + 1
        seq_frame("C_one_before_dirty", [C_FIRST, (8, 15, off(32))]),     # source [48, 63)
        seq_frame("C_own_literals", [C_FIRST, (8, 4, off(6))]),           # source [74, 78), this sequence's literals
        seq_frame("C_own_literals_overlap", [C_FIRST, (8, 40, off(5))]),  # span = off: the source ends where the match starts
        seq_frame("C_ll0_reads_first_match", [C_FIRST, (0, 9, off(8))]),   # ll 0: the match at 72, source [64, 72) = the first match
    ]
    # 100 sequences whose sources all end at or before 64 (no wait: the stores pile up), one far
    # back, then one that reads the newest bytes
    many = [C_FIRST] + [(4, 4, off(72 + 8 * k + 4 - 60 + (k % 5))) for k in range(100)]
    end = 72 + 800
    many += [(2, 30, off(end + 2 - 3)), (1, 6, off(3)), (0, 5, off(700))]
    out.append(seq_frame("C_far_back_after_many_stores", many))
    # 200 short sequences, each reading the bytes of the one before
    chain = [(4, 3, off(2))] + [(1 + k % 2, 3 + k % 3, off(2 + k % 4)) for k in range(199)]
    out.append(seq_frame("C_chain_200", chain))
    return out


# ------------------------------------------------------------------ D
FSE_LL = ("fse", 5, (8, 8, 8, 8))          # literal lengths 0..3
FSE_OF = ("fse", 5, (4,) * 8)              # offset values 1..255
FSE_ML = ("fse", 5, (8, 8, 8, 4, -1, 1, 2))  # match lengths 3..9


def _lits(seqs, tail=3):
    n = sum(s[0] for s in seqs) + tail
    return _bytes(n * 7 + len(seqs), n)


def _comp(seqs, tail=3, **kw):
    return zp.comp(_lits(seqs, tail), seqs, **kw)


@functools.lru_cache(maxsize=None)
def group_d():
    six = ["rep1", "rep2", "rep3", "rep2_at_ll0", "rep3_at_ll0", "rep1_minus_1"]
    out = [Case("D_every_repeat_index", [zp.raw(_bytes(1, 32)), _comp(
        [(2, 5, off(10)), (3, 4, off(20)), (1, 4, off(6)), (2, 3, CODE1), (2, 3, CODE2), (2, 3, CODE3), (0, 3, CODE1),
         (0, 3, CODE2), (0, 3, CODE3), (1, 7, CODE3), (0, 4, CODE3), (2, 4, CODE1)])], classes=six)]
    out.append(Case("D_initial_offsets", [zp.raw(_bytes(2, 16)), _comp([(1, 3, CODE1), (1, 3, CODE2), (1, 3, CODE3)])]))
    out.append(Case("D_rep1_minus_1_is_zero", [zp.raw(_bytes(3, 8)), _comp([(0, 3, CODE3)])]))
    out.append(Case("D_offsets_over_raw_and_rle", [
        _comp([(8, 4, off(5)), (2, 3, off(9)), (3, 3, off(11))]), zp.raw(_bytes(4, 10)), zp.rle(0x11, 7),
        _comp([(1, 3, CODE3), (1, 3, CODE3), (0, 3, CODE3), (0, 4, CODE1), (2, 3, CODE1)]), zp.rle(0x22, 1),
        _comp([(0, 5, CODE2), (1, 5, CODE2)])], classes=["rle_then_compressed"]))
    # Repeat_Mode after each kind of table; s1 and s2 use the same codes where a table is RLE
    s1 = [(2, 4, off(7)), (1, 5, off(100)), (0, 3, off(30)), (3, 9, CODE1), (2, 7, off(1))]
    s2 = [(3, 9, off(60)), (0, 8, CODE2), (1, 3, off(200)), (2, 6, off(2))]
    r1 = [(2, 4, off(5)), (2, 4, off(6)), (2, 4, off(7))]
    r2 = [(2, 4, off(6)), (2, 4, off(9))]
    pre = zp.raw(_bytes(5, 210))
    rep = {"ll": "repeat", "of": "repeat", "ml": "repeat"}
    out.append(Case("D_repeat_after_predefined", [pre, _comp(s1), _comp(s2, **rep)],
                    classes=["ll_repeat", "of_repeat", "ml_repeat"]))
    out.append(Case("D_repeat_after_rle", [pre, _comp(r1, ll="rle", of="rle", ml="rle"), _comp(r2, **rep)],
                    classes=["ll_rle", "of_rle", "ml_rle"]))
    out.append(Case("D_repeat_after_fse", [pre, _comp(s1, ll=FSE_LL, of=FSE_OF, ml=FSE_ML), _comp(s2, **rep),
                                            zp.raw(b"gap"), _comp(s1, **rep)], classes=["ll_fse", "of_fse", "ml_fse"]))
    out.append(Case("D_repeat_mixed", [pre, _comp(r1, ll=FSE_LL, of="rle", ml="predefined"), _comp(r2, **rep),
                                        _comp(r1, ll="predefined", of=FSE_OF, ml="rle"), _comp(r2, **rep),
                                        _comp(r2, ll="rle", of="repeat", ml=FSE_ML), _comp(r1, **rep)]))
    for t in ("ll", "of", "ml"):
        out.append(Case("D_repeat_in_first_block_" + t, [pre, _comp(s1, **{t: "repeat"})]))
    out.append(Case("D_repeat_after_empty_sequences", [pre, _comp([]), _comp(s1, **rep)]))
    # sequence counts
    for n in (127, 128):
        out.append(Case("D_nseq_%d" % n, [pre, _comp([(1 + k % 3, 3 + k % 5, off(1 + k % 200)) for k in range(n)])],
                        classes=["nseq_header%d" % (1 if n < 128 else 2)]))
    for n in (0x7EFF, 0x7F00):  # all tables RLE: ll 0, ml 3, offset code 2 -- two offset bits per sequence and nothing else
        out.append(Case("D_nseq_0x%X" % n, [zp.raw(_bytes(6, 16)), zp.comp(
            b"end", [(0, 3, off(1 + (k * 7 + k // 5) % 4)) for k in range(n)], ll="rle", of="rle", ml="rle")],
            classes=["nseq_header%d" % (2 if n < 0x7F00 else 3), "nseq_ge7f00" if n >= 0x7F00 else "nseq_lt7f00"]))
    out.append(Case("D_nseq_5_in_two_bytes", [pre, zp.comp(_lits(s1), s1, nseq_width=2)], classes=["nseq_header2"]))
    out.append(Case("D_nseq_zero_in_two_bytes", [pre, zp.comp(b"literals only", [], nseq_width=2)]))
    # literals headers, smallest and wider than needed
    for w in (1, 2, 3):
        out.append(Case("D_lit_raw_header%d" % w, [pre, zp.comp(_lits(r1, 9), r1, lit_width=w)], classes=["lit_raw_header%d" % w]))
        out.append(Case("D_lit_rle_header%d" % w, [pre, zp.comp(lit_rle=(0x7E, 15), seqs=r1, lit_width=w)],
                        classes=["lit_rle_header%d" % w]))
    out.append(Case("D_lit_raw_4096", [zp.comp(_bytes(7, 4096), [(4090, 3, off(4000))])], classes=["lit_raw_header3"]))
    out.append(Case("D_lit_overrun", [zp.comp(b"abcd", [(5, 3, off(1))])]))
    # a 1 KiB window and an offset of 1,500 inside 2,000 bytes of output
    out.append(Case("D_offset_beyond_window", [zp.raw(_bytes(8, 2000)), _comp([(3, 40, off(1500))])],
                    header=zp.header(window=0x00)))
    return out


# ------------------------------------------------------------------ E
def _payload(small):
    if small:  # 170 bytes: a 1-byte content size holds at most 255
        return [zp.raw(_bytes(9, 100)), _comp([(30, 10, off(33))], tail=30)]
    return [zp.raw(_bytes(10, 200)), _comp([(50, 10, off(30))], tail=50)]  # 310 bytes: the 2-byte field starts at 256


@functools.lru_cache(maxsize=None)
def group_e():
    out = []
    for single in (True, False):
        for fw in ((1, 2, 4, 8) if single else (0, 2, 4, 8)):
            for dw in (0, 1, 2, 4):
                h = zp.header(single=single, window=0x38, fcs_width=fw, did=bytes(dw))
                out.append(Case("E_%s_fcs%d_did%d" % ("single" if single else "window", fw, dw), _payload(fw == 1), header=h,
                                classes=["single_segment" if single else "window_descriptor", "fcs_%d" % fw,
                                         "dict_id_%d" % dw]))
    for fw, size in ((1, 170), (2, 310), (4, 310), (8, 310)):
        for delta in (1, -1) + ((256,) if fw == 2 else ()):
            # the 2-byte field: +256 is the value a reader that forgets the field's bias accepts
            h = zp.header(single=True, fcs_width=fw, fcs=size + delta)
            out.append(Case("E_wrong_fcs%d_%+d" % (fw, delta), _payload(fw == 1), header=h))
    out.append(Case("E_fcs8_high_bytes", _payload(False), header=zp.header(single=True, fcs_width=8, fcs=310 + (1 << 32))))
    for dw in (1, 2, 4):
        out.append(Case("E_dict_id%d" % dw, _payload(False), header=zp.header(did=bytes(dw - 1) + b"\x01")))
    out.append(Case("E_reserved_bit", _payload(False), header=zp.header(reserved=True)))
    out.append(Case("E_checksum_flag", _payload(False), header=zp.header(checksum=True)))
    out.append(Case("E_window_at_bound", _payload(False), header=zp.header(window=(21 << 3) | 7)))
    out.append(Case("E_window_above_bound", _payload(False), header=zp.header(window=22 << 3)))
    out.append(Case("E_window_largest_byte", _payload(False), header=zp.header(window=0xFF)))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    out = group_a() + group_b() + group_c() + group_d() + group_e()
    assert len({c.name for c in out}) == len(out)
    return out
