"""A reader for the magicless zstd frames this project emits, written from RFC 8878 alone (test
infrastructure: it imports neither the oracle nor the product, so it is a third reading of the
format next to libzstd's and the oracle's).  It does not regenerate the data; it walks every
header, table description and the whole sequences bitstream, consumes the frame exactly (ValueError
otherwise) and reports which of the format's modes each block uses, so that a corpus can be shown
to reach every branch of the encoder (tests/test_zstd.py, the census).

Frame: descriptor byte 0x00 (no content size, no checksum, no dictionary), a window descriptor,
then blocks.  classify(frame) -> [block record]; frame_classes(records) -> the set of class names
a frame reaches; FORMAT_CLASSES lists every name.
"""

LL_BITS = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14,
           15, 16)
ML_BITS = (0,) * 32 + (1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)
LL_BASE = tuple(range(16)) + (16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384,
                              32768, 65536)
ML_BASE = tuple(range(3, 35)) + (35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                 16387, 32771, 65539)
LL_DEFAULT = (4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1,
              -1, -1)
ML_DEFAULT = (1, 4, 3, 2, 2, 2, 2, 2, 2) + (1,) * 37 + (-1,) * 7
OF_DEFAULT = (1, 1, 1, 1, 1, 1, 2, 2, 2) + (1,) * 15 + (-1,) * 5
BLOCK_MAX = 128 * 1024
# Offset codes above this need more bits than a 32-bit decoder's accumulator holds in one refill
# (RFC 8878 3.1.1.3.2.1.1 "offset codes ... above 25"; libzstd's STREAM_ACCUMULATOR_MIN_32).
LONG_OFFSET_CODE = 25
LIT_THRESHOLDS = (255, 256, 1023, 1024, 16383, 16384)  # 1 stream below 256; header width at 1,024 and 16,384

BLOCK_TYPES = ("raw", "rle", "compressed")
LIT_TYPES = ("raw", "rle", "huffman", "huffman_repeat")
MODES = ("predefined", "rle", "fse", "repeat")


def _need(cond, what):
    if not cond:
        raise ValueError("zstd frame: " + what)


def _read_ncount(buf, pos, end, max_symbol, max_log):
    """An FSE table description (RFC 8878 4.1.1) at buf[pos:end] -> (accuracy log, counts, next pos)."""
    acc = int.from_bytes(buf[pos:min(end, pos + 600)], "little")
    avail = 8 * (min(end, pos + 600) - pos)
    log = (acc & 15) + 5
    _need(log <= max_log, "FSE accuracy log %d over %d" % (log, max_log))
    at = 4
    remaining = 1 << log
    counts = []
    while remaining > 0 and len(counts) <= max_symbol:
        bits = (remaining + 1).bit_length()
        val = (acc >> at) & ((1 << bits) - 1)
        low = (1 << (bits - 1)) - 1
        threshold = (1 << bits) - 1 - (remaining + 1)
        if (val & low) < threshold:
            val &= low
            at += bits - 1
        else:
            if val > low:
                val -= threshold
            at += bits
        p = val - 1
        remaining -= -p if p < 0 else p
        counts.append(p)
        if p == 0:
            while True:
                rep = (acc >> at) & 3
                at += 2
                counts.extend([0] * rep)
                if rep != 3:
                    break
    _need(remaining == 0, "FSE counts do not sum to the table size")
    _need(len(counts) <= max_symbol + 1, "FSE table describes too many symbols")
    _need(at <= avail, "FSE table description runs past its section")
    return log, counts, pos + (at + 7) // 8


def _fse_table(log, counts):
    """Decoding table (RFC 8878 4.1.1): per state (symbol, bits to read, base of the next state)."""
    size = 1 << log
    sym = [0] * size
    high = size
    for s, c in enumerate(counts):
        if c == -1:
            high -= 1
            sym[high] = s
    step = (size >> 1) + (size >> 3) + 3
    pos = 0
    for s, c in enumerate(counts):
        for _ in range(c if c > 0 else 0):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos >= high:
                pos = (pos + step) & (size - 1)
    _need(pos == 0, "FSE table spread does not close")
    nxt = [1 if c == -1 else c for c in counts]
    nb, base = [0] * size, [0] * size
    for i in range(size):
        s = sym[i]
        n = nxt[s]
        nxt[s] = n + 1
        b = log - (n.bit_length() - 1)
        nb[i] = b
        base[i] = (n << b) - size
    return log, sym, nb, base


def _rle_table(symbol):
    return 0, [symbol], [0], [0]


class _Back:
    """A bitstream read from its last byte down (RFC 8878 4.1: the final byte's highest set bit
    is the end mark)."""

    def __init__(self, buf, start, end):
        _need(end > start, "empty bitstream")
        _need(buf[end - 1] != 0, "bitstream without an end mark")
        self.v = buf[start:end]
        self.pos = 8 * (end - start) - (9 - buf[end - 1].bit_length())

    def read(self, n):
        if n == 0:
            return 0
        self.pos -= n
        p = self.pos
        _need(p >= 0, "bitstream underflow")
        return (int.from_bytes(self.v[p >> 3:(p + n + 7) >> 3], "little") >> (p & 7)) & ((1 << n) - 1)


def _huffman_weights(buf, pos, end):
    """The Huffman tree description (RFC 8878 4.2.1) -> (coding, weights, next pos)."""
    _need(pos < end, "missing Huffman tree description")
    h = buf[pos]
    pos += 1
    if h >= 128:
        n = h - 127
        nbytes = (n + 1) // 2
        _need(pos + nbytes <= end, "direct Huffman weights run past the literals section")
        w = []
        for b in buf[pos:pos + nbytes]:
            w += [b >> 4, b & 15]
        w = w[:n]
        coding, pos = "direct", pos + nbytes
    else:
        _need(h > 0 and pos + h <= end, "FSE Huffman weights run past the literals section")
        log, counts, p = _read_ncount(buf, pos, pos + h, 12, 6)
        _, sym, nb, base = _fse_table(log, counts)
        bits = _Back(buf, p, pos + h)
        s1 = bits.read(log)
        s2 = bits.read(log)
        w = []
        while True:  # two interleaved states; the stream ends when a state update runs out of bits
            w.append(sym[s1])
            if bits.pos < nb[s1]:
                w.append(sym[s2])
                break
            s1 = base[s1] + bits.read(nb[s1])
            w.append(sym[s2])
            if bits.pos < nb[s2]:
                w.append(sym[s1])
                break
            s2 = base[s2] + bits.read(nb[s2])
            _need(len(w) <= 255, "too many Huffman weights")
        coding, pos = "fse", pos + h
    _need(all(x <= 12 for x in w), "Huffman weight over 12")
    total = sum(1 << (x - 1) for x in w if x)
    _need(total > 0, "empty Huffman tree")
    top = 1 << total.bit_length()  # the last weight completes the next power of two
    rest = top - total
    _need(rest & (rest - 1) == 0, "Huffman weights do not complete a power of two")
    _need(top.bit_length() - 1 <= 11, "Huffman tree deeper than 11 bits")
    return coding, w + [rest.bit_length()], pos


def _literals(buf, pos, end, have_tree):
    """The literals section (RFC 8878 3.1.1.3.1) -> (record fields, next pos)."""
    _need(pos < end, "missing literals section")
    b0 = buf[pos]
    kind, sf = b0 & 3, (b0 >> 2) & 3
    r = {"lit_type": LIT_TYPES[kind], "huf_weights": None, "huf_symbols": 0}
    if kind < 2:
        width = 1 if sf in (0, 2) else (2 if sf == 1 else 3)
        _need(pos + width <= end, "literals header runs past the block")
        v = int.from_bytes(buf[pos:pos + width], "little")
        regen = v >> (3 if width == 1 else 4)
        comp = regen if kind == 0 else 1
        streams = 0
    else:
        width = 3 if sf < 2 else sf + 2
        nbits = 10 if sf < 2 else (14 if sf == 2 else 18)
        _need(pos + width <= end, "literals header runs past the block")
        v = int.from_bytes(buf[pos:pos + width], "little") >> 4
        regen, comp = v & ((1 << nbits) - 1), v >> nbits
        streams = 1 if sf == 0 else 4
    pos += width
    _need(regen <= BLOCK_MAX, "more literals than a block holds")
    _need(pos + comp <= end, "literals run past the block")
    lit_end = pos + comp
    if kind >= 2:
        _need(regen > 0, "compressed literals of size 0")
        if kind == 2:
            coding, weights, pos = _huffman_weights(buf, pos, lit_end)
            r["huf_weights"] = coding
            r["huf_symbols"] = len(weights)
        else:
            _need(have_tree, "treeless literals with no earlier Huffman tree")
        if streams == 4:
            _need(pos + 6 <= lit_end, "missing jump table")
            sizes = [int.from_bytes(buf[pos + 2 * i:pos + 2 * i + 2], "little") for i in range(3)]
            pos += 6
            sizes.append(lit_end - pos - sum(sizes))
            _need(sizes[3] > 0, "jump table over the literals size")
        else:
            sizes = [lit_end - pos]
        for s in sizes:
            _need(s > 0 and buf[pos + s - 1] != 0, "Huffman stream without an end mark")
            pos += s
    r.update(lit_header=width, lit_streams=streams, lit_regen=regen, lit_comp=comp)
    return r, lit_end


def _sequences(buf, pos, end, tables, lit_regen):
    """The sequences section (RFC 8878 3.1.1.3.2), decoded to the end of its bitstream."""
    _need(pos < end, "missing sequences section")
    b0 = buf[pos]
    if b0 < 128:
        nseq, width = b0, 1
    elif b0 < 255:
        _need(pos + 2 <= end, "sequence count runs past the block")
        nseq, width = ((b0 - 128) << 8) + buf[pos + 1], 2
    else:
        _need(pos + 3 <= end, "sequence count runs past the block")
        nseq, width = buf[pos + 1] + (buf[pos + 2] << 8) + 0x7F00, 3
    pos += width
    r = {"nseq": nseq, "nseq_header": width, "ll_mode": None, "of_mode": None, "ml_mode": None, "max_ll_code": -1,
         "max_ml_code": -1, "max_of_code": -1, "long_offset": False, "rep_codes": frozenset(), "match_bytes": 0}
    if nseq == 0:
        _need(pos == end, "bytes after an empty sequences section")
        _need(width == 1, "zero sequences in a wide count")
        return r
    _need(pos < end, "missing compression modes")
    modes = buf[pos]
    pos += 1
    _need(modes & 3 == 0, "reserved compression-mode bits set")
    for i, (name, default, dlog, max_sym, max_log) in enumerate((("ll", LL_DEFAULT, 6, 35, 9), ("of", OF_DEFAULT, 5, 31, 8),
                                                                ("ml", ML_DEFAULT, 6, 52, 9))):
        m = (modes >> (6 - 2 * i)) & 3
        r[name + "_mode"] = MODES[m]
        if m == 0:
            tables[name] = _fse_table(dlog, default)
        elif m == 1:
            _need(pos < end, "missing RLE table symbol")
            _need(buf[pos] <= max_sym, "RLE table symbol out of range")
            tables[name] = _rle_table(buf[pos])
            pos += 1
        elif m == 2:
            log, counts, pos = _read_ncount(buf, pos, end, max_sym, max_log)
            tables[name] = _fse_table(log, counts)
        else:
            _need(tables.get(name) is not None, "repeat mode with no earlier table")
    bits = _Back(buf, pos, end)
    (gl, syl, nbl, bal), (go, syo, nbo, bao), (gm, sym, nbm, bam) = tables["ll"], tables["of"], tables["ml"]
    sl, so, sm = bits.read(gl), bits.read(go), bits.read(gm)
    v, p = bits.v, bits.pos
    max_ll = max_ml = max_of = -1
    reps = set()
    lits = match = 0
    for i in range(nseq):
        cl, co, cm = syl[sl], syo[so], sym[sm]
        xl, xm = LL_BITS[cl], ML_BITS[cm]
        last = i == nseq - 1
        ul, um, uo = (0, 0, 0) if last else (nbl[sl], nbm[sm], nbo[so])
        n = co + xm + xl + ul + um + uo
        p -= n
        _need(p >= 0, "sequences bitstream underflow")
        x = int.from_bytes(v[p >> 3:(p + n + 7) >> 3], "little") >> (p & 7)
        # fields from the top of x down: offset, match length, literal length, then the LL, ML, OF state updates
        n -= co
        ov = (1 << co) + ((x >> n) & ((1 << co) - 1))
        n -= xm
        ml = ML_BASE[cm] + ((x >> n) & ((1 << xm) - 1))
        n -= xl
        ll = LL_BASE[cl] + ((x >> n) & ((1 << xl) - 1))
        if not last:
            n -= ul
            sl = bal[sl] + ((x >> n) & ((1 << ul) - 1))
            n -= um
            sm = bam[sm] + ((x >> n) & ((1 << um) - 1))
            so = bao[so] + (x & ((1 << uo) - 1))
        if cl > max_ll:
            max_ll = cl
        if cm > max_ml:
            max_ml = cm
        if co > max_of:
            max_of = co
        if ov <= 3:
            reps.add((ov, ll == 0))
        lits += ll
        match += ml
    _need(p == 0, "sequences bitstream not consumed exactly (%d bits left)" % p)
    _need(lits <= lit_regen, "sequences use more literals than the block has")
    names = {(1, False): "rep1", (1, True): "rep2_at_ll0", (2, False): "rep2", (2, True): "rep3_at_ll0", (3, False): "rep3",
             (3, True): "rep1_minus_1"}
    r.update(max_ll_code=max_ll, max_ml_code=max_ml, max_of_code=max_of, long_offset=max_of > LONG_OFFSET_CODE,
             rep_codes=frozenset(names[k] for k in reps), match_bytes=match)
    return r


def _frame_header(buf):
    """Every form of the frame header (RFC 8878 3.1.1.1) -> (header fields, next pos).  Refused, as
    the decoder refuses them: the reserved bit, the checksum flag, a non-zero dictionary id and a
    window above 2^31."""
    _need(len(buf) >= 1, "shorter than its header")
    d = buf[0]
    _need(d & 8 == 0, "reserved bit of the frame header descriptor")
    _need(d & 4 == 0, "content checksum flag")
    single, pos = bool(d & 0x20), 1
    window_log = None
    if not single:
        _need(pos < len(buf), "missing window descriptor")
        window_log = 10 + (buf[pos] >> 3)
        _need(window_log <= 31, "window above 2^31")
        pos += 1
    did_width = (0, 1, 2, 4)[d & 3]
    _need(pos + did_width <= len(buf), "dictionary id runs past the frame")
    _need(not any(buf[pos:pos + did_width]), "non-zero dictionary id")
    pos += did_width
    fcs_width = (1 if single else 0, 2, 4, 8)[d >> 6]
    _need(pos + fcs_width <= len(buf), "content size runs past the frame")
    fcs = int.from_bytes(buf[pos:pos + fcs_width], "little") + (256 if fcs_width == 2 else 0) if fcs_width else None
    return {"single_segment": single, "window_log": window_log, "did_width": did_width, "fcs_width": fcs_width,
            "fcs": fcs}, pos + fcs_width


def classify(frame, any_header=False):
    """One record per block of a magicless frame; ValueError if the frame is not consumed exactly.
    any_header=False: only the header this project's encoder writes (descriptor 0x00).  True: every
    header form, its fields in each record's "header"; a content size must be the regenerated one."""
    buf = bytes(frame)
    if any_header:
        head, pos = _frame_header(buf)
        window_log = head["window_log"]
    else:
        _need(len(buf) >= 2, "shorter than its header")
        _need(buf[0] == 0, "frame header descriptor is not 0")
        _need(buf[1] & 7 == 0 and (buf[1] >> 3) <= 12, "window descriptor outside 1 KiB..4 MiB powers of two")
        window_log = 10 + (buf[1] >> 3)
        head, pos = None, 2
    out, tables, have_tree = [], {}, False
    while True:
        _need(pos + 3 <= len(buf), "missing block header")
        h = int.from_bytes(buf[pos:pos + 3], "little")
        pos += 3
        last, btype, size = h & 1, (h >> 1) & 3, h >> 3
        _need(btype < 3, "reserved block type")
        rec = {"type": BLOCK_TYPES[btype], "last": bool(last), "window_log": window_log, "lit_type": None,
               "lit_header": 0, "lit_streams": 0, "lit_regen": 0, "lit_comp": 0, "huf_weights": None, "huf_symbols": 0,
               "nseq": None, "nseq_header": 0, "ll_mode": None, "of_mode": None, "ml_mode": None, "max_ll_code": -1,
               "max_ml_code": -1, "max_of_code": -1, "long_offset": False, "rep_codes": frozenset()}
        if btype == 0:
            _need(pos + size <= len(buf), "raw block runs past the frame")
            rec["regen"], rec["body"] = size, size
            pos += size
        elif btype == 1:
            _need(pos + 1 <= len(buf), "RLE block runs past the frame")
            rec["regen"], rec["body"] = size, 1
            pos += 1
        else:
            end = pos + size
            _need(size > 0 and end <= len(buf), "compressed block runs past the frame")
            lit, p = _literals(buf, pos, end, have_tree)
            have_tree = have_tree or lit["lit_type"] == "huffman"
            rec.update(lit)
            seq = _sequences(buf, p, end, tables, lit["lit_regen"])
            rec["regen"] = lit["lit_regen"] + seq.pop("match_bytes")
            rec.update(seq)
            rec["body"] = size
            pos = end
        _need(rec["regen"] <= BLOCK_MAX, "block regenerates more than 128 KiB")
        if head is not None:
            rec["header"] = head
        out.append(rec)
        if last:
            break
    _need(pos == len(buf), "%d bytes after the last block" % (len(buf) - pos))
    if head is not None and head["fcs_width"]:
        _need(head["fcs"] == sum(r["regen"] for r in out), "content size differs from the regenerated size")
    return out


def _block_classes(b):
    c = {"block_" + b["type"]}
    if b["type"] != "compressed":
        return c
    c.add("lit_" + b["lit_type"])
    if b["lit_type"] in ("huffman", "huffman_repeat"):
        c.add("lit_header%d_%dstream" % (b["lit_header"], b["lit_streams"]) if b["lit_header"] == 3
              else "lit_header%d" % b["lit_header"])
        if b["lit_regen"] in LIT_THRESHOLDS:
            c.add("literal_count_at_%d" % b["lit_regen"])
        if b["lit_type"] == "huffman_repeat" and b["lit_streams"] == 1:
            c.add("huffman_repeat_1stream")
    if b["huf_weights"]:
        c.add("huf_weights_" + b["huf_weights"])
    n = b["nseq"]
    c.add("nseq_0" if n == 0 else "nseq_lt128" if n < 128 else "nseq_lt7f00" if n < 0x7F00 else "nseq_ge7f00")
    if n:
        for t in ("ll", "of", "ml"):
            c.add("%s_%s" % (t, b[t + "_mode"]))
        c.update(b["rep_codes"])
        if b["long_offset"]:
            c.add("long_offset")
        if b["max_of_code"] >= 20:
            c.add("of_code_ge20")
        if b["max_ll_code"] == 35:
            c.add("ll_code_35")
        if b["max_ml_code"] == 52:
            c.add("ml_code_52")
    return c


def frame_classes(blocks):
    """The class names one frame reaches: its blocks' classes and the classes of block sequences."""
    c = set()
    for b in blocks:
        c |= _block_classes(b)
    tree = False       # a Huffman tree has been written
    gap = False        # ... and a raw or RLE block came after it
    for i, b in enumerate(blocks):
        if b["type"] != "compressed":
            gap = tree
            if not b["last"] and any(x["type"] == "compressed" for x in blocks[i + 1:i + 2]):
                c.add("uncompressed_then_compressed")
                c.add(b["type"] + "_then_compressed")
            continue
        if b["lit_type"] == "huffman_repeat" and gap:
            c.add("huffman_table_reused_after_raw_block")
        if b["lit_type"] == "huffman":
            tree, gap = True, False
    return c


FORMAT_CLASSES = (
    "block_compressed", "block_raw", "block_rle",
    "huf_weights_fse", "huf_weights_direct",
    "lit_raw", "lit_rle", "lit_huffman", "lit_huffman_repeat", "huffman_repeat_1stream",
    "lit_header3_1stream", "lit_header3_4stream", "lit_header4", "lit_header5",
    "ll_predefined", "ll_rle", "ll_fse", "ll_repeat",
    "of_predefined", "of_rle", "of_fse", "of_repeat",
    "ml_predefined", "ml_rle", "ml_fse", "ml_repeat",
    "nseq_0", "nseq_lt128", "nseq_lt7f00", "nseq_ge7f00",
    "uncompressed_then_compressed", "raw_then_compressed", "rle_then_compressed",
    "huffman_table_reused_after_raw_block",
) + tuple("literal_count_at_%d" % n for n in LIT_THRESHOLDS) + (
    "long_offset", "of_code_ge20", "ll_code_35", "ml_code_52",
    "rep1", "rep2_at_ll0", "rep2", "rep3_at_ll0", "rep3", "rep1_minus_1",
)


# What a decoder must read beyond what this project's encoder writes: the header forms, the width
# of the sequence count and of a raw / RLE literals header.  (The repeat-offset index of every
# sequence -- codes 1, 2, 3, each with ll == 0 and ll > 0 -- and direct / FSE-coded Huffman weights
# are the rep* and huf_weights_* names above.)
HEADER_CLASSES = ("single_segment", "window_descriptor", "fcs_0", "fcs_1", "fcs_2", "fcs_4", "fcs_8",
                  "dict_id_0", "dict_id_1", "dict_id_2", "dict_id_4")
DECODER_CLASSES = FORMAT_CLASSES + HEADER_CLASSES + (
    "nseq_header1", "nseq_header2", "nseq_header3",
    "lit_raw_header1", "lit_raw_header2", "lit_raw_header3", "lit_rle_header1", "lit_rle_header2", "lit_rle_header3",
)


def decoder_classes(blocks):
    """frame_classes plus the DECODER_CLASSES names, over the records of classify(frame, any_header=True)."""
    c = frame_classes(blocks)
    h = blocks[0]["header"]
    c.add("single_segment" if h["single_segment"] else "window_descriptor")
    c.add("fcs_%d" % h["fcs_width"])
    c.add("dict_id_%d" % h["did_width"])
    for b in blocks:
        if b["type"] == "compressed":
            c.add("nseq_header%d" % b["nseq_header"])
            if b["lit_type"] in ("raw", "rle"):
                c.add("lit_%s_header%d" % (b["lit_type"], b["lit_header"]))
    return c


def census(frames):
    """{class: number of frames that reach it} over an iterable of frames, every class present."""
    count = dict.fromkeys(FORMAT_CLASSES, 0)
    for f in frames:
        for k in frame_classes(classify(f)):
            count[k] += 1
    return count
