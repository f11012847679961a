"""Planted cut candidates for the gear scan (pure numpy; the gear table and the masks come from the
oracle, so nothing here restates the library).

FastCDC's per-byte form is h_p = (h_{p-1} << 1) + GEAR[src[p]]; position p is a candidate iff
(h_p & mask) == 0, and a candidate that wins makes p the START of the next chunk (the crate's
cut() returns p as the chunk's length).  Every mask bit is <= 47, so the test at p depends on the
48 bytes src[p-47 ..= p] alone: writing a known 48-byte window so that its last byte is at p makes p
a candidate whatever surrounds it.  tests/golden/cdc_windows.json holds such windows for the masks
of avg = 1 MiB (backuwup's), found by tests/golden/make_cdc_windows.py.

The builders below return Case objects: an input, the parameters, the absolute positions that must
and must not start a chunk, and what the scan must see per tile.  tests/test_cdc_plant.py holds
every condition against the CPU oracle; tests/test_gpu_cdc_planted.py runs the same cases on the
GPU and then asserts, from bw_batch_counters, that the path the case was built for produced them.
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "cdc_windows.json")

P1 = (64, 1 << 20, 1 << 20)        # min 64: a cut may follow the previous one by 111 bytes
P3 = (64, 1 << 20, 3 << 20)        # the same masks, mask_l region from 1 MiB to 3 MiB
BK = (262144, 1 << 20, 3 << 20)    # backuwup: defaults.rs:61-68
WINDOW = 48                        # bytes that decide a mask test (top mask bit 47)
SCAN_CAP = 16                      # candidate / flagged-block slots per scan tile (bw_internal.h)
TILES = (131072, 65536)            # the two scan tiles (BW_OPT_SCAN_SMALL_BYTES = 0 / 2^64 - 1)
CHAIN_CAP = 128                    # cuts a segment's chain holds before the file is walked serially

S, L_ONLY, PRE_ONLY, NONE = "S", "L", "PRE", "-"


class Gear:
    """The gear table and one parameter set's masks, with the three tests the scan makes."""

    def __init__(self, table, mask_s, mask_l):
        self.g = np.asarray(table, dtype=np.uint64)
        self.mask_s, self.mask_l = int(mask_s), int(mask_l)
        top = (self.mask_s | self.mask_l).bit_length() - 1
        assert top < WINDOW
        # the scan's prefilter: the bits of mask_s & mask_l that fall into the high dword of
        # h << pre_shift, pre_shift = 63 - top (k_scan's pre_hi), as a mask on h itself
        pre_shift = 63 - top
        self.mask_pre = (((self.mask_s & self.mask_l) << pre_shift) >> 32 << 32 >> pre_shift) & ((1 << 64) - 1)

    @classmethod
    def of(cls, oracle, params):
        return cls(oracle.gear_table(), *oracle.masks(*params))

    def hash_all(self, buf, block=1 << 18):
        """The gear hash at every byte of buf, started from 0 at buf[0], low 48 bits exact (bits
        above 47 are dropped: no mask reads them).  From byte 47 on this is the windowed hash."""
        buf = np.asarray(buf, dtype=np.uint8)
        out = np.empty(buf.size, dtype=np.uint64)
        for lo in range(0, buf.size, block):  # cache-sized blocks, each with 47 bytes of history
            a = max(lo - (WINDOW - 1), 0)
            gb = self.g[buf[a:lo + block]]
            h = gb.copy()
            for i in range(1, WINDOW):
                h[i:] += gb[:-i] << np.uint64(i)
            out[lo:lo + block] = h[lo - a:]
        return out & np.uint64((1 << WINDOW) - 1)

    def hash_prefix(self, prefix):
        """The chunk-local (truncated) hash after the bytes of `prefix`, started from 0: what the
        crate holds len(prefix) bytes after a chunk's start + 2 * (min / 2).  All 64 bits."""
        h = 0
        for b in bytes(prefix):
            h = ((h << 1) + int(self.g[b])) & ((1 << 64) - 1)
        return h

    def classify_hash(self, h):
        h = int(h)
        if h & self.mask_s == 0:
            return S
        if h & self.mask_l == 0:
            return L_ONLY
        if h & self.mask_pre == 0:
            return PRE_ONLY
        return NONE

    def classify(self, window):
        """S (passes mask_s; mask_l is a subset here, so it passes that too), L (mask_l only), PRE
        (only the scan's prefilter: flags its 64-byte block, yields no candidate) or '-'."""
        w = bytes(window)
        assert len(w) >= WINDOW
        return self.classify_hash(self.hash_prefix(w[-64:]))

    def census(self, buf, tile, h=None):
        """Per tile of `tile` bytes: (candidates, flagged 64-byte blocks) as k_scan counts them
        (h = hash_all(buf), when the caller has it)."""
        h = self.hash_all(buf) if h is None else h
        cand = (h & np.uint64(self.mask_l)) == 0
        flag = (h & np.uint64(self.mask_pre)) == 0
        nt = (len(h) + tile - 1) // tile
        pos = np.nonzero(cand)[0]
        blocks = np.unique(np.nonzero(flag)[0] // 64)
        return (np.bincount(pos // tile, minlength=nt), np.bincount(blocks * 64 // tile, minlength=nt))


def plant(buf, pos, window):
    """Write `window` so that its last byte is buf[pos]."""
    w = np.frombuffer(bytes(window), dtype=np.uint8)
    assert pos - len(w) + 1 >= 0 and pos < len(buf), (pos, len(w), len(buf))
    buf[pos - len(w) + 1:pos + 1] = w


def load_windows():
    with open(FIXTURE) as f:
        j = json.load(f)
    out = {k: [bytes.fromhex(x) for x in j[k]] for k in (S, L_ONLY, PRE_ONLY)}
    out["TRUNC"] = {int(k): (None if v is None else bytes.fromhex(v)) for k, v in j["truncated_prefix_mask_s"].items()}
    out["params"] = tuple(j["params"])
    return out


def filler(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def scrub(gear, buf, keep, candidates_only=False):
    """Remove every stray hit of buf that is not a planted position in `keep` (position -> planted
    length) by changing one filler byte inside the hit's window; planted bytes are left alone.
    A hit is a prefilter pass (which includes every candidate), or with candidates_only a mask_l
    pass.  Afterwards the candidates (and flagged blocks) of buf are exactly the planted ones.
    Hits in the first 47 bytes of the buffer (a hash with less than a window of history) stay."""
    mask = np.uint64(gear.mask_l if candidates_only else gear.mask_pre)
    prot = np.zeros(len(buf), dtype=bool)
    for p, n in keep.items():
        prot[p - n + 1:p + 1] = True
    h = gear.hash_all(buf)
    todo = [int(p) for p in np.nonzero((h & mask) == 0)[0] if int(p) not in keep and p >= WINDOW - 1]
    for _ in range(100000):
        if not todo:
            return
        p = todo.pop()
        q = p
        while prot[q]:
            q -= 1
        assert p - q < WINDOW, "a stray hit at %d lies wholly inside planted windows" % p
        buf[q] ^= 0x55
        # the change reaches the hashes of [q, q + 47]: test those again
        a, b = max(q - (WINDOW - 1), 0), min(q + WINDOW, len(buf))
        hh = gear.hash_all(buf[a:b])
        todo = [t for t in todo if not q <= t < q + WINDOW]
        todo += [a + int(i) for i in np.nonzero((hh & mask) == 0)[0]
                 if q <= a + int(i) and a + int(i) not in keep and a + int(i) >= WINDOW - 1]
    raise AssertionError("scrub did not converge")


class Case:
    """One input: cuts / no_cuts are absolute buffer positions that must / must not start a chunk;
    expect maps bw_batch_counters names to the values the GPU must report (callables take the
    counters); tiles = {tile index: (candidates, flagged blocks)} the census must give."""

    def __init__(self, name, data, offs, lens, params, cuts=(), no_cuts=(), expect=None, tiles=None, tile=None):
        self.name, self.data, self.params = name, data, params
        self.offs = np.asarray(offs, dtype=np.uint64)
        self.lens = np.asarray(lens, dtype=np.uint64)
        self.cuts, self.no_cuts = sorted(set(cuts)), sorted(set(no_cuts))
        self.expect = dict(expect or {})
        self.tiles, self.tile = tiles, tile

    def starts(self, blobs):
        """Absolute positions at which the chunks of a blob table start."""
        return set((self.offs[blobs["file"]] + blobs["offset"]).tolist())

    def check_cuts(self, blobs):
        st = self.starts(blobs)
        missing = [p for p in self.cuts if p not in st]
        extra = [p for p in self.no_cuts if p in st]
        assert not missing and not extra, (self.name, "planted cuts missing", missing[:8], "cut where none may be",
                                           extra[:8])


FAST = {"ovf_tiles": 0, "trunc": (1 << 64) - 1, "serial_files": 0}


# ------------------------------------------------------------------ A: strip-offset sweep

def sweep(win, stride=16385, count=2052, seed=2):
    """S windows at an odd stride = 1 (mod 2048) in random filler, one file, P1: the planted cuts
    visit every offset of a 2 KiB (and 1 KiB) strip, hence every lane of a 64-byte block, every
    staging row and both parities.  64 planted cuts per 1 MiB segment stay under CHAIN_CAP."""
    assert stride % 2048 == 1
    n = stride * (count + 1)
    buf = filler(seed, n)
    pos = [stride * (i + 1) for i in range(count)]
    for i, p in enumerate(pos):
        plant(buf, p, win[S][i % len(win[S])])
    assert len({p % 2048 for p in pos}) == 2048
    return Case("sweep", buf, [0], [n], P1, cuts=pos, expect=FAST)


# ------------------------------------------------------------------ B: tile and buffer edges

def edge_offsets(tile):
    strip = tile // 64
    return [0, 1, 63, 64, 65, strip - 1, strip, strip + 1, tile - 64, tile - 1]


EDGE_PHASES = 7  # groups of edge_offsets whose files do not reach into each other's windows


def edge_phase(tile, phase):
    strip = tile // 64
    return [[0, strip - 1], [1, strip], [63, strip + 1], [64], [65], [tile - 64], [tile - 1]][phase]


def edges(win, tile, phase, k=5, delta=0, seed=5):
    """One S window per file at T * tile + o, o in edge_phase(tile, phase), for T = first, a middle
    and the last full tile, and the same offsets inside the ragged tail tile (k_scan's exact byte
    path); the buffer is k * tile + delta bytes (delta 0: no ragged tile; a position with less than
    two bytes after it falls away, as it could not cut).  Each file starts 200 bytes before its
    planted position -- past s0 + 47 = 111, so the candidate array answers, and files straddle the
    tile edges -- and ends 300 bytes after it; tile 0's offsets below 200 have no room for that
    and fall away.  The seven phases together cover edge_offsets(tile): neighbouring offsets
    (63, 64, 65; tile - 1 and the next tile's 0) go to different phases, or their windows and files
    would overlap."""
    n = k * tile + delta
    buf = filler(seed + phase, n)
    last_full = n // tile - 1
    assert last_full >= 3
    pos = [t * tile + o for t in sorted({0, last_full // 2, last_full, n // tile}) for o in edge_phase(tile, phase)]
    pos = sorted(p for p in set(pos) if 200 <= p and p + 2 <= n)
    for i, p in enumerate(pos):
        plant(buf, p, win[S][(i + phase) % len(win[S])])
    offs = [p - 200 for p in pos]
    lens = [min(500, n - o) for o in offs]
    return Case("edges", buf, offs, lens, P1, cuts=pos, expect=FAST, tile=tile)


# ------------------------------------------------------------------ C: slot capacity

def capacity(gear, win, tile, n_cand, n_pre=0, pair=False, seed=7):
    """Three tiles and a ragged one; tile 1 holds n_cand planted candidates (S windows, 1 KiB apart
    from the tile's byte 4096 on) and n_pre prefilter-only windows in 64-byte blocks of their own;
    tiles 0 and 2 hold one candidate each.  pair: two more candidates in ONE 64-byte block of tile
    1, 48 bytes apart (block offsets 8 and 56).  One file, P1; strays are scrubbed, so the census
    of every tile is exactly what was planted."""
    n = 3 * tile + 1000
    buf = filler(seed, n)
    base = tile
    pos = [tile // 2, 2 * tile + tile // 2]
    pos += [base + 4096 + 1024 * i + (i % 7) for i in range(n_cand)]
    if pair:
        pos += [base + 2048 + 8, base + 2048 + 56]
    pre = [base + 30000 + 128 * i + (i % 5) for i in range(n_pre)]
    assert not pre or max(pre) < 2 * tile
    keep = {}
    for i, p in enumerate(sorted(pos)):
        plant(buf, p, win[S][i % len(win[S])])
        keep[p] = WINDOW
    for i, p in enumerate(pre):
        plant(buf, p, win[PRE_ONLY][i % len(win[PRE_ONLY])])
        keep[p] = WINDOW
    scrub(gear, buf, keep)
    in1 = n_cand + (2 if pair else 0)
    blocks1 = len({p // 64 for p in pos + pre if tile <= p < 2 * tile})
    over = in1 > SCAN_CAP or blocks1 > SCAN_CAP
    exp = dict(FAST, ovf_tiles=1 if over else 0, cand_found=in1 + 2)
    shadowed = [base + 2048 + 56] if pair else []  # 48 bytes after a cut: inside the next chunk's min
    return Case("capacity", buf, [0], [n], P1, cuts=[p for p in pos if p not in shadowed], no_cuts=pre + shadowed,
                expect=exp,
                tiles={0: (1, 1), 1: (in1, blocks1), 2: (1, 1), 3: (0, 0)}, tile=tile)


# ------------------------------------------------------------------ D: mask switch at center

def mask_switch(gear, win, seed=11):
    """P3, one planted window per file, every stray candidate scrubbed: a file's first chunk runs
    to its planted position or, where that must not cut, to the file's end.  center = avg = 1 MiB
    for files of at least 1 MiB, r2 = remaining & ~1."""
    c = P3[1]
    plan = [  # (file length, position in the file, window kind, cuts?)
        ((1 << 20) + 5000, c - 1, L_ONLY, False),   # mask_s region: an L-only window is no candidate
        ((1 << 20) + 5000, c, L_ONLY, True),        # first position of the mask_l region
        ((1 << 20) + 5000, c - 1, S, True),
        ((1 << 20) + 5001, c + 1, L_ONLY, True),    # the other parity of the mask_l region
        ((1 << 20) + 4001, (1 << 20) + 3999, L_ONLY, True),   # odd length: r2 - 1, the last tested position
        ((1 << 20) + 4001, (1 << 20) + 4000, L_ONLY, False),  # r2 itself (the file's last byte): never tested
        ((1 << 20) + 4001, (1 << 20) + 4000, S, False),
        ((1 << 20) + 4000, (1 << 20) + 3999, L_ONLY, True),   # even length: r2 - 1 is the last byte
        ((1 << 20) - 4000, (1 << 20) - 8000, L_ONLY, False),  # shorter than avg: center = rem, mask_s throughout
        ((1 << 20) - 4000, (1 << 20) - 8000, S, True),
        ((1 << 20) - 4001, (1 << 20) - 4003, S, True),        # short and odd: r2 - 1
        ((1 << 20) - 4001, (1 << 20) - 4002, S, False),       # short and odd: r2
    ]
    offs, lens, cuts, no_cuts = [], [], [], []
    total = sum(ln for ln, _, _, _ in plan)
    buf = filler(seed, total)
    o = 0
    keep = {}
    for i, (ln, p, kind, cut) in enumerate(plan):
        plant(buf, o + p, win[kind][i % len(win[kind])])
        keep[o + p] = WINDOW
        (cuts if cut else no_cuts).append(o + p)
        offs.append(o)
        lens.append(ln)
        o += ln
    scrub(gear, buf, keep, candidates_only=True)
    return Case("mask_switch", buf, offs, lens, P3, cuts=cuts, no_cuts=no_cuts, expect=FAST)


# ------------------------------------------------------------------ E: head region

HEAD_K = (0, 1, 45, 46)


def head(gear, win, seed=13):
    """P1, files of 4 KiB: s0 = 64, so the positions s + 64 + k, k < 47, are judged by the hash
    truncated at s + 64 (walk_next's head), k = 47 is the first the candidate array answers.
    A windowed-hash candidate at k < 47 whose truncated hash does not pass is no cut (at k = 46 the
    two differ in bit 47 alone, by the low bit of the gear value of the window's first byte: the
    window is chosen so that they do); the fixture's truncated prefixes are cuts; each file also
    carries an S window at 2000, its one ordinary cut."""
    s0 = 2 * (P1[0] // 2)

    def miss(k):  # an S window whose last k + 1 bytes, hashed from zero, do not pass mask_s
        return next(w for w in win[S] if gear.hash_prefix(w[-(k + 1):]) & gear.mask_s)
    plan = [(k, "window") for k in HEAD_K] + [(47, "window")]
    plan += [(k, "prefix") for k, v in sorted(win["TRUNC"].items()) if v is not None]
    flen = 4096
    buf = filler(seed, flen * len(plan))
    offs, lens, cuts, no_cuts = [], [], [], []
    for i, (k, what) in enumerate(plan):
        s = i * flen
        p = s + s0 + k
        if what == "window":
            plant(buf, p, win[S][i % len(win[S])] if k >= 47 else miss(k))
            (cuts if k >= 47 else no_cuts).append(p)
        else:
            pre = win["TRUNC"][k]
            assert len(pre) == k + 1
            plant(buf, p, pre)
            cuts.append(p)
        plant(buf, s + 2000, win[S][(i + 3) % len(win[S])])
        cuts.append(s + 2000)
        offs.append(s)
        lens.append(flen)
    return Case("head", buf, offs, lens, P1, cuts=cuts, no_cuts=no_cuts, expect=FAST)


# ------------------------------------------------------------------ F: segments

def segments(gear, win, seg_bytes=1 << 20, empty=True, seed=17):
    """P1, one file of 5 segments + 777 bytes, a cut exactly on the start of segment 1, stray
    candidates scrubbed from the whole file.  empty: cuts inside segments 0, 2 and 4 only and no
    candidate at all in segment 3, which the true chain crosses with one forced cut, max = 1 MiB
    after the cut in segment 2.  Not empty: a cut inside every segment, none forced.
    seg_bytes is what bw_batch_counters reports for P1; the CPU test uses the default."""
    n = 5 * seg_bytes + 777
    buf = filler(seed, n)
    pos = [seg_bytes // 2, seg_bytes, 2 * seg_bytes + seg_bytes // 2 + 1, 4 * seg_bytes + 12345]
    if not empty:  # a cut in every segment, less than max apart: no forced cut anywhere
        pos = [seg_bytes // 2, seg_bytes, seg_bytes + seg_bytes // 2 + 1, 2 * seg_bytes + seg_bytes // 4,
               3 * seg_bytes + 4097, 4 * seg_bytes - 5000, 4 * seg_bytes + 12345]
        assert max(b - a for a, b in zip([0] + pos, pos + [n])) < P1[2]
    keep = {}
    for i, p in enumerate(pos):
        plant(buf, p, win[S][i % len(win[S])])
        keep[p] = WINDOW
    scrub(gear, buf, keep, candidates_only=True)
    forced = []
    if empty:
        forced = [pos[2] + P1[2]]
        assert 3 * seg_bytes <= forced[0] < 4 * seg_bytes
    return Case("segments", buf, [0], [n], P1, cuts=pos + forced, expect=dict(FAST, cand_found=len(pos)))


def backuwup_sweep(gear, win, seed=19):
    """True backuwup parameters (min 256 KiB), one 24 MiB file, 8 planted cuts about 2.6 MiB apart
    at assorted strip offsets: each lies in the mask_l region of the chunk the previous one
    starts, so S and L-only windows alternate.  Stray candidates are scrubbed (about five per gap
    otherwise), so the chunk list is exactly the planted cuts and the tail."""
    n = 24 << 20
    buf = filler(seed, n)
    pos = [(i + 1) * 2730000 + 2048 * i + (0, 1, 63, 64, 1023, 1024, 2047, 65)[i] for i in range(8)]
    keep = {}
    for i, p in enumerate(pos):
        plant(buf, p, win[S if i % 2 == 0 else L_ONLY][i % 8])
        keep[p] = WINDOW
    scrub(gear, buf, keep, candidates_only=True)
    return Case("backuwup_sweep", buf, [0], [n], BK, cuts=pos, expect=dict(FAST, cand_found=len(pos)))
