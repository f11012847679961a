"""Planted chains for the chunker's second stage: a plain model of the speculative chain walk and
its resolution, and inputs that hold neighbouring chains apart on purpose (pure Python + numpy).

The gear scan leaves a sorted candidate array; bw_cdc.hip then walks one speculative chain per
segment (k_chains), extends each until it meets its right neighbour's (k_extend), takes the running
maximum of the merge points per file (k_resolve) and either assembles the blobs from the chains or
hands the file to the serial walker (k_fallback).  On random data a chain resynchronises at the first
cut after its segment's start, so none of the decisions in between is exercised.

Two tools hold chains apart (tests/cdc_plant.py has the windows):

  the ladder   At P1 (min 64, avg = max = 1 MiB) a cut at x is followed by the first S window at
               x + 111 or later: a window less than 64 bytes after x is skipped, one 64..110 bytes
               after it is judged by a truncated hash and does not pass.  Windows 55..62 bytes
               apart are therefore taken alternately by two chains that start on opposite rungs,
               and the two meet at the first window that follows a gap of 111 bytes or more.
  forced cuts  Without candidates a chain cuts every max bytes from where it stands.  Segments are
               a multiple of max, so a true chain that last cut off a segment start stays out of
               phase with every speculative chain for as many candidate-free segments as follow.

Model.cut is the crate's cut() as the oracle has it, over the candidate list; Model.resolve is the
rule of k_chains / k_extend / k_resolve as their comments and DESIGN.md state it.  The model only
predicts the PATH (serial_files, segments, seg_bytes, and each segment's contribution): the chunks
of every case are compared with the CPU oracle, never with the model.  tests/test_cdc_chain_plant.py
checks the model's cut against the oracle and every structural fact the cases rest on;
tests/test_gpu_cdc_chains.py runs the cases on the GPU.
"""
import bisect

import numpy as np

import cdc_plant as cp
from cdc_plant import CHAIN_CAP, P1, P3, S, L_ONLY, WINDOW, plant

NONE = (1 << 64) - 1
M64 = (1 << 64) - 1
MIB = 1 << 20
PF = (64, 256, 1024)               # small parameters: 2 KiB segments in a small batch
SMALL_BATCH_BYTES = 1 << 32        # batches below this count as small (BW_OPT_SCAN_SMALL_BYTES' default)
RESOLVE_THREADS = 1024             # k_resolve's one block
UNIT_BLOCK = 256                   # units per block of k_unit_count


def seg_len_for(params, small_batch):
    """bw_capi.hip seg_len_for: a multiple of max that keeps a segment's own cuts within
    CHAIN_CAP / 2, at most 2 x max for a small batch and 8 x max otherwise."""
    mn, _, mx = params
    s0 = 2 * (mn // 2)
    k = (CHAIN_CAP // 2) * min(s0, mx) // mx
    k = max(k, 1)
    k = min(k, 2 if small_batch else 8)
    return k * mx


class Model:
    """cut() over a candidate list, and the resolution rule.  The keyword flags are the one-line
    mistakes the discrimination check applies; all False (and cap = CHAIN_CAP) is the rule."""

    def __init__(self, gear, data, params, no_beyond=False, first64=False, last_merge=False, end_gt=False,
                 cover_gt=False, cap=CHAIN_CAP, late_neighbour=False, like=None):
        self.gear, self.data, self.params = gear, np.asarray(data, dtype=np.uint8), params
        self.mn, self.avg, self.mx = params
        assert self.avg <= self.mx  # (avg > max is the crate's out-of-bounds corner; not modelled)
        self.s0 = 2 * (self.mn // 2)
        self.g = [int(x) for x in gear.g]
        if like is not None:  # the same input under another rule: its candidates and cuts are the same
            self.cand, self.cand_s, self.cand_l, self._memo = like.cand, like.cand_s, like.cand_l, like._memo
        else:
            h = gear.hash_all(self.data)
            is_l = (h & np.uint64(gear.mask_l)) == 0
            is_s = (h & np.uint64(gear.mask_s)) == 0
            pos = np.nonzero(is_l | is_s)[0]
            self.cand = [int(p) for p in pos]
            self.cand_s = [bool(x) for x in is_s[pos]]
            self.cand_l = [bool(x) for x in is_l[pos]]
            self._memo = {}
        self.no_beyond, self.first64, self.last_merge = no_beyond, first64, last_merge
        self.end_gt, self.cover_gt, self.cap, self.late_neighbour = end_gt, cover_gt, cap, late_neighbour

    # ---------------------------------------------------------------- the crate's cut()

    def cut(self, start, file_end):
        """The start of the chunk after the one starting at `start` in a file ending at file_end."""
        key = (start, file_end)
        if key not in self._memo:
            self._memo[key] = self._cut(start, file_end)
        return self._memo[key]

    def _cut(self, s, fe):
        rem = fe - s
        assert rem > 0
        if rem <= self.mn:
            return fe
        center, remaining = self.avg, rem
        if rem > self.mx:
            remaining = self.mx
        elif rem < center:
            center = rem
        c2, r2 = center & ~1, remaining & ~1
        # the 47 positions after s + s0 see a hash that starts from 0 at s + s0 (Gear.hash_prefix)
        h = 0
        for k in range(WINDOW - 1):
            p = self.s0 + k
            if p >= r2:
                break
            h = ((h << 1) + self.g[self.data[s + p]]) & M64
            if h & (self.gear.mask_s if p < c2 else self.gear.mask_l) == 0:
                return s + p
        # from there on the windowed hash decides: the candidate list
        lo, hi, c2a = s + self.s0 + WINDOW - 1, s + r2, s + c2
        i = bisect.bisect_left(self.cand, lo)
        while i < len(self.cand) and self.cand[i] < hi:
            p = self.cand[i]
            if self.cand_s[i] if p < c2a else self.cand_l[i]:
                return p
            i += 1
        return s + remaining

    def true_chain(self, start, file_end):
        out, s = [], start
        while s < file_end:
            out.append(s)
            s = self.cut(s, file_end)
        return out

    # ---------------------------------------------------------------- chains, extension, resolution

    def chain(self, start, end, file_end):
        """k_chains: (entries stored, cuts made).  The chain runs one cut beyond its first cut at or
        past the segment's end; at most cap entries are stored, and cap + 1 cuts mark it overlong."""
        ent, n, s, past = [], 0, start, False
        while True:
            c = self.cut(s, file_end)
            if n < self.cap:
                ent.append(c)
            n += 1
            beyond = c > end if self.end_gt else c >= end
            if n > self.cap or c >= file_end or (beyond and (past or self.no_beyond)):
                break
            past = beyond
            s = c
        return ent, n

    def extend(self, ent, n, nb_ent, nb_n, nb_start, file_end):
        """k_extend: continue the chain until a cut is one of the neighbour's stored entries or the
        neighbour's start; give up when the neighbour's coverage or the cap is used up."""
        if n > self.cap or nb_n == 0:
            return ent, n, NONE, None
        stored = nb_ent[:min(nb_n, self.cap)]
        seen = stored[:64] if self.first64 else stored
        last1 = stored[-1]
        ent, e = list(ent), ent[n - 1]
        while True:
            if e == nb_start:
                return ent, n, e, -1
            if e in seen:
                return ent, n, e, seen.index(e)
            if (e > last1 if self.cover_gt else e >= last1) or n >= self.cap:
                return ent, n, NONE, None
            e = self.cut(e, file_end)
            ent.append(e)
            n += 1

    def resolve(self, offs, lens, threshold=0, small_batch=True):
        """The whole second stage.  Returns a dict: seg_bytes, segments, cdc_files, serial (file
        indices that go to the serial walker), segs (per segment: file, start, end, stored chain
        length before and after extension, merge, index of the merge in the neighbour's stored
        entries, M, and `starts`, the chunk starts the segment contributes)."""
        L = seg_len_for(self.params, small_batch)
        segs, serial, ncf = [], [], 0
        for f, (o, ln) in enumerate(zip(offs, lens)):
            o, ln = int(o), int(ln)
            if not (ln > threshold and ln > 0):
                continue
            ncf += 1
            fe, ns = o + ln, -(-ln // L)
            mine = []
            for j in range(ns):
                st, en = o + j * L, min(o + (j + 1) * L, fe)
                ent, n = self.chain(st, en, fe)
                mine.append(dict(file=f, start=st, end=en, file_end=fe, last=j + 1 == ns, chain0=ent, n0=n))
            for j in reversed(range(ns)):  # right to left, so that late_neighbour can see extended chains
                sd = mine[j]
                if sd["last"]:
                    sd.update(chain=sd["chain0"], n=sd["n0"], merge=fe, merge_idx=None)
                    continue
                nb = mine[j + 1]
                nb_ent, nb_n = (nb["chain"], nb["n"]) if self.late_neighbour else (nb["chain0"], nb["n0"])
                ent, n, m, idx = self.extend(sd["chain0"], sd["n0"], nb_ent, nb_n, nb["start"], fe)
                sd.update(chain=ent, n=n, merge=m, merge_idx=idx)
            run, bad = 0, False
            for j, sd in enumerate(mine):
                sd["M"] = sd["start"] if j == 0 else run
                run = sd["merge"] if (self.last_merge or j == 0) else max(run, sd["merge"])
            for j, sd in enumerate(mine):
                M = sd["M"]
                R = fe if sd["last"] else mine[j + 1]["M"]
                ent = sd["chain"][:min(sd["n"], self.cap)]
                ok = sd["n"] <= self.cap and M != NONE and R != NONE
                starts = []
                if ok:
                    found = M == sd["start"] or M in ent
                    if M == sd["start"] and sd["start"] < R:
                        starts.append(sd["start"])
                    starts += [e for e in ent if M <= e < R and e != sd["start"]]
                    if not sd["last"] and R > M:
                        ok = R in ent
                    ok = ok and found
                sd["ok"], sd["starts"] = ok, starts
                bad = bad or not ok
            if bad:
                serial.append(f)
            segs += mine
        return dict(seg_bytes=L, segments=len(segs), cdc_files=ncf, serial=serial, segs=segs)


def signature(res):
    """What the discrimination check compares: the serial set and every segment's contribution."""
    return (tuple(res["serial"]), tuple(tuple(sd["starts"]) for sd in res["segs"]))


# ---------------------------------------------------------------------- cases

class ChainCase(cp.Case):
    """A Case plus: planted = the windowed candidates the input must have and no others; path =
    'chain' or 'serial' (what the case is built to give; the model must agree); facts = what the CPU
    test asserts about the model's view of it; threshold = small_file_threshold of the batch."""

    def __init__(self, name, data, offs, lens, params, planted, path, cuts=(), no_cuts=(), facts=None, threshold=0):
        super().__init__(name, data, offs, lens, params, cuts=cuts, no_cuts=no_cuts)
        self.planted, self.path, self.facts, self.threshold = sorted(planted), path, dict(facts or {}), threshold


class Builder:
    """A filler buffer, planted S windows (and other pieces), then a scrub of every stray candidate."""

    def __init__(self, win, n, seed):
        self.win, self.buf, self.keep, self.planted, self.i = win, cp.filler(seed, n), {}, [], 0

    def s(self, pos, kind=S):
        w = self.win[kind][self.i % len(self.win[kind])]
        self.i += 1
        for p, n in self.keep.items():
            assert pos - WINDOW >= p or p - n >= pos, ("planted pieces overlap", p, pos)
        plant(self.buf, pos, w)
        self.keep[pos] = WINDOW
        self.planted.append(pos)
        return pos

    def prefix(self, pos, k):
        """A truncated prefix of k + 1 bytes ending at pos: a cut for the chain whose head region
        starts at pos - k, a handful of protected bytes for every other."""
        pre = self.win["TRUNC"][k]
        assert pre is not None and len(pre) == k + 1
        plant(self.buf, pos, pre)
        self.keep[pos] = len(pre)
        return pos

    def done(self, gear):
        cp.scrub(gear, self.buf, self.keep, candidates_only=True)
        return self.buf


def ladder_a(gear, win, k, tail_cut=True, seed=101):
    """A: two segments at P1, b = 1 MiB.  The true chain cuts at t = b - 40; the chain from b cuts
    first at a 3-byte truncated prefix at b + 66 (for the true chain, 106 bytes after t, that is no
    cut), and from there the two take the rungs b + 120 + 60 i alternately -- the true chain the
    even ones -- until both cut at Z, 200 bytes after the last rung: chain 1 stores Z at index k,
    and chain 0 ends with k + 1 entries (t, k - 1 rungs, Z).  The file ends 50 bytes after Z, less
    than min, so chain 1 has k + 2 entries.  tail_cut False leaves Z out and ends the file 50 bytes
    after the last rung: the chains then first meet at the file's end, chain 1's entry k.
    k_extend compares from the chain's last stored entry on, and chain 0 stores t and its first two
    cuts past b, so for k < 2 the layout is: k = 1, one rung (the true chain's) between the prefix
    and Z; k = 0, no prefix, t = b - 100 and one window at b + 20, which the chain from b skips: it
    cuts first at Z."""
    b = MIB
    rungs = [b + 120 + 60 * i for i in range(max(2 * (k - 1), 1))] if k else [b + 20]
    last = rungs[-1]
    z = last + 200
    fe = (z if tail_cut else last) + 50
    B = Builder(win, fe, seed + k)
    t = B.s(b - 40 if k else b - 100)
    if k:
        B.prefix(b + 66, 2)
    for r in rungs:
        B.s(r)
    if tail_cut:
        B.s(z)
    meet = z if tail_cut else fe
    true_cuts = [t] + rungs[0::2] + ([z] if tail_cut else [])
    other = ([b + 66] if k else []) + rungs[1::2]
    facts = dict(meet=meet, index=k, chain_len=(max(k + 1, 3), k + 2 if tail_cut else k + 1))
    return ChainCase("ladder_a[%d%s]" % (k, "" if tail_cut else ",end"), B.done(gear), [0], [fe], P1, B.planted, "chain",
                     cuts=true_cuts, no_cuts=other, facts=facts)


A_CASES = [(0, True), (1, True), (63, True), (64, True), (126, True), (127, False)]


def cap_b(gear, win, m, steps, on_end=False, seed=131):
    """B: three segments at P1; the middle one's chain is the one under test.  It holds m cuts of
    its own, 200 bytes apart from b1 + 200 on (every chain takes all of them), then its first two
    cuts past b2: m + 2 stored entries.  steps = 0: both of those are cuts of chain 2 as well, the
    chains merge without an extension.  steps >= 1: the true chain (w) and chain 2 (y) take the
    windows after b2 alternately, w1 = b2 + 50, y1 = b2 + 112, w_i = w1 + 120 (i - 1),
    y_i = b2 + 110 + 120 (i - 1), through w_{steps + 1}, and meet at Z 200 bytes later: the stored
    chain ends at w2 and needs `steps` extension steps to reach Z.  on_end: the first cut past the
    segment is exactly b2 (and the second b2 + 150)."""
    b1, b2 = MIB, 2 * MIB
    q = [b1 + 200 * (i + 1) for i in range(m)]
    if steps == 0:
        w, y = ([b2, b2 + 150] if on_end else [b2 + 150, b2 + 300]), []
        z = w[-1] + 200
    else:
        assert not on_end
        w = [b2 + 50 + 120 * i for i in range(steps + 1)]
        y = [b2 + 112] + [b2 + 110 + 120 * i for i in range(1, steps)]
        z = w[-1] + 200
    fe = z + 5000
    B = Builder(win, fe, seed + m * 8 + steps)
    u = B.s(b1 - 5000)
    for p in sorted(q + w + y + [z]):
        B.s(p)
    n1 = m + 2
    over = m > CHAIN_CAP or n1 > CHAIN_CAP or (steps and n1 + steps > CHAIN_CAP)
    facts = dict(n0=min(n1, CHAIN_CAP + 1), steps=steps)
    return ChainCase("cap_b[m%d,s%d%s]" % (m, steps, ",end" if on_end else ""), B.done(gear), [0], [fe], P1, B.planted,
                     "serial" if over else "chain", cuts=[u] + q + w + [z], no_cuts=y, facts=facts)


# (m, steps, on_end) -> path, by the rule: a chain may hold CHAIN_CAP entries, extension included
B_CASES = [(CHAIN_CAP - 2, 0, False),   # exactly CHAIN_CAP entries, merges on a stored one: chain
           (CHAIN_CAP - 2, 1, False),   # the same needing one extension step: serial
           (CHAIN_CAP + 1, 0, False),   # CHAIN_CAP + 1 cuts inside the segment: serial
           (CHAIN_CAP - 3, 2, False),   # reaches the cap while extending, one rung short: serial
           (CHAIN_CAP - 3, 1, False),   # one rung fewer: the last entry is the merge: chain
           (CHAIN_CAP - 2, 0, True)]    # exactly CHAIN_CAP entries, the first cut past the segment ON b2: chain


def beyond_c(gear, win, sub, seed=151):
    """C: four segments at P1.  The true chain cuts at t = b1 - x (x = 6049) and finds nothing in
    segment 1 until its forced cut F = t + max = b2 - x; chain 1, from b1, finds nothing either and
    cuts first at F + 50.  From there the two take a ladder alternately (chain 1 the even rungs
    F + 50 + 120 i, the true chain the odd ones F + 112 + 120 i; the 50 even rungs i < 50 lie below
    b2, rung 50 is b2 + 1), and after the ladder both cut at three windows 300, 700 and 1100 bytes
    after it.
      sub 1: four rung pairs, then nothing up to b2 + 300: the chains meet there, at chain 1's
             first cut past its segment.
      sub 2: 51 pairs: chain 1's first cut past its segment is the rung b2 + 1, and the chains meet
             at its second, its last stored entry.
      sub 3: 52 pairs: chain 1's two cuts past its segment are both rungs (b2 + 1, b2 + 121), the
             true chain passes its last entry (b2 + 63, then b2 + 183) unmerged: merge[0] is none,
             the file is walked serially.  Chain 2, from b2, skips b2 + 63 and cuts at b2 + 121,
             so chain 1 itself merges on its last stored entry and is never extended: what chain
             0 compares with does not depend on which of the two waves runs first."""
    b1, b2, x = MIB, 2 * MIB, 6049
    t, F = b1 - x, b2 - x
    inside = -(-(x - 50) // 120)                             # even rungs below b2: 50
    pairs = 4 if sub == 1 else inside + (sub - 1)            # rung pairs (even, odd)
    ev = [F + 50 + 120 * i for i in range(pairs)]
    od = [F + 112 + 120 * i for i in range(pairs)]
    if sub == 1:
        z = [b2 + 300, b2 + 700, b2 + 1100]
    else:
        z = [od[-1] + 300 + 400 * i for i in range(3)]
    fe = 3 * MIB + 4000
    B = Builder(win, fe, seed + sub)
    for p in sorted([t] + ev + od + z):
        B.s(p)
    past = [p for p in ev if p >= b2]
    facts = dict(past_rungs=len(past))
    return ChainCase("beyond_c[%d]" % sub, B.done(gear), [0], [fe], P1, B.planted, "serial" if sub == 3 else "chain",
                     cuts=[t, F] + od + z, no_cuts=ev, facts=facts)


def forced_d(gear, win, empty, tail=True, seed=171):
    """D: one content cut at 3.5 MiB + 1, then `empty` candidate-free segments before the next
    planted cut (12345 bytes into the segment after them), and 777 bytes past that segment's end.
    empty = 1 is tests/cdc_plant.py's `segments`: the chain of the empty segment walks one cut
    beyond its forced cut and meets the true chain at the planted one.  With 2 or 3 the first empty
    segment's chain ends on the next segment's start, which the true chain (3.5 MiB + 1 + k max)
    never cuts: serial.  tail False: nothing follows the off-phase cut up to the file's end."""
    first = 3 * MIB + MIB // 2 + 1
    nseg = 4 + empty + 1
    fe = nseg * MIB + 777 if tail else (4 + empty) * MIB + MIB // 2
    B = Builder(win, fe, seed + empty * 2 + tail)
    pos = [MIB // 2, MIB + 400000, 2 * MIB + 300000, 3 * MIB + 200000, first]
    if tail:
        pos.append((4 + empty) * MIB + 12345)
    for p in pos:
        B.s(p)
    forced = [first + k * MIB for k in range(1, empty + 1 if tail else 99) if first + k * MIB < fe]
    return ChainCase("forced_d[%d%s]" % (empty, "" if tail else ",end"), B.done(gear), [0], [fe], P1, B.planted,
                     "chain" if empty == 1 and tail else "serial", cuts=pos + forced,
                     no_cuts=[(4 + k) * MIB for k in range(empty + 1) if (4 + k) * MIB < fe])


D_CASES = [(1, True), (2, True), (3, True), (2, False)]


def constant_byte(gear):
    """A byte value whose constant run never passes a mask: neither in the steady state (48 or
    more equal bytes) nor in a head region (1..47 equal bytes hashed from zero)."""
    for v in range(256):
        run = bytes([v]) * 64
        if all(gear.hash_prefix(run[:k]) & gear.mask_s and gear.hash_prefix(run[:k]) & gear.mask_l for k in range(1, 65)):
            return v
    raise AssertionError("every constant byte passes a mask somewhere")


F_SEGMENTS = [1, 2, 3, 5, 7, 1000, 1, 1500, 2, 13, 1, 1, 64, 3]  # per file, in 2 KiB segments (small batch)


def resolve_f(oracle):
    """F: min 64, avg 256, max 1024 and files of one constant byte that passes no mask: every chunk
    is max, every chain merges at once.  File lengths are F_SEGMENTS x 2 KiB less 0, 1 or 1023
    bytes (so the last segment is whole, one short, or half), more than 2 x 1024 segments: each of
    k_resolve's 1024 threads takes per = ceil(segments / 1024) consecutive ones, and the file
    heads fall at the start, inside and at the end of those ranges."""
    gear = cp.Gear.of(oracle, PF)
    v = constant_byte(gear)
    L = seg_len_for(PF, True)
    lens = [k * L - (0, 1, 1023)[i % 3] for i, k in enumerate(F_SEGMENTS)]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    data = np.full(sum(lens), v, dtype=np.uint8)
    return ChainCase("resolve_f", data, offs, lens, PF, [], "chain", facts=dict(byte=v)), gear


def units_g(gear, win, tiny=66000, seed=191):
    """G: `tiny` files of 0..3 bytes and three planted CDC files of three segments each (2 MiB +
    5000 bytes, one cut 150 bytes before and one 300 bytes after each inner segment start) whose
    units straddle unit indices 255 / 256 and 65,535 / 65,536 of k_unit_count's two-level scan; the
    third sits at the end.  With threshold 0 every non-empty file is a CDC file of one segment."""
    big = 2 * MIB + 5000
    # Every file is one unit except a big one, which is three: file index f starts at unit f plus 2
    # for each big file before it.  Big files at indices 254 and 65,532 take units 254..256 and
    # 65,534..65,536.  A smaller `tiny`, for the CPU test, leaves the second one out.
    at = [UNIT_BLOCK - 2] + [a for a in [UNIT_BLOCK * UNIT_BLOCK - 2 - 2] if a < tiny]
    at.append(tiny + len(at))
    nfiles = tiny + len(at)
    rng = np.random.default_rng(seed)
    lens = []
    for f in range(nfiles):
        lens.append(big if f in at else int(rng.integers(0, 4)))
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    B = Builder(win, int(sum(lens)), seed)
    # tiny files repeat a few byte patterns, so that most of them are duplicates of earlier ones
    small = np.nonzero(np.asarray(lens) < big)[0]
    for f in small:
        o, n = int(offs[f]), lens[f]
        B.buf[o:o + n] = (f % 5) + 1
    cuts = []
    for f in at:
        o = int(offs[f])
        for b in (o + MIB, o + 2 * MIB):
            cuts += [B.s(b - 150), B.s(b + 300)]
    return ChainCase("units_g", B.done(gear), offs, lens, P1, B.planted, "chain", cuts=cuts,
                     facts=dict(big=sorted(at), nunits=tiny + 3 * len(at)))


def direct_h(gear, win, seed=211):
    """H: P1, one chunk start per file with the deciding position at the edges of walk_next's body
    range [lo, hi) = [s + 111, s + r2): a planted cut exactly at lo, at lo + 63 and lo + 64 (the
    last lane of direct_scan's first step and the first of its second), at hi - 1, a window at
    hi itself (never tested: no cut), and a file longer than max without any candidate (a forced
    cut).  With the candidate array cut down to one entry all of them are direct_scan's."""
    lo = 64 + WINDOW - 1
    plan = [(4096, lo, True), (4096, lo + 63, True), (4096, lo + 64, True), (5000, 4999, True), (5001, 5000, False),
            (MIB + 1000, None, False)]
    lens = [p[0] for p in plan]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    B = Builder(win, sum(lens), seed)
    cuts, no_cuts = [], []
    for (ln, p, cut), o in zip(plan, offs.tolist()):
        if p is None:
            cuts.append(o + MIB)
        else:
            (cuts if cut else no_cuts).append(B.s(o + p))
    return ChainCase("direct_h", B.done(gear), offs, lens, P1, B.planted, "chain", cuts=cuts, no_cuts=no_cuts)


def expected_trunc(gear, data, tile, cap):
    """bw_batch_counters' trunc for a candidate array of `cap` entries: the start of the first scan
    tile whose candidates do not all fit below cap (k_compact), or NONE."""
    cand, _ = gear.census(data, tile)
    run = 0
    for t, c in enumerate(cand.tolist()):
        if run + c > cap:
            return t * tile
        run += c
    return NONE


E_THRESHOLD = 4096


def shapes_e(gear, win, seed=231):
    """E: file shapes in one P1 batch, small_file_threshold = 4096, offsets ascending and back to
    back.  (name, length, planted cuts relative to the file):
      chainX   1 MiB + 5000: two segments, cuts 150 before and 300 after the segment start
      empty, tiny (100 bytes): single blobs
      exact    exactly one segment (1 MiB), ending on the segment boundary
      plus1    1 MiB + 1: a second segment of one byte, and a last chunk of 30 bytes (<= min)
      minus1   1 MiB - 1: one segment
      atthr    4096 bytes: not above the threshold, a single blob
      serial   3.25 MiB, one cut at 0.5 MiB + 1 and nothing after it: the true chain's forced cuts
               stay off every segment start, chain 0 passes chain 1's last entry unmerged, the
               file is walked serially -- between chain-path files, so its fallback offset follows
               theirs and theirs must not be touched by it
      empty
      chainY   2 MiB + 50: a last segment of 50 bytes (<= min), cuts around both segment starts
      above    4097 bytes: the smallest CDC file, one segment, one cut"""
    plan = [("chainX", MIB + 5000, [MIB - 150, MIB + 300]), ("empty", 0, []), ("tiny", 100, []),
            ("exact", MIB, [500000]), ("plus1", MIB + 1, [400000, MIB + 1 - 30]), ("minus1", MIB - 1, [300000]),
            ("atthr", E_THRESHOLD, []), ("serial", 3 * MIB + MIB // 4, [MIB // 2 + 1]), ("empty", 0, []),
            ("chainY", 2 * MIB + 50, [MIB - 150, MIB + 300, 2 * MIB - 150]), ("above", E_THRESHOLD + 1, [2000])]
    lens = [p[1] for p in plan]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    B = Builder(win, sum(lens), seed)
    cuts = [B.s(o + c) for (_, _, cs), o in zip(plan, offs.tolist()) for c in cs]
    so = int(offs[7])
    cuts += [so + MIB // 2 + 1 + k * MIB for k in (1, 2)]
    names = [p[0] for p in plan]
    return ChainCase("shapes_e", B.done(gear), offs, lens, P1, B.planted, "serial", cuts=cuts,
                     no_cuts=[so + MIB, so + 2 * MIB, so + 3 * MIB], facts=dict(names=names, serial=[7]),
                     threshold=E_THRESHOLD)


def remainder_e(gear, win, seed=251):
    """E at P3 (avg 1 MiB, max 3 MiB; one 3 MiB segment per file): a remainder between min and avg
    makes center = rem, so mask_s holds to the end and an L-only window is no cut where an S window
    is.  Files of 900,000 bytes with one window at 500,000; files of 1 MiB + 600,000 with an S
    window at 700,000 (a cut) and the window under test 500,000 bytes into the 948,576 that remain."""
    plan = [(900000, [(500000, L_ONLY, False)]), (900000, [(500000, S, True)]),
            (MIB + 600000, [(700000, S, True), (1200000, L_ONLY, False)]),
            (MIB + 600000, [(700000, S, True), (1200000, S, True)])]
    lens = [p[0] for p in plan]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    B = Builder(win, sum(lens), seed)
    cuts, no_cuts = [], []
    for (_, ws), o in zip(plan, offs.tolist()):
        for p, kind, cut in ws:
            (cuts if cut else no_cuts).append(B.s(o + p, kind))
    return ChainCase("remainder_e", B.done(gear), offs, lens, P3, B.planted, "chain", cuts=cuts, no_cuts=no_cuts,
                     threshold=E_THRESHOLD)
