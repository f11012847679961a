"""Planted digests for the seen-chunk index: the slot hash inverted, a sequential model of the probe,
claim, verdict and rehash of backuwup_amd/csrc/bw_dedup.hip, the plain duplicate rule as reference,
one-line mutants of the model, and the cases built from them (pure Python + numpy).

The table keys a digest by fmix64 of its first 8 bytes: the slot index is the hash's low bits, the
tag its top 24 bits, and a slot whose tag matches is compared by the whole 32-byte digest it names.
With random digests no two share a tag in one probe run, so nothing after the tag compare ever
decides.  fmix64 is a bijection (two odd multipliers and three xor-shifts), so digest(h, tail) builds
a digest with ANY chosen 64-bit slot hash h: slot, tag and the bits in neither are free, and so is
the 24-byte tail the slot hash does not see.  A hash whose low 20 bits are all ones has its home in
the last slot at every capacity up to 2^20.

Nothing here holds a literal of the kernel's constants: the multipliers, the shift and SEQ_BITS are
read out of bw_dedup.hip, the first capacities and the doubling rule out of index_capacity() in
bw_capi.hip, and a pattern that no longer matches raises (a planter that silently stopped planting
after a change of the hash would hide what it is for).

Model restates claim() and the verdict loop over a Python list; it predicts the PATH (the census:
which probes met an equal tag and a different digest, wraps, edge words, where a match's digest was
read from, what each growth re-claimed).  Verdicts are never taken from it: every case is compared
with reference(), the rule of the kernel file's header (a Python set of bytes), and the model itself
must agree with that rule.  tests/test_index_plant.py checks all of this on the CPU;
tests/test_gpu_index_planted.py runs the cases on the GPU.
"""
import functools
import os
import re

import numpy as np

M64 = (1 << 64) - 1
EMPTY = M64                      # SLOT_EMPTY
ZERO32 = bytes(32)               # what a log entry holds before its batch has written it
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "backuwup_amd", "csrc")


# ------------------------------------------------------------------ the kernel's constants, from its sources

def _source(name):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _body(src, head, name):
    """The text of the function whose signature matches `head`, up to the next line-initial '}'."""
    m = re.search(head, src)
    if not m:
        raise RuntimeError("index_plant: %s not found; the planter must be re-derived from the source" % name)
    end = src.index("\n}", m.end())
    return src[m.end():end]


def _need(pattern, text, what, count=None):
    found = re.findall(pattern, text)
    if not found or (count is not None and len(found) != count):
        raise RuntimeError("index_plant: %s no longer matches (%d hits for %r); the planter must be re-derived "
                           "from the source" % (what, len(found), pattern))
    return found


def _read_constants():
    dedup, capi = _source("bw_dedup.hip"), _source("bw_capi.hip")
    mix = _body(dedup, r"uint64_t fmix64\(uint64_t k\) \{", "fmix64")
    steps = _need(r"k (\^= k >> \d+|\*= 0x[0-9a-fA-F]+ull);", mix, "fmix64's steps", 5)
    if [s[0] for s in steps] != ["^", "*", "^", "*", "^"]:
        raise RuntimeError("index_plant: fmix64 is no longer shift, multiply, shift, multiply, shift; the planter "
                           "must be re-derived from the source")
    shifts = {int(s.split(">>")[1]) for s in steps[0::2]}
    if len(shifts) != 1:
        raise RuntimeError("index_plant: fmix64's three shifts differ; the planter must be re-derived")
    c = {"shift": shifts.pop(), "mul": [int(s.split("0x")[1][:-3], 16) for s in steps[1::2]]}
    c["seq_bits"] = int(_need(r"constexpr int SEQ_BITS = (\d+);", dedup, "SEQ_BITS", 1)[0])
    # the first 8 digest bytes little-endian, the slot from the low bits, the tag above the position
    _need(r"fmix64\(\(\(uint64_t\)d\.a\.y << 32\) \| d\.a\.x\)", dedup, "dig_hash's byte order", 1)
    _need(r"h = dig_hash\(d\), tag = h >> SEQ_BITS;", dedup, "the tag's place in the hash", 2)
    _need(r"uint64_t s = h & mask", dedup, "the slot's place in the hash", 2)
    _need(r"\(tag << SEQ_BITS\) \| seq", dedup, "the table word's layout", 1)
    _need(r"s = \(s \+ 1\) & mask", dedup, "the linear probe", 2)
    _need(r"constexpr uint64_t SLOT_EMPTY = ~0ull;", dedup, "SLOT_EMPTY", 1)
    cap = _body(capi, r"static int index_capacity\(bw_ctx\* c, uint64_t incoming, hipStream_t st\) \{",
                "index_capacity()")
    c["log_cap0"] = 1 << int(_need(r"x->log_cap \? x->log_cap : 1 << (\d+);", cap, "the first log capacity", 1)[0])
    c["table_cap0"] = 1 << int(_need(r"x->table_cap \? x->table_cap : 1 << (\d+);", cap,
                                     "the first table capacity", 1)[0])
    _need(r"if \(need_log \* 2 > x->table_cap\)", cap, "the table's half-full rule", 1)
    _need(r"while \(cap < need_log \* 2\) cap \*= 2;", cap, "the table's doubling", 1)
    _need(r"if \(need_log > x->log_cap\)", cap, "the log's growth rule", 1)
    _need(r"while \(cap < need_log\) cap \*= 2;", cap, "the log's doubling", 1)
    _need(r"\(x->log_hi \+ incoming\) > x->log_cap \|\| \(x->log_hi \+ incoming\) \* 2 > x->table_cap", cap,
          "the read of the log length before a growth", 1)
    _need(r"x->log_hi = std::min\(x->log_hi, len\);", cap, "the tightening of the bound before a growth", 1)
    reset = _body(capi, r"static int index_reset_locked\(bw_ctx\* c, uint64_t hint, hipStream_t st\) \{",
                  "index_reset_locked()")
    c["reset_hint"] = int(_need(r"index_capacity\(c, hint \? hint : (\d+), st\)", reset,
                                "the reset's default hint", 1)[0])
    return c


C = _read_constants()
SHIFT, MUL1, MUL2 = C["shift"], C["mul"][0], C["mul"][1]
SEQ_BITS = C["seq_bits"]
SEQ_MASK = (1 << SEQ_BITS) - 1
TAG_BITS = 64 - SEQ_BITS
TAG_MAX = (1 << TAG_BITS) - 1
TABLE_CAP0, LOG_CAP0, RESET_HINT = C["table_cap0"], C["log_cap0"], C["reset_hint"]
LOW_BITS = 20                    # the planted slots hold at every capacity up to 2^LOW_BITS
LAST = (1 << LOW_BITS) - 1       # low bits of a hash whose home is the last slot at all of them
assert TABLE_CAP0 == 1 << 16 and SEQ_BITS >= LOW_BITS + 4, "the cases below plant bits 16..19 and 20..SEQ_BITS"


# ------------------------------------------------------------------ the hash and its inverse

def fmix64(k):
    k ^= k >> SHIFT
    k = k * MUL1 & M64
    k ^= k >> SHIFT
    k = k * MUL2 & M64
    k ^= k >> SHIFT
    return k


def _unshift(k):
    """x with x ^ (x >> SHIFT) == k (for SHIFT >= 32 the xor-shift is its own inverse)."""
    x, s = k, SHIFT
    while s < 64:
        x = k ^ (x >> SHIFT)
        s += SHIFT
    return x


_INV1, _INV2 = pow(MUL1, -1, 1 << 64), pow(MUL2, -1, 1 << 64)


def fmix64_inv(h):
    h = _unshift(h)
    h = h * _INV2 & M64
    h = _unshift(h)
    h = h * _INV1 & M64
    return _unshift(h)


def fmix64_np(k):
    k = np.asarray(k, dtype=np.uint64).copy()
    s = np.uint64(SHIFT)
    k ^= k >> s
    k *= np.uint64(MUL1)
    k ^= k >> s
    k *= np.uint64(MUL2)
    k ^= k >> s
    return k


def slot_hash(low, tag, mid=0):
    """The 64-bit slot hash with the given low LOW_BITS bits, the bits between them and the tag, and the tag."""
    assert 0 <= low <= LAST and 0 <= tag <= TAG_MAX and 0 <= mid < 1 << (SEQ_BITS - LOW_BITS)
    return tag << SEQ_BITS | mid << LOW_BITS | low


def digest(h, tail24):
    """32 bytes whose slot hash is h: fmix64_inv(h) little-endian, then the 24 bytes the hash ignores."""
    tail24 = bytes(tail24)
    assert len(tail24) == 24
    return fmix64_inv(h).to_bytes(8, "little") + tail24


def hash_of(d):
    """dig_hash of one digest (bytes)."""
    return fmix64(int.from_bytes(bytes(d[:8]), "little"))


def hashes(digests):
    """dig_hash of every row of an (n, 32) uint8 array -> list of Python ints."""
    d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
    return [int(x) for x in fmix64_np(np.ascontiguousarray(d[:, :8]).view("<u8").reshape(-1))]


def as_array(rows):
    """[bytes] -> (n, 32) uint8."""
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 32).copy()


# ------------------------------------------------------------------ index_capacity()

class Capacity:
    """The host side of the index: the bound log_hi, the real log length, and the two capacities, as
    index_capacity(), index_reset_locked() and the result reads of bw_capi.hip move them."""

    def __init__(self, reset_hint=None):
        """A fresh context's first operation: the gate resets with the default hint, bw_index_reset
        with its own."""
        self.log_hi = self.log_len = 0
        self.log_cap = self.table_cap = 0
        self._room(reset_hint or RESET_HINT)

    def _room(self, incoming):
        """-> whether the table grew (and was rebuilt from the log)."""
        if self.table_cap and (self.log_hi + incoming > self.log_cap or (self.log_hi + incoming) * 2 > self.table_cap):
            self.log_hi = min(self.log_hi, self.log_len)  # the length is read before anything grows
        need = self.log_hi + incoming
        if need > self.log_cap:
            cap = self.log_cap or LOG_CAP0
            while cap < need:
                cap *= 2
            self.log_cap = cap
        if need * 2 > self.table_cap:
            cap = self.table_cap or TABLE_CAP0
            while cap < need * 2:
                cap *= 2
            old, self.table_cap = self.table_cap, cap
            return bool(old)
        return False

    def gate(self, max_n, n=None):
        """One gate call bounded by max_n that appends n (default max_n) -> whether the table grew."""
        n = max_n if n is None else n
        assert n <= max_n
        if not max_n:
            return False
        grew = self._room(max_n)
        self.log_hi += max_n
        self.log_len += n
        return grew

    def read(self):
        """A result read (bw_index_size, bw_index_check, the host gate's own) with nothing in flight."""
        self.log_hi = min(self.log_hi, self.log_len)


def capacity_after(log_bounds, reset_hint=None, read=True):
    """[(table capacity, log capacity)] after each gate call of a fresh context.  An entry of
    log_bounds is a call's max_n, or (max_n, n) where fewer are appended than the bound; read: a
    result read follows every call (the tests read the size after every batch)."""
    c, out = Capacity(reset_hint), []
    for b in log_bounds:
        max_n, n = b if isinstance(b, tuple) else (b, b)
        c.gate(max_n, n)
        if read:
            c.read()
        out.append((c.table_cap, c.log_cap))
    return out


# ------------------------------------------------------------------ the model

MUTANTS = ("eq28", "eq8", "tag_only", "from_log", "from_batch", "no_min", "rehash_unique", "rehash_old_mask")
CENSUS_KEYS = ("tag_eq_dig_ne", "tag_ne", "wraps", "longest_run", "from_batch", "from_log", "zero_words",
               "tag_max_slots")


class Model:
    """claim(), the verdict loop and the rehash, one digest after the other.

    The kernel's claims of one launch run in any order; `order` picks the model's ("forward":
    canonical, "reverse": the last position first).  Verdicts must not depend on it: the minimum
    kept in the slot is what makes the first occurrence win.

    mutant: one way a kernel could be wrong without faulting --
      eq28 / eq8       the digest compare reads the first 28 / 8 bytes only
      tag_only         a slot with an equal tag counts as equal
      from_log         a matching slot's digest is always read from the log; the entries of the
                       running batch are not written yet when its claims read them (ZERO32)
      from_batch       ... always from the batch array, with the index clamped into it
      no_min           the last claimer's position stays in the slot
      rehash_unique    a growth re-claims as many log entries as there were distinct digests
      rehash_old_mask  a growth re-claims with the mask of the table it replaces
    """

    def __init__(self, reset_hint=None, mutant=None, order="forward"):
        assert mutant is None or mutant in MUTANTS
        assert order in ("forward", "reverse")
        self.mutant, self.order = mutant, order
        self.cap = Capacity(reset_hint)
        self.table = [EMPTY] * self.cap.table_cap
        self.log, self.log_h = [], []
        self.nunique = 0
        self.lost = False
        self.census = []      # one dict per call (seed included)
        self.growths = []     # one dict per growth: entries re-claimed, and the rebuild's own census

    # -- the compare
    def _eq(self, a, b):
        if self.mutant == "eq28":
            return a[:28] == b[:28]
        if self.mutant == "eq8":
            return a[:8] == b[:8]
        if self.mutant == "tag_only":
            return True
        return a == b

    def _digest_at(self, w, base, batch, claiming):
        """digest_at(): -> (digest, came from the batch array)."""
        if batch is None:  # the rehash: every entry from the log
            return self.log[w], False
        if self.mutant == "from_log":
            if w >= base:
                return (ZERO32 if claiming else self.log[w]), False
            return self.log[w], False
        if self.mutant == "from_batch":
            return batch[min((w - base) & M64, len(batch) - 1)], True
        return (batch[w - base], True) if w >= base else (self.log[w], False)

    def _claim(self, table, mask, d, h, seq, base, batch, c):
        tag = h >> SEQ_BITS
        mine = tag << SEQ_BITS | seq
        s, run = h & mask, 0
        for _ in range(mask + 1):
            run += 1
            v = table[s]
            if v == EMPTY:
                table[s] = mine
                break
            if v >> SEQ_BITS == tag:
                other, in_batch = self._digest_at(v & SEQ_MASK, base, batch, True)
                if self._eq(other, d):
                    c["from_batch" if in_batch else "from_log"] += 1
                    table[s] = mine if self.mutant == "no_min" else min(v, mine)
                    break
                c["tag_eq_dig_ne"] += 1
            else:
                c["tag_ne"] += 1
            s = (s + 1) & mask
            if s == 0:
                c["wraps"] += 1
        c["longest_run"] = max(c["longest_run"], run)

    def _grow(self):
        c = dict.fromkeys(CENSUS_KEYS, 0)
        cap = self.cap.table_cap
        mask = (len(self.table) if self.mutant == "rehash_old_mask" else cap) - 1
        n = self.nunique if self.mutant == "rehash_unique" else len(self.log)
        table = [EMPTY] * cap
        for i in range(n):
            self._claim(table, mask, self.log[i], self.log_h[i], i, M64, None, c)
        c["entries"], c["table_cap"] = n, cap
        self.table = table
        self.growths.append(c)

    def gate(self, digests, max_n=None, read=True):
        """One launch_dedup over an (n, 32) array -> verdicts (uint8); appends the call's census."""
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        n = len(d)
        batch, hs = [x.tobytes() for x in d], hashes(d)
        if self.cap.gate(n if max_n is None else max_n, n):
            self._grow()
        table, mask = self.table, len(self.table) - 1
        base = len(self.log)
        c = dict.fromkeys(CENSUS_KEYS, 0)
        for i in (range(n) if self.order == "forward" else range(n - 1, -1, -1)):
            self._claim(table, mask, batch[i], hs[i], base + i, base, batch, c)
        self.log.extend(batch)
        self.log_h.extend(hs)
        out = np.zeros(n, dtype=np.uint8)
        for i in range(n):
            seq, tag, s, w = base + i, hs[i] >> SEQ_BITS, hs[i] & mask, EMPTY
            for _ in range(mask + 1):
                v = table[s]
                if v == EMPTY:
                    break
                if v >> SEQ_BITS == tag and (v & SEQ_MASK == seq or
                                             self._eq(self._digest_at(v & SEQ_MASK, base, batch, False)[0], batch[i])):
                    w = v & SEQ_MASK
                    break
                s = (s + 1) & mask
            if w == seq:
                self.nunique += 1
            else:
                out[i] = 1
                self.lost |= w == EMPTY
        c["zero_words"] = table.count(0)
        c["tag_max_slots"] = sum(1 for v in table if v != EMPTY and v >> SEQ_BITS == TAG_MAX)
        c["n"], c["table_cap"] = n, len(table)
        self.census.append(c)
        if read:
            self.cap.read()
        return out

    def homes(self, digests, cap=None):
        """The home slots of the digests at table capacity cap (default: the current one)."""
        mask = (cap or len(self.table)) - 1
        return [h & mask for h in hashes(digests)]


def total(census):
    """The sum of a list of per-call census dicts (the longest run: their maximum)."""
    out = dict.fromkeys(CENSUS_KEYS, 0)
    for c in census:
        for k in CENSUS_KEYS:
            out[k] = max(out[k], c[k]) if k in ("longest_run", "zero_words", "tag_max_slots") else out[k] + c[k]
    return out


def run_model(case, **kw):
    """The case through a Model -> (verdicts per batch, distinct count after each batch, the model).
    The seed is a call of its own ahead of the batches (census[0]); it has no verdicts."""
    seed, batches = case
    m = Model(**kw)
    if seed is not None and len(seed):
        m.gate(seed)
    verdicts, counts = [], []
    for b in batches:
        verdicts.append(m.gate(b))
        counts.append(m.nunique)
    return verdicts, counts, m


# ------------------------------------------------------------------ the reference

def reference(batches, seed=None):
    """The rule of bw_dedup.hip's header: position i is a duplicate iff its digest was seeded or
    appears at an earlier canonical position -> (verdicts per batch, distinct count after each)."""
    seen = set() if seed is None else {x.tobytes() for x in np.asarray(seed, dtype=np.uint8).reshape(-1, 32)}
    verdicts, counts = [], []
    for b in batches:
        v = np.zeros(len(b), dtype=np.uint8)
        for i, x in enumerate(np.asarray(b, dtype=np.uint8).reshape(-1, 32)):
            k = x.tobytes()
            if k in seen:
                v[i] = 1
            else:
                seen.add(k)
        verdicts.append(v)
        counts.append(len(seen))
    return verdicts, counts


def reference_oracle(oracle, batches, seed=None):
    """The same through the CPU oracle's BlobIndex restatement (sorted seed + queued set)."""
    ix = oracle.Index(b"" if seed is None else np.ascontiguousarray(seed, dtype=np.uint8).tobytes())
    verdicts = []
    for b in batches:
        v = np.zeros(len(b), dtype=np.uint8)
        for i, x in enumerate(np.asarray(b, dtype=np.uint8).reshape(-1, 32)):
            k = x.tobytes()
            v[i] = ix.is_blob_duplicate(k)
            ix.insert(k)
        verdicts.append(v)
    return verdicts


# ------------------------------------------------------------------ planted clusters

def _tail(seed):
    return np.random.default_rng(seed).integers(0, 256, 24, dtype=np.uint8).tobytes()


def member(h, tail, k):
    """The k-th digest of slot hash h: the base tail with ONE byte changed, byte k % 24 (k = 23 and
    47 change the digest's 32nd byte); k = -1 is the base tail itself.  Distinct k, distinct digests."""
    if k < 0:
        return digest(h, tail)
    t = bytearray(tail)
    t[k % 24] ^= 0xFF - k // 24
    assert 0 <= k < 24 * 255
    return digest(h, t)


H_CT = slot_hash(LAST, 0x5EED01, 0x9ABCD)           # cluster_tail: one hash, home in the last slot
T_CT = _tail(101)
TAGS = (0, TAG_MAX, 1, 0x800000, 0x7FFFFF, 0xFFFFFE, 0x00FFFF, 0xA5A5A5)   # tags: the edge tags first
H_TAGS = tuple(slot_hash(LAST, t, 0x11111 * (i + 1) & 0xFFFFF) for i, t in enumerate(TAGS))
T_TAGS = _tail(102)
TAG_MEMBERS = (23, 20, 0, 11)                       # bytes 32 and 29 (equal in the first 28), 9 and 20
IB_LOW, IB_TAG_A, IB_TAG_B = 0x2B3C5, 0x00ABCD, 0x00BEEF
T_IB = _tail(103)
W1_TAGS = tuple(0x0A0000 + 0x111 * j for j in range(10))
H_W1 = tuple(slot_hash(LAST, t, 0x00F0F) for t in W1_TAGS)   # wrap: 10 tags x 4 tails, home in the last slot
H_W2 = tuple(slot_hash(3, 0x0B0000 + j, 0x12345) for j in range(5))  # 5 tags x 2 tails, home in slot 3
T_W = _tail(104)
H_HOT = slot_hash(LAST, 0xC0FFEE, 0x0CAFE)          # contend: the ten hot digests of one hash
T_HOT = _tail(105)


def h_ignored_a(k):
    """Same slot and tag at every capacity up to 2^20; the hashes differ in bits 20..39 only."""
    return slot_hash(IB_LOW, IB_TAG_A, (k * 0x10101 + 1) & 0xFFFFF)


def h_ignored_b(k):
    """Same slot at 2^16, the same tag; the hashes differ in bits 16..19 only."""
    assert 0 <= k < 16
    return slot_hash((IB_LOW & 0xFFFF) ^ 0x7E57 | k << 16, IB_TAG_B, 0x54321)


def _shuffled(rows, seed):
    rows = list(rows)
    return [rows[i] for i in np.random.default_rng(seed).permutation(len(rows))]


def decoys():
    """Planted digests that are in no batch of any case: members of the last-slot cluster, of the
    hash every `tags` digest of tag 0 has, and of the ignored-bits slot."""
    rows = [member(H_CT, T_CT, 2000 + k) for k in range(24)]
    rows += [member(H_TAGS[0], T_TAGS, 2000 + k) for k in range(8)]
    rows += [member(h_ignored_a(500 + k), T_IB, -1) for k in range(8)]
    return as_array(rows)


# ------------------------------------------------------------------ the cases: -> (seed or None, [batches])

def _ct_rows():
    first = [member(H_CT, T_CT, k) for k in range(24)]          # one digest per tail byte position
    new = [member(H_CT, T_CT, -1)] + [member(H_CT, T_CT, 24 + k) for k in range(7)]
    return first, new


def cluster_tail():
    first, new = _ct_rows()
    b1 = first + first[0::2]
    b2 = _shuffled(first + new + new, 201)  # matches from the log and from the batch in one launch
    return None, [as_array(b1), as_array(b2)]


def _tag_rows():
    first = [member(h, T_TAGS, k) for k in TAG_MEMBERS for h in H_TAGS]  # tag 0 first, the tags interleaved
    new = [member(h, T_TAGS, 17) for h in H_TAGS]
    return first, new


def tags():
    first, new = _tag_rows()
    assert hash_of(first[0]) >> SEQ_BITS == 0  # log position 0 on a fresh index: the table word 0
    b1 = first + first[1::3]
    b2 = _shuffled(first + new + new, 202)
    return None, [as_array(b1), as_array(b2)]


def _ib_rows():
    a = [member(h_ignored_a(k), T_IB, -1) for k in range(16)]
    b = [member(h_ignored_b(k), T_IB, -1) for k in range(16)]
    new = [member(h_ignored_a(16), T_IB, -1), member(h_ignored_b(0), T_IB, 7)]
    return a, b, new


def ignored_bits():
    a, b, new = _ib_rows()
    b1 = a + b + _shuffled(a + b, 203)
    b2 = _shuffled(a + b + new + new, 204)
    return None, [as_array(b1), as_array(b2)]


def _wrap_rows():
    w1 = [member(h, T_W, k) for k in (23, 21, 12, 6) for h in H_W1]   # 40 homes in the last slot
    w2 = [member(h, T_W, k) for k in (23, 2) for h in H_W2]          # 10 in slot 3, which the spill covers
    new = [member(H_W1[0], T_W, 30), member(H_W2[0], T_W, 30)]
    return w1, w2, new


def wrap():
    w1, w2, new = _wrap_rows()
    b1 = w1 + w2 + _shuffled(w1 + w2, 205)
    b2 = _shuffled(w1 + w2 + new + new, 206)
    return None, [as_array(b1), as_array(b2)]


CONTEND_N, CONTEND_HOT, CONTEND_REPEATS, CONTEND_SHARED = 20000, 50, 300, 10


def contend():
    """One batch: 50 hot digests, 300 occurrences each, ten of them of one hash.  Hot digest k
    occurs only at positions >= contend_from(k), so the first occurrence of the later ones lies in a
    late block while most of their claims come from other blocks."""
    rng = np.random.default_rng(207)
    hot = [member(H_HOT, T_HOT, k) for k in range(CONTEND_SHARED)]
    hot += [x.tobytes() for x in rng.integers(0, 256, (CONTEND_HOT - CONTEND_SHARED, 32), dtype=np.uint8)]
    hot = _shuffled(hot, 208)  # the shared-hash ten spread over early and late starts
    label = np.full(CONTEND_N, -1, dtype=np.int64)
    for k in range(CONTEND_HOT - 1, -1, -1):
        free = np.flatnonzero(label[contend_from(k):] < 0) + contend_from(k)
        label[rng.permutation(free)[:CONTEND_REPEATS]] = k
    d = rng.integers(0, 256, (CONTEND_N, 32), dtype=np.uint8)  # the singles
    for k in range(CONTEND_HOT):
        d[label == k] = np.frombuffer(hot[k], dtype=np.uint8)
    return None, [d]


def contend_from(k):
    return 0 if k < 25 else (k - 24) * 600


GROW_FILLER, GROW_TAIL = 9000, 256


def _probe(planted, new, seed, extra=()):
    """Every planted digest again (all duplicates), one new member per cluster and its repeat."""
    return as_array(_shuffled(list(planted) + list(new) + list(new) + list(extra), seed))


def _grow_new(r):
    """Round r's new member of every cluster planted in `grow`."""
    return [member(H_CT, T_CT, 40 + r), member(h_ignored_a(20 + r), T_IB, -1), member(h_ignored_b(r), T_IB, 9),
            member(H_W1[1], T_W, 40 + r), member(H_W2[1], T_W, 40 + r)]


def grow():
    """The planted clusters, then random filler until the log has passed half of the first table
    capacity (the first growth and rehash) and then the first log capacity (the log's reallocation
    with its copy, and the second rehash).  After each, a probe batch: every planted digest again,
    a new member per cluster, and the last digests of every filler batch so far (the entries a
    rebuild from too short a log would miss)."""
    batches = cluster_tail()[1] + ignored_bits()[1] + wrap()[1]
    planted = list(dict.fromkeys(x.tobytes() for b in batches for x in b))
    rng = np.random.default_rng(209)
    cap, tails, r = Capacity(), [], 0
    for b in batches:
        cap.gate(len(b))
    while r < 2:
        f = rng.integers(0, 256, (GROW_FILLER, 32), dtype=np.uint8)
        grew = cap.gate(len(f))
        batches.append(f)
        if grew:  # this filler call grew the table: probe behind it
            new = _grow_new(r)
            p = _probe(planted, new, 210 + r, [x.tobytes() for t in tails for x in t])
            assert not cap.gate(len(p))  # the growths are the filler's
            batches.append(p)
            planted += new
            r += 1
        tails.append(f[-GROW_TAIL:])
    return None, batches


def seeded():
    ct, ct_new = _ct_rows()
    tg, tg_new = _tag_rows()
    planted = ct + tg
    seed = as_array(sorted(planted))
    new1 = ct_new[:4] + tg_new[:4]
    new2 = ct_new[4:] + tg_new[4:]
    b1 = _probe(planted, new1, 211)
    b2 = _probe(planted + new1, new2, 212)
    return seed, [b1, b2]


CASES = {"cluster_tail": cluster_tail, "tags": tags, "ignored_bits": ignored_bits, "wrap": wrap,
         "contend": contend, "grow": grow, "seeded": seeded}


@functools.lru_cache(maxsize=None)
def case(name):
    """(seed, batches) of a case, built once; the arrays are read-only."""
    seed, batches = CASES[name]()
    for a in batches + ([] if seed is None else [seed]):
        a.setflags(write=False)
    return seed, tuple(batches)


@functools.lru_cache(maxsize=None)
def expected(name):
    """reference() of a case, computed once and shared."""
    seed, batches = case(name)
    verdicts, counts = reference(batches, seed)
    for v in verdicts:
        v.setflags(write=False)
    return tuple(verdicts), tuple(counts)


# ------------------------------------------------------------------ the layouts of the GPU test

PRESIZE = 200_000     # bw_index_reset's hint for the run of `grow` that must not grow
BUCKET_SLACK = 300    # unused slots per bucket: more than one 256-thread block of the gate stays empty


def bucket_layout(n, n_src):
    """A batch of n as n_src exchange buckets, source-major = canonical order
    -> (counts, slots per bucket, the gate's bound n_src x slots)."""
    counts = np.full(n_src, n // n_src, dtype=np.int64)
    counts[:n % n_src] += 1
    cap = int(counts.max()) + BUCKET_SLACK
    return counts, cap, n_src * cap


def buckets(batch, n_src, fill):
    """-> (the (n_src, cap, 32) bucket array, counts, cap): the batch in the counted slots, and in
    every slot beyond a count a digest of `fill` (digests that are NOT part of the batch)."""
    counts, cap, _ = bucket_layout(len(batch), n_src)
    out = np.asarray(fill, dtype=np.uint8).reshape(-1, 32)[np.arange(n_src * cap) % len(fill)].reshape(n_src, cap, 32)
    out = np.ascontiguousarray(out)
    at = 0
    for s, c in enumerate(counts):
        out[s, :c] = batch[at:at + c]
        at += c
    return out, counts, cap
