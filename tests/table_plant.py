"""Planted keys, names and rows for the read side's open-addressing tables: the locator's three tables
(rs_insert / rs_find, bw_restore.h), the two name joins (k_df_join / k_df_pair, bw_diff.hip, and
k_pm_build / k_pm_probe, bw_parent.hip) and the diff walk's row set (k_df_insert / df_find).  Pure
Python + numpy; a helper, not a test.

All of them probe linearly from rs_mix of the key's first 8 bytes (or of an FNV of a name) and tell keys
that share a slot apart by a whole-key compare.  With BLAKE3 outputs and ordinary file names at a load of
one half no two keys share 8 bytes, runs are a slot or two long and none needs to cross the table's end.
rs_mix is the low 32 bits of a 64-bit bijection (an xor-shift that is its own inverse and a multiply by
an odd number), so key8() builds the 8 leading key bytes of ANY chosen home; names are found by a bounded
search over short ASCII names.

Nothing here holds a literal of the kernels' constants: shift, multiplier, byte order, salt position, FNV
offset and prime, the joins' seeds, the row hash's node mix and the capacity rules are read out of the
sources by read_constants(), and a pattern that no longer matches raises.

Table is a sequential model of insert and find over a Python list.  It is used for STRUCTURE: which
slots a case occupies, whether a run crosses the table's end, how long the probes are (the occupied set
of linear probing does not depend on the order of insertion, so these hold on the device whatever order
the lanes win in).  Answers are never taken from it: every case carries its expected result by
construction, and tests/test_table_plant.py holds both equal to restore_ref / prune_ref, diff_ref and
parent_ref.  The model's one-line mutants (MUTANTS) show what each case is there to catch.
tests/test_gpu_tables_planted.py runs the cases on the device.
"""
import functools
import os
import re
import struct
from collections import Counter

import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
NONE = M64
ZERO = bytes(32)
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "backuwup_amd", "csrc")
SOURCES = ("bw_restore.h", "bw_restore.hip", "bw_walk.h", "bw_diff.hip", "bw_diff_host.h", "bw_parent.hip",
           "bw_parent_host.h")


# ------------------------------------------------------------------ the kernels' constants, from their sources

def sources():
    out = {}
    for name in SOURCES:
        with open(os.path.join(_CSRC, name)) as f:
            out[name] = f.read()
    return out


def _body(src, head, name):
    """The text of the function whose signature matches `head`, up to the next line-initial '}'."""
    m = re.search(head, src)
    if not m:
        raise RuntimeError("table_plant: %s not found; the planter must be re-derived from the source" % name)
    return src[m.end():src.index("\n}", m.end())]


def _need(pattern, text, what, count=1):
    found = re.findall(pattern, text)
    if len(found) != count:
        raise RuntimeError("table_plant: %s no longer matches (%d hits for %r); the planter must be re-derived "
                           "from the source" % (what, len(found), pattern))
    return found


def read_constants(src=None):
    """The constants of the tables out of the source texts {file name: text} (default: the tree's)."""
    src = sources() if src is None else src
    rh, rhip, wk = src["bw_restore.h"], src["bw_restore.hip"], src["bw_walk.h"]
    c = {}
    mix = _body(rh, r"uint32_t rs_mix\(uint64_t x\) \{", "rs_mix")
    steps = _need(r"x (\^= x >> \d+|\*= 0x[0-9a-fA-F]+ull);", mix, "rs_mix's steps", 3)
    if [s[0] for s in steps] != ["^", "*", "^"] or steps[0] != steps[2]:
        raise RuntimeError("table_plant: rs_mix is no longer shift, multiply, the same shift; the planter must be "
                           "re-derived from the source")
    _need(r"return \(uint32_t\)x;", mix, "rs_mix's truncation")
    c["shift"] = int(steps[0].split(">>")[1])
    c["mul"] = int(steps[1].split("0x")[1][:-3], 16)
    if c["shift"] < 32 or not c["mul"] & 1:
        raise RuntimeError("table_plant: rs_mix's shift is below 32 or its multiplier even: it is not inverted this way")
    _need(r"v \|= \(uint64_t\)p\[i\] << \(8 \* i\);", _body(rh, r"uint64_t rs_load8\(const uint8_t\* p\) \{", "rs_load8"),
          "rs_load8's byte order")
    _need(r"rs_mix\(rs_load8\(key\) \^ \(\(uint64_t\)salt << 32\)\)", rh, "the salt's place in rs_insert and rs_find", 2)
    _need(r"\(h \+ probe\) & \(cap - 1\)", rh, "the locator's linear probe", 2)
    c["empty"] = int(_need(r"constexpr uint32_t RS_EMPTY = (0x[0-9a-fA-F]+)u;", rh, "RS_EMPTY")[0], 16)
    kh = _body(wk, r"uint32_t wk_key_hash\(uint64_t seed, const uint8_t\* p, uint64_t len\) \{", "wk_key_hash")
    c["fnv_offset"] = int(_need(r"uint64_t h = (0x[0-9a-fA-F]+)ull \^ seed;", kh, "the FNV offset")[0], 16)
    c["fnv_prime"] = int(_need(r"h = \(h \^ p\[i\]\) \* (0x[0-9a-fA-F]+)ull;", kh, "the FNV step")[0], 16)
    _need(r"return rs_mix\(h\);", kh, "the mix of the FNV")
    c["df_seed_mul"] = int(_need(r"wk_key_hash\(\(n\.parent \* (0x[0-9a-fA-F]+)ull\) \^ side,", src["bw_diff.hip"],
                                 "df_key_hash's seed")[0], 16)
    c["pm_seed_mul"] = int(_need(r"wk_key_hash\(item \* (0x[0-9a-fA-F]+)ull,", src["bw_parent.hip"],
                                 "pm_key_hash's seed")[0], 16)
    _need(r"rs_mix\(\*\(const uint64_t\*\)row \^ \(\(uint64_t\)node << 32\) \^ node\)", src["bw_diff.hip"],
          "df_row_hash's node mix")
    _need(r"\(h \+ probe\) & \(cap - 1\)", src["bw_diff.hip"], "the diff walk's linear probes", 4)
    _need(r"\(h \+ probe\) & \(cap - 1\)", src["bw_parent.hip"], "the parent match's linear probes", 2)
    p2 = _body(rhip, r"uint32_t pow2_cap\(uint64_t n\) \{", "pow2_cap")
    c["pow2_floor"] = int(_need(r"uint64_t c = (\d+);", p2, "pow2_cap's floor")[0])
    _need(r"while \(c < 2 \* n\) c <<= 1;", p2, "pow2_cap's doubling")
    dc = _body(src["bw_diff_host.h"], r"uint32_t df_table_cap\(uint64_t n\) \{", "df_table_cap")
    c["df_floor"] = int(_need(r"uint64_t cap = (\d+);", dc, "df_table_cap's floor")[0])
    _need(r"while \(cap < 2 \* n && cap < \(1ull << 31\)\) cap <<= 1;", dc, "df_table_cap's doubling")
    _need(r"pm_table_cap\(uint64_t n\) \{ return df_table_cap\(n\); \}", src["bw_parent_host.h"], "pm_table_cap")
    return c


C = read_constants()
SHIFT, MUL, EMPTY = C["shift"], C["mul"], C["empty"]
_INV = pow(MUL, -1, 1 << 64)


def pow2_cap(n):
    c = C["pow2_floor"]
    while c < 2 * n:
        c <<= 1
    return c


def df_table_cap(n):
    c = C["df_floor"]
    while c < 2 * n and c < 1 << 31:
        c <<= 1
    return c


pm_table_cap = df_table_cap


# ------------------------------------------------------------------ the hashes and the inverse

def mix64(x):
    """The 64-bit bijection whose low 32 bits are rs_mix."""
    x ^= x >> SHIFT
    x = x * MUL & M64
    return x ^ (x >> SHIFT)


def mix64_inv(h):
    h ^= h >> SHIFT                  # for a shift of 32 or more the xor-shift is its own inverse
    h = h * _INV & M64
    return h ^ (h >> SHIFT)


def rs_mix(x):
    return mix64(x) & M32


def load8(key):
    return int.from_bytes(bytes(key[:8]), "little")


def key_home(key, salt=0):
    """rs_insert's and rs_find's 32-bit hash of a key (bytes) under a salt."""
    return rs_mix(load8(key) ^ (salt << 32))


def key8(home_bits, salt=0, hi=0):
    """The 8 leading key bytes whose 32-bit hash under `salt` is home_bits: the home is its low bits at
    every capacity.  hi: the 32 bits of the bijection's value that rs_mix drops; distinct hi, distinct keys."""
    assert 0 <= home_bits <= M32 and 0 <= hi <= M32 and 0 <= salt <= M32
    return (mix64_inv(hi << 32 | home_bits) ^ (salt << 32)).to_bytes(8, "little")


def digest(h64, tail):
    """32 bytes whose (unsalted) 64-bit mix is h64, then the 24 bytes the hash does not see."""
    tail = bytes(tail)
    assert len(tail) == 24
    return mix64_inv(h64).to_bytes(8, "little") + tail


def row_home(row, node):
    """df_row_hash."""
    return rs_mix(load8(row) ^ (node << 32) ^ node)


def fnv(seed, name):
    h = C["fnv_offset"] ^ seed
    for b in bytes(name):
        h = (h ^ b) * C["fnv_prime"] & M64
    return h


def name_home(seed, name):
    """wk_key_hash."""
    return rs_mix(fnv(seed, name))


def df_seed(parent, side):
    return (parent * C["df_seed_mul"] & M64) ^ side


def pm_seed(item):
    return item * C["pm_seed_mul"] & M64


# ------------------------------------------------------------------ names with chosen homes
ALPHABET = b"abcdefghijklmnopqrstuvwxyz0123456789"
NAME_DIGITS = 6                      # a candidate: the stem and six letters of ALPHABET
MAX_CANDIDATES = 1 << 27
_A = len(ALPHABET)
_LOW = np.array([[ALPHABET[(i // _A ** k) % _A] for i in range(_A ** 3)] for k in (2, 1, 0)], dtype=np.uint64)


def _mix_np(h):
    s = np.uint64(SHIFT)
    h = h ^ (h >> s)
    h = h * np.uint64(MUL)
    return (h ^ (h >> s)) & np.uint64(M32)


def names_with_home(seed, cap, homes, count, taken=(), stem=b""):
    """`count` names stem + six letters, in the order of the search, whose home at capacity `cap` lies in
    `homes` and that are not in `taken`.  seed and homes may be tuples of equal length: the name's home under
    every seed lies in that seed's set (one name that collides on both sides of a diff).  The search is
    bounded: after MAX_CANDIDATES names it raises."""
    seeds = tuple(seed) if isinstance(seed, (tuple, list)) else (seed,)
    sets = tuple(homes) if isinstance(seed, (tuple, list)) else (homes,)
    assert len(seeds) == len(sets) and cap & (cap - 1) == 0
    want = [np.array(sorted(s), dtype=np.uint64) for s in sets]
    prime, mask = np.uint64(C["fnv_prime"]), np.uint64(cap - 1)
    out, taken, block = [], set(taken), _A ** 3
    for hi in range(0, MAX_CANDIDATES, block):
        head = bytes(stem) + bytes(ALPHABET[(hi // block // _A ** k) % _A] for k in (2, 1, 0))
        ok = np.ones(block, dtype=bool)
        for s, w in zip(seeds, want):
            h = np.full(block, fnv(s, head), dtype=np.uint64)
            for k in range(3):
                h = (h ^ _LOW[k]) * prime
            ok &= np.isin(_mix_np(h) & mask, w)
        for i in np.flatnonzero(ok):
            name = head + bytes(int(_LOW[k][i]) for k in range(3))
            if name not in taken:
                taken.add(name)
                out.append(name)
                if len(out) == count:
                    return out
    raise RuntimeError("table_plant: no %d names with homes %r at capacity %d among %d candidates"
                       % (count, sets, cap, MAX_CANDIDATES))


def name_with_home(seed, cap, homes, taken=(), stem=b""):
    return names_with_home(seed, cap, homes, 1, taken, stem)[0]


# ------------------------------------------------------------------ the model
MUTANTS = ("no_wrap", "home_only", "eq8", "len_only", "no_salt", "first_wins")


class Table:
    """One table: linear probing from a record's home, an equal key keeping the lowest rank.

    A key is (salt, bytes, is_name): the salt is what the device compares beside the bytes (a packfile
    position; parent record and side; an item; a node).  A record is (home hash, key, rank); the slot
    keeps the record of the lowest rank among those of its key (rs_insert: the lowest index, by atomicMin
    on the slot; the joins: the lowest (position, node), in best[]).  The device's lanes claim in any
    order; the model's order is `reverse`: False ascending, True descending.

    The mutants, one way each a kernel could be wrong without faulting:
      no_wrap     the probe ends at the table's last slot
      home_only   find gives up after the home slot
      eq8         the byte compare of a hash, id or row reads the first 8 bytes
      len_only    the name compare reads the lengths
      no_salt     the salt (position, side, item, node) is left out of the compare
      first_wins  the first claimant of a key answers; shown with the claims in descending order
    """

    def __init__(self, cap, mutant=None, reverse=False):
        assert mutant is None or mutant in MUTANTS
        self.cap, self.mutant = cap, mutant
        self.reverse = reverse or mutant == "first_wins"
        self.slots = [None] * cap
        self.longest = 0              # the longest probe, in slots looked at
        self.crossed = False          # a probe went from the last slot to slot 0
        self.lost = 0                 # records that found no place (no_wrap only)

    def eq(self, a, b):
        if self.mutant != "no_salt" and a[0] != b[0]:
            return False
        if a[2]:
            return len(a[1]) == len(b[1]) if self.mutant == "len_only" else a[1] == b[1]
        return a[1][:8] == b[1][:8] if self.mutant == "eq8" else a[1] == b[1]

    def _walk(self, h):
        home = h & (self.cap - 1)
        for probe in range(self.cap):
            if self.mutant == "no_wrap" and home + probe >= self.cap:
                return
            if probe and (home + probe) & (self.cap - 1) == 0:
                self.crossed = True
            self.longest = max(self.longest, probe + 1)
            yield (home + probe) & (self.cap - 1)

    def build(self, records):
        """records: [(hash, key, rank)]; every one is inserted."""
        for h, key, rank in (reversed(records) if self.reverse else records):
            for s in self._walk(h):
                cur = self.slots[s]
                if cur is None:
                    self.slots[s] = (key, rank)
                    break
                if self.eq(cur[0], key):
                    if self.mutant != "first_wins":
                        self.slots[s] = (cur[0], min(cur[1], rank))
                    break
            else:
                self.lost += 1
        return self

    def find(self, h, key):
        """-> the rank that answers for the key, or None."""
        for s in self._walk(h):
            cur = self.slots[s]
            if cur is None:
                return None
            if self.eq(cur[0], key):
                return cur[1]
            if self.mutant == "home_only":
                return None
        return None

    # -- structure
    def occupied(self):
        return {s for s, v in enumerate(self.slots) if v is not None}

    def longest_run(self):
        """The longest stretch of occupied slots, the table taken as a ring."""
        occ = self.occupied()
        if len(occ) == self.cap:
            return self.cap
        best = 0
        for s in occ:
            if (s - 1) % self.cap not in occ:
                n = 0
                while (s + n) % self.cap in occ:
                    n += 1
                best = max(best, n)
        return best

    def wraps(self):
        """A run crosses the table's end."""
        occ = self.occupied()
        return self.cap - 1 in occ and 0 in occ


def shape(tables):
    """{table name: dict(cap, keys, run, wraps, longest_probe)} of a model's tables."""
    return {k: dict(cap=t.cap, keys=len(t.occupied()), run=t.longest_run(), wraps=t.wraps(), longest_probe=t.longest)
            for k, t in tables.items()}


# ------------------------------------------------------------------ stores
PRK = bytes.fromhex("a7" * 32)
KIND_FILE, KIND_DIR = 0, 1
OK, ENOTFOUND, EMISMATCH, ENOPACKFILE = 0, 16, 17, 18
ADDED, REMOVED, MODIFIED, TYPE_CHANGED = 1, 2, 3, 4
PM_NEW, PM_UNCHANGED, PM_CHANGED = 0, 1, 2


def _tail(seed, k=0):
    t = bytearray(np.random.default_rng(seed).integers(0, 256, 24, dtype=np.uint8).tobytes())
    t[k % 24] ^= 1 + k // 24
    return bytes(t)


def builder(seed):
    import restore_store
    return restore_store.Builder(prk=PRK, seed=seed)


def finish(b, sizes, ids=None):
    """restore_store.Builder.finish with the packfiles' sizes in blobs, and their ids, chosen
    -> (packs, index, entries [(packfile position, hash)] in entry order)."""
    from oracle import pack_oracle as po
    assert sum(sizes) == len(b.blobs)
    if ids is None:
        ids = [bytes(b.rng.integers(0, 256, 12, dtype=np.uint8)) for _ in sizes]
    packs, index, entries, f = [], [], [], 0
    for p, n in enumerate(sizes):
        packs.append((ids[p], po.serialize_packfile(b.prk, ids[p], b.blobs[f:f + n])))
        index += [(blob[0], ids[p]) for blob in b.blobs[f:f + n]]
        entries += [(p, blob[0]) for blob in b.blobs[f:f + n]]
        f += n
    return packs, index, entries


def _chunk(b, h, k):
    return b.add(struct.pack("<I", k), blob_hash=h, again=True)


# ------------------------------------------------------------------ the locator's cases
# -> dict(packs, index, entries, queries [hash], want [(status, entry index or None)], wraps {table: bool})

def _locate_case(packs, index, entries, queries, want, **facts):
    assert len(queries) == len(want)
    return dict(kind="locate", packs=packs, index=index, entries=entries, queries=queries, want=want, facts=facts)


def loc_wrap():
    """24 items with homes in the last two slots of the 64-slot item table; one packfile, so the entry
    table (salt 0) has the same homes.  Absent probes: home before the run, inside it, and slot 0."""
    b = builder(11)
    hs = [digest((0x1000 + i) << 32 | (i << 6 | 62 + i % 2), _tail(11, i)) for i in range(24)]
    for k, h in enumerate(hs):
        _chunk(b, h, k)
    packs, index, entries = finish(b, [24])
    absent = [digest(0x2000 << 32 | (1 << 6 | 61), _tail(12)), digest(0x2001 << 32 | (2 << 6 | 63), _tail(13)),
              digest(0x2002 << 32 | (3 << 6 | 0), _tail(14))]
    return _locate_case(packs, index, entries, hs + absent, [(OK, i) for i in range(24)] + [(ENOTFOUND, None)] * 3,
                        wraps=("items", "entries"))


def loc_same_eight():
    """8 hashes that share their first 8 bytes (tails differing in their first, middle and last bytes),
    among ordinary ones, and an absent sibling."""
    b = builder(12)
    rng = np.random.default_rng(12)
    head = digest(0x3000 << 32 | 5, bytes(24))[:8]
    tails = [_tail(15, k) for k in (0, 1, 11, 12, 22, 23)] + [_tail(15, 23 + 24), _tail(15, 24)]
    plain = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(6)]
    hs = plain[:3] + [head + t for t in tails] + plain[3:]
    for k, h in enumerate(hs):
        _chunk(b, h, k)
    packs, index, entries = finish(b, [len(hs)])
    absent = [head + _tail(15, 23 + 48)]
    return _locate_case(packs, index, entries, hs + absent, [(OK, i) for i in range(len(hs))] + [(ENOTFOUND, None)])


SALTED_POS = (0, 6)


def _salted_key(home, cap, n, pos=SALTED_POS):
    """n 8-byte heads whose home at `cap` is `home` under both packfile positions of `pos`.  The salt
    enters above bit 32 and reaches the home through the xor-shifts only: at 16 slots a search finds no
    head that has one home under position 0 and under a position below 6, and plenty for 0 and 6, so the
    case has seven packfiles.  Bounded: it raises after 2^16 heads."""
    out = []
    for hi in range(1 << 16):
        k = key8(home, pos[0], hi)
        if key_home(k, pos[1]) & (cap - 1) == home & (cap - 1):
            out.append(k)
            if len(out) == n:
                return out
    raise RuntimeError("table_plant: no %d keys of home %d under positions %r among 2^16" % (n, home, pos))


def loc_salted():
    """Seven packfiles: [h, g], [f0], [f1], [f2], [f3], [f4], [h].  h is in packfiles 0 and 6, and (0, h),
    (6, h), (0, g) and the absent (6, g) all have the entry table's home 9 (16 slots).  The index names
    packfile 6 for h and for g: h's entry is the one of packfile 6 (entry 7), g is EMISMATCH."""
    b = builder(13)
    rng = np.random.default_rng(13)
    kh, kg = _salted_key(9, 16, 2)
    h, g = kh + _tail(16), kg + _tail(17)
    f = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(5)]
    for k, x in enumerate([h, g] + f + [h]):
        _chunk(b, x, k)
    packs, index, entries = finish(b, [2, 1, 1, 1, 1, 1, 1])
    ids = [p[0] for p in packs]
    index = [(f[0], ids[1]), (h, ids[6]), (f[1], ids[2]), (g, ids[6]), (f[2], ids[3]), (f[3], ids[4]), (f[4], ids[5])]
    return _locate_case(packs, index, entries, [h, g] + f, [(OK, 7), (EMISMATCH, None)] + [(OK, 2 + i) for i in range(5)])


DUP_N, DUP_FIRST = 70, 13


def loc_duplicates_behind_a_run():
    """One header: 3 fillers, 10 keys of home 200 (256 slots), then the hash d, of the same home, 70 times
    (entries 13 .. 82: two waves' worth of lanes), then 3 fillers.  d answers with entry 13."""
    b = builder(14)
    rng = np.random.default_rng(14)
    f = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(6)]
    run = [digest((0x4000 + i) << 32 | ((i + 1) << 8 | 200), _tail(18, i)) for i in range(10)]
    d = digest(0x4100 << 32 | (77 << 8 | 200), _tail(19))
    blobs = f[:3] + run + [d] * DUP_N + f[3:]
    for k, x in enumerate(blobs):
        _chunk(b, x, k)
    packs, index, entries = finish(b, [len(blobs)])
    seen, uniq = set(), []
    for x, pid in index:               # one item per hash
        if x not in seen:
            seen.add(x)
            uniq.append((x, pid))
    queries = [d] + run + f
    want = [(OK, DUP_FIRST)] + [(OK, 3 + i) for i in range(10)] + [(OK, 0), (OK, 1), (OK, 2)] + \
        [(OK, DUP_FIRST + DUP_N + i) for i in range(3)]
    return _locate_case(packs, uniq, entries, queries, want)


def loc_ids():
    """6 packfiles whose 12-byte ids share their first 8 bytes, with their home in the last slot of the
    16-slot id table; 3 blobs each.  Every item resolves to its own packfile's position."""
    b = builder(15)
    rng = np.random.default_rng(15)
    head = key8(0x5A5A5A0F | 0xF)
    ids = [head + bytes([0, 0, 0, k]) for k in range(3)] + [head + bytes([k, 0, 0, 0]) for k in range(1, 4)]
    hs = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(18)]
    for k, x in enumerate(hs):
        _chunk(b, x, k)
    packs, index, entries = finish(b, [3] * 6, ids)
    order = rng.permutation(18)
    index = [index[i] for i in order]
    absent_id = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    index.append((absent_id, head + bytes([9, 9, 9, 9])))     # the same 8 bytes, in no packfile
    return _locate_case(packs, index, entries, hs + [absent_id], [(OK, i) for i in range(18)] + [(ENOPACKFILE, None)],
                        wraps=("ids",))


CROWD = 300


def loc_crowd():
    """300 items of one home, slot 924 of 1,024: a run of 300 slots across the table's end, in the item
    table and in the entry table, built by two workgroups.  Then 300 absent keys of the same home."""
    b = builder(16)
    hs = [digest((0x6000 + i) << 32 | ((i + 1) << 10 | 924), _tail(20, i)) for i in range(CROWD)]
    for k, x in enumerate(hs):
        _chunk(b, x, k)
    packs, index, entries = finish(b, [CROWD])
    absent = [digest((0x7000 + i) << 32 | ((i + 1) << 10 | 924), _tail(21, i)) for i in range(CROWD)]
    return _locate_case(packs, index, entries, hs + absent, [(OK, i) for i in range(CROWD)] + [(ENOTFOUND, None)] * CROWD,
                        wraps=("items", "entries"))


def model_locate(case, mutant=None):
    """The three tables and the queries through the model -> (answers [(status, entry)], {name: Table})."""
    ids = [p[0] for p in case["packs"]]
    n_pf, n_i, n_e = len(ids), len(case["index"]), len(case["entries"])
    t_ids = Table(pow2_cap(n_pf), mutant).build([(key_home(i), (0, i, False), k) for k, i in enumerate(ids)])
    item_pos = [t_ids.find(key_home(pid), (0, pid, False)) for _, pid in case["index"]]
    t_items = Table(pow2_cap(n_i), mutant).build([(key_home(h), (0, h, False), k) for k, (h, _) in enumerate(case["index"])])
    t_ent = Table(pow2_cap(n_e), mutant).build([(key_home(h, p), (p, h, False), k) for k, (p, h) in enumerate(case["entries"])])
    out = []
    for q in case["queries"]:
        item = t_items.find(key_home(q), (0, q, False))
        if item is None:
            out.append((ENOTFOUND, None))
        elif item_pos[item] is None:
            out.append((ENOPACKFILE, None))
        else:
            e = t_ent.find(key_home(q, item_pos[item]), (item_pos[item], q, False))
            out.append((EMISMATCH, None) if e is None else (OK, e))
    return out, dict(ids=t_ids, items=t_items, entries=t_ent)


def reference_locate(case):
    """The same queries through restore_ref.Store and prune_ref.Locator."""
    import prune_ref
    import restore_ref
    store = restore_ref.Store(PRK, case["packs"], case["index"])
    locate = prune_ref.Locator(store, prune_ref.headers_of(PRK, case["packs"]))
    return [locate(q) for q in case["queries"]]


# ------------------------------------------------------------------ the diff walk's cases
# -> dict(packs, index, root_a, root_b, level1 [(side, pos, name, kind, hash)],
#         want Counter((name, change, A hash, B hash)) of the records below the root, ...)
# A child is a File without chunks (or an empty Dir); its metadata makes its hash.

def _kid(b, name, kind=KIND_FILE, mtime=1, children=(), blob_hash=None):
    from oracle import oracle
    data = oracle.tree_serialize(kind, name, 7 if kind == KIND_FILE else None, mtime, None, b"".join(children))
    return b.add(data, 1, blob_hash=blob_hash)          # pack_oracle.KIND_TREE


def _diff_case(b, kids_a, kids_b, **more):
    """kids: [(name, kind, mtime)] per side, in position order -> the case, the expectation by
    diff_ref's rules 2 and 4 written out over names: the lowest position of a name represents it."""
    sides, level1 = [], []
    for side, kids in enumerate((kids_a, kids_b)):
        hs = [_kid(b, n, k, m) for n, k, m in kids]
        sides.append(hs)
    for side, kids in enumerate((kids_a, kids_b)):
        other = set(sides[side ^ 1])
        level1 += [(side, pos, n, k, sides[side][pos]) for pos, (n, k, m) in enumerate(kids) if sides[side][pos] not in other]
    from oracle import oracle
    roots = [b.add(oracle.tree_serialize(KIND_DIR, "", None, 100 + side, None, b"".join(sides[side])), 1) for side in (0, 1)]
    packs, index, entries = finish(b, [len(b.blobs)])
    reps = [{}, {}]
    for side, pos, n, k, h in level1:
        reps[side].setdefault(n, (pos, k, h))             # level1 is in position order
    want = Counter()
    for side, pos, n, k, h in level1:
        mine, theirs = reps[side][n], reps[side ^ 1].get(n)
        if mine[0] != pos or theirs is None:
            want[(n, ADDED if side else REMOVED, ZERO if side else h, h if side else ZERO)] += 1
        elif side == 0:
            want[(n, MODIFIED if k == theirs[1] else TYPE_CHANGED, h, theirs[2])] += 1
    return dict(kind="diff", packs=packs, index=index, entries=entries, root_a=roots[0], root_b=roots[1], level1=level1,
                rows=[(0, sides[0]), (1, sides[1])], want=want, facts=more)


END3 = {61, 62, 63}


def diff_names_wrap():
    """15 children a side, none shared: 30 nodes on level 1, a 64-slot table.  8 names are on both sides
    (metadata differs; one pair File against Dir) with both sides' homes in the last three slots, 7 are
    A's alone and 7 B's alone, theirs there too."""
    sa, sb = df_seed(0, 0), df_seed(0, 1)
    both = names_with_home((sa, sb), 64, (END3, END3), 8)
    only_a = names_with_home(sa, 64, END3, 7, both)
    only_b = names_with_home(sb, 64, END3, 7, both + only_a)
    ka = [(n, KIND_FILE, 10 + i) for i, n in enumerate(both)] + [(n, KIND_FILE, 30 + i) for i, n in enumerate(only_a)]
    kb = [(n, KIND_FILE, 50 + i) for i, n in enumerate(only_b)] + \
         [(n, KIND_DIR if i == 3 else KIND_FILE, 70 + i) for i, n in enumerate(both)]
    ka = [ka[i] for i in np.random.default_rng(21).permutation(15)]
    return _diff_case(builder(21), ka, kb, wraps=("names",), n_level1=30)


def diff_names_crowd():
    """300 children a side, all 600 with their home in slot 1,848 of 2,048: one run of 600 slots across
    the table's end.  4 names are on both sides (their A home and their B home are that slot)."""
    sa, sb = df_seed(0, 0), df_seed(0, 1)
    home = {1848}
    both = names_with_home((sa, sb), 2048, (home, home), 4)
    only_a = names_with_home(sa, 2048, home, CROWD - 4, both)
    only_b = names_with_home(sb, 2048, home, CROWD - 4, both + only_a)
    ka = [(n, KIND_FILE, 1000 + i) for i, n in enumerate(only_a[:150] + both + only_a[150:])]
    kb = [(n, KIND_FILE, 2000 + i) for i, n in enumerate(both[::-1] + only_b)]
    return _diff_case(builder(22), ka, kb, wraps=("names",), n_level1=600)


def diff_dup_names():
    """Side A: 7 names of home 40 (64 slots), and the name N of the same home three times, at positions
    3, 7 and 9.  Side B has N once: it pairs with A's position 3; positions 7 and 9 are REMOVED."""
    sa, sb = df_seed(0, 0), df_seed(0, 1)
    run = names_with_home(sa, 64, {40}, 8)
    n, run = run[0], run[1:]
    ka = [(x, KIND_FILE, 10 + i) for i, x in enumerate(run)]
    for pos, m in ((3, 20), (7, 21), (9, 22)):
        ka.insert(pos, (n, KIND_FILE, m))
    assert [i for i, k in enumerate(ka) if k[0] == n] == [3, 7, 9]
    kb = [(run[1], KIND_FILE, 40), (n, KIND_FILE, 41), (name_with_home(sb, 64, {40}, run + [n]), KIND_FILE, 42)]
    return _diff_case(builder(23), ka, kb, dup=(n, 3), n_level1=13)


def near_names(seed, cap):
    """Names that share a home under `seed` on purpose: the empty name and a name of its home; a name and
    its extension by one letter; two names of one length that differ in their last byte."""
    mask = cap - 1
    home = lambda n: name_home(seed, n) & mask
    e = name_with_home(seed, cap, {home(b"")})
    ext = last = None
    for p in names_with_home(seed, cap, set(range(cap)), 400, stem=b"p"):
        more = [p + bytes([c]) for c in ALPHABET if home(p + bytes([c])) == home(p)]
        if more and ext is None:
            ext = (p, more[0])
        same = [p[:-1] + bytes([c]) for c in ALPHABET if c != p[-1] and home(p[:-1] + bytes([c])) == home(p)]
        if same and last is None and (ext is None or p != ext[0]):
            last = (p, same[0])
    if ext is None or last is None:
        raise RuntimeError("table_plant: no colliding name pairs at capacity %d among 400 names" % cap)
    return [(b"", e), ext, last]


def diff_near_names():
    """Side A holds the three colliding pairs; side B holds the empty name and the second of the other
    two pairs (metadata differs): each of B's probes into A's side starts in the home its pair shares."""
    sa = df_seed(0, 0)
    pairs = near_names(sa, 64)
    ka = [(n, KIND_FILE, 10 + i) for i, n in enumerate(x for pair in pairs for x in pair)]
    kb = [(pairs[0][0], KIND_FILE, 30), (pairs[1][1], KIND_FILE, 31), (pairs[2][1], KIND_FILE, 32)]
    return _diff_case(builder(24), ka, kb, pairs=pairs, n_level1=9)


ROWS_N = 40


def diff_rows_same_eight():
    """A File "f" on both sides, 40 chunk rows on side A that all share their first 8 bytes; side B keeps
    the first 10 and the last 10 and has 20 new rows of the same 8 bytes between them."""
    from oracle import oracle
    b = builder(25)
    head = digest(0x8000 << 32 | 0x1234, bytes(24))[:8]
    ra = [head + _tail(22, k) for k in range(ROWS_N)]
    new = [head + _tail(22, 100 + k) for k in range(20)]
    rb = ra[:10] + new + ra[30:]
    fa = b.add(oracle.tree_serialize(KIND_FILE, "f", 4000, 5, None, b"".join(ra)), 1)
    fb = b.add(oracle.tree_serialize(KIND_FILE, "f", 4000, 6, None, b"".join(rb)), 1)
    same = _kid(b, b"same", KIND_FILE, 9)
    roots = [b.add(oracle.tree_serialize(KIND_DIR, "", None, 100 + s, None, same + f), 1) for s, f in enumerate((fa, fb))]
    packs, index, entries = finish(b, [len(b.blobs)])
    return dict(kind="diff", packs=packs, index=index, entries=entries, root_a=roots[0], root_b=roots[1],
                level1=[(0, 1, b"f", KIND_FILE, fa), (1, 1, b"f", KIND_FILE, fb)], want=Counter({(b"f", MODIFIED, fa, fb): 1}),
                rows=[(0, ra), (1, rb)], row_nodes=True, file_want=dict(n_new=20, common_prefix=10, common_suffix=10, n_a=40, n_b=40),
                facts=dict(n_level1=2))


ROOT_END, ROOT_START = {62, 63}, {0, 1}


def _root_row(i, homes):
    """A 32-byte row whose home in a 64-slot table lies, for every node of homes {node: slots}, in that
    node's slots.  Bounded: it raises after 4,096 candidates."""
    for hi in range(i << 12, (i + 1) << 12):
        h = digest(hi << 32 | (i << 6 | 62 + i % 2), _tail(23, i))
        h = (load8(h) ^ (1 << 32 | 1)).to_bytes(8, "little") + h[8:] if 0 not in homes else h   # the low bits are node 1's
        if all(row_home(h, n) & 63 in slots for n, slots in homes.items()):
            return h
    raise RuntimeError("table_plant: no row with homes %r among 4,096" % (homes,))


def diff_root_rows_wrap():
    """The roots are nodes 0 and 1 of level 0 (the host writes them), so their rows' homes are known.  12
    children a root, tree blobs stored under planted hashes.  6 are A's alone (home in the last two of 64
    slots for node 0), 6 are B's alone (the same for node 1), 6 are both roots': their home for node 0
    lies in the last two slots and their home for node 1 in the first two (the node mix flips bits 0 and
    32 of the key, and no key has both homes in the last four slots).  24 rows in one run across the
    table's end; the 12 that are one root's alone are the records of level 1."""
    b = builder(26)
    shared = [_root_row(i, {0: ROOT_END, 1: ROOT_START}) for i in range(6)]
    only = [[_root_row(10 + 10 * side + i, {side: ROOT_END}) for i in range(6)] for side in (0, 1)]
    for i, h in enumerate(shared):
        _kid(b, b"s%d" % i, KIND_FILE, 10 + i, blob_hash=h)
    for side in (0, 1):
        for i, h in enumerate(only[side]):
            _kid(b, b"%s%d" % (b"ab"[side:side + 1], i), KIND_FILE, 20 + i, blob_hash=h)
    from oracle import oracle
    rows = [[x for pair in zip(shared, only[side]) for x in (pair if side == 0 else pair[::-1])] for side in (0, 1)]
    roots = [b.add(oracle.tree_serialize(KIND_DIR, "", None, 100 + side, None, b"".join(rows[side])), 1) for side in (0, 1)]
    packs, index, entries = finish(b, [len(b.blobs)])
    level1 = [(side, rows[side].index(h), b"%s%d" % (b"ab"[side:side + 1], i), KIND_FILE, h)
              for side in (0, 1) for i, h in enumerate(only[side])]
    want = Counter((n, ADDED if side else REMOVED, ZERO if side else h, h if side else ZERO) for side, _, n, _, h in level1)
    return dict(kind="diff", packs=packs, index=index, entries=entries, root_a=roots[0], root_b=roots[1], level1=level1,
                want=want, rows=[(0, rows[0]), (1, rows[1])], root_rows=True, facts=dict(wraps=("rows",), n_level1=12))


def model_diff(case, mutant=None):
    """The rows of the case's two lists and the names of level 1 through the model ->
    (answers: dict(unmatched {(side, hash)}, n_new, records Counter as case["want"]), {name: Table})."""
    (na, ra), (nb, rb) = case["rows"]
    t_rows = Table(df_table_cap(len(ra) + len(rb)), mutant)
    flat = [(n, r) for n, rows in ((na, ra), (nb, rb)) for r in rows]
    t_rows.build([(row_home(r, n), (n, r, False), k) for k, (n, r) in enumerate(flat)])
    found = lambda row, node: t_rows.find(row_home(row, node), (node, row, False)) is not None
    unmatched = {(0, r) for r in ra if not found(r, nb)} | {(1, r) for r in rb if not found(r, na)}
    n_new = sum(1 for r in rb if not found(r, na))
    # the join of level 1: key (parent record 0, side, name), rank (position << 32 | node)
    nodes = case["level1"]
    t_names = Table(df_table_cap(len(nodes)), mutant)
    key = lambda side, name: (side, name, True)
    t_names.build([(name_home(df_seed(0, s), n), key(s, n), pos << 32 | i) for i, (s, pos, n, k, h) in enumerate(nodes)])
    records = Counter()
    for i, (s, pos, n, k, h) in enumerate(nodes):
        one = (n, ADDED if s else REMOVED, ZERO if s else h, h if s else ZERO)
        if t_names.find(name_home(df_seed(0, s), n), key(s, n)) != pos << 32 | i:
            records[one] += 1                                   # not the representative of its name
            continue
        p = t_names.find(name_home(df_seed(0, s ^ 1), n), key(s ^ 1, n))
        if p is None:
            records[one] += 1
        elif s == 0:
            o = nodes[p & M32]
            records[(n, MODIFIED if k == o[3] else TYPE_CHANGED, h, o[4])] += 1
    return dict(unmatched=unmatched, n_new=n_new, records=records), dict(rows=t_rows, names=t_names)


def reference_diff(case):
    """diff_ref.diff -> (the records below the root as case["want"], the root record or the File's, all records, errors)."""
    import diff_ref
    import prune_ref
    import restore_ref
    store = restore_ref.Store(PRK, case["packs"], case["index"])
    return diff_ref.diff(store, prune_ref.headers_of(PRK, case["packs"]), case["root_a"], case["root_b"])


def level1_records(records):
    """Records in diff_ref's shape -> Counter((name, change, A hash, B hash)) of those whose parent is record 0."""
    return Counter((r["name"], r["change"], r["a"][0], r["b"][0]) for r in records if r["parent"] == 0)


# ------------------------------------------------------------------ the parent match's cases
# -> dict(packs, index, root, scan (parent_ref's), kids [(name, hash)] in position order,
#         want [hash or None per scan child])

def _pm_case(b, kids, asked, **facts):
    """kids: [(name, mtime)] the parent Dir's children (Files of size 7); asked: [(name, mtime)] the scan's.
    want: the hash of the lowest position of the name, or None."""
    from oracle import oracle
    hs = [_kid(b, n, KIND_FILE, m) for n, m in kids]
    root = b.add(oracle.tree_serialize(KIND_DIR, "", None, 100, None, b"".join(hs)), 1)
    packs, index, entries = finish(b, [len(b.blobs)])
    first = {}
    for (n, m), h in zip(kids, hs):
        first.setdefault(n, (h, m))
    scan = [dict(kind=KIND_DIR, flags=2, size=0, mtime=100, ctime=0, child_first=1, n_children=len(asked), name=b"")]
    scan += [dict(kind=KIND_FILE, flags=3, size=7, mtime=m, ctime=0, child_first=0, n_children=0, name=n) for n, m in asked]
    want = [first[n][0] if n in first else None for n, m in asked]
    status = [PM_NEW if n not in first else (PM_UNCHANGED if first[n][1] == m else PM_CHANGED) for n, m in asked]
    return dict(kind="parent", packs=packs, index=index, entries=entries, root=root, scan=scan,
                kids=[(n, h) for (n, m), h in zip(kids, hs)], want=want, status=status, facts=facts)


def pm_wrap():
    """12 parent children with homes in the last two of 64 slots; the scan asks for them and for 6 names
    that are absent and have the same homes: NEW, after the whole run across the table's end."""
    s = pm_seed(0)
    names = names_with_home(s, 64, {62, 63}, 18)
    kids = [(n, 10 + i) for i, n in enumerate(names[:12])]
    asked = [kids[i] for i in np.random.default_rng(31).permutation(12)] + [(n, 50) for n in names[12:]]
    return _pm_case(builder(31), kids, asked, wraps=("names",))


def pm_dup():
    """8 parent children of home 30 (64 slots); the name N is at positions 2, 5 and 7.  Position 2 answers."""
    s = pm_seed(0)
    names = names_with_home(s, 64, {30}, 6)
    n = names[0]
    kids = [(x, 10 + i) for i, x in enumerate(names[1:])]
    for pos, m in ((2, 20), (5, 21), (7, 22)):
        kids.insert(pos, (n, m))
    asked = [(n, 20), (names[1], 10), (names[5], 99)]
    return _pm_case(builder(32), kids, asked, dup=(n, 2))


def pm_crowd():
    """300 parent children of one home, slot 924 of 1,024, and 20 absent names of that home."""
    s = pm_seed(0)
    names = names_with_home(s, 1024, {924}, CROWD + 20)
    kids = [(n, 1000 + i) for i, n in enumerate(names[:CROWD])]
    asked = kids[::-1] + [(n, 5) for n in names[CROWD:]]
    return _pm_case(builder(33), kids, asked, wraps=("names",))


def model_parent(case, mutant=None):
    """The (item 0, name) table over the parent's children and the scan's probes -> ([hash or None], tables)."""
    kids = case["kids"]
    t = Table(pm_table_cap(len(kids)), mutant)
    t.build([(name_home(pm_seed(0), n), (0, n, True), pos << 32 | pos) for pos, (n, h) in enumerate(kids)])
    out = []
    for sn in case["scan"][1:]:
        r = t.find(name_home(pm_seed(0), sn["name"]), (0, sn["name"], True))
        out.append(None if r is None else kids[r & M32][1])
    return out, dict(names=t)


def reference_parent(case):
    import parent_ref
    import prune_ref
    import restore_ref
    store = restore_ref.Store(PRK, case["packs"], case["index"])
    return parent_ref.match(store, prune_ref.headers_of(PRK, case["packs"]), case["root"], case["scan"])


# ------------------------------------------------------------------ all of them
CASES = {"wrap": loc_wrap, "same_eight": loc_same_eight, "salted": loc_salted,
         "duplicates_behind_a_run": loc_duplicates_behind_a_run, "ids": loc_ids, "crowd": loc_crowd,
         "names_wrap": diff_names_wrap, "names_crowd": diff_names_crowd, "dup_names": diff_dup_names,
         "near_names": diff_near_names, "rows_same_eight": diff_rows_same_eight, "root_rows_wrap": diff_root_rows_wrap,
         "pm_wrap": pm_wrap, "pm_dup": pm_dup, "pm_crowd": pm_crowd}
LOCATE = tuple(k for k, f in CASES.items() if f.__name__.startswith("loc_"))
DIFF = tuple(k for k, f in CASES.items() if f.__name__.startswith("diff_"))
PARENT = tuple(k for k, f in CASES.items() if f.__name__.startswith("pm_"))


@functools.lru_cache(maxsize=None)
def case(name):
    """A case, built once per process; nobody changes it."""
    return CASES[name]()


def model(name, mutant=None):
    """(answers, tables) of a case through the model."""
    c = case(name)
    return {"locate": model_locate, "diff": model_diff, "parent": model_parent}[c["kind"]](c, mutant)


def constructed(name):
    """The case's answers by construction, in the shape of model()'s."""
    c = case(name)
    if c["kind"] == "locate":
        return c["want"]
    if c["kind"] == "parent":
        return c["want"]
    (na, ra), (nb, rb) = c["rows"]
    sa, sb = set(ra), set(rb)
    return dict(unmatched={(0, r) for r in ra if r not in sb} | {(1, r) for r in rb if r not in sa},
                n_new=sum(1 for r in rb if r not in sa), records=c["want"])
