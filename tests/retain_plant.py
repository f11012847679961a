"""Planted masks, root words and batches for retain's drop and mark (bw_retain_drop, bw_retain_mark,
backuwup_amd/csrc/bw_retain.hip).  Pure Python + numpy; a helper, not a test.

The drop takes the caller's masks, so it needs no tree: a FLAT store is unreferenced file chunks whose
packfiles hold a chosen number of entries each (where a packfile begins inside a wave is the geometry), the
masks over it are planted (empty, full, a lone last bit, bits in the first and the last word, orphans at
chosen lanes) and the drop sets come in families that make the host's batch loop go round: bits_of_q
(every set distinct, past RT_DROP_BATCH_SETS sets), cycle (8 distinct sets over a store of more than 4096
entries, where RT_DROP_BATCH_BYTES binds first) and wide (whole words of 4096 roots).  The expected result
is tests/retain_ref.py's drop, a few lines of integer arithmetic; reference_drop_np() restates it over
numpy for the family of 65,537 sets and tests/test_retain_plant.py holds the two equal.

model_drop() is k_rt_drop and the host loop around it with their geometry: waves of 64 lanes in
workgroups of 256, a wave inside one packfile adding its sums once and a wave across packfiles lane by
lane, batches of `per` sets with the sums cleared in between.  Answers are never taken from it: its
one-line mutants (DROP_MUTANTS) show that the cases can fail.  model_mark() does the same for k_rt_seed,
k_rt_propagate and k_rt_stats over retain_ref.walk's edges (MARK_MUTANTS), on two tree stores:
staircase(k), where root B's bit needs k + 1 productive sweeps, and cycled_roots(n), ten distinct small
roots repeated to n (up to 4096) with the once-only ones in the first and the last word.

Nothing here holds a literal of the kernels' constants: the batch bounds, the root limit, the workgroup,
the wave and the nonce size are read out of the sources by read_constants(), and a pattern that no longer
matches raises.  tests/test_gpu_retain_planted.py runs the cases on the device.
"""
import functools
import os
import re
from collections import Counter

import numpy as np

M64 = (1 << 64) - 1
NONE = M64
ZERO = bytes(32)
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "backuwup_amd", "csrc")
SOURCES = {"bw_retain.h": _CSRC, "bw_retain_host.h": _CSRC, "bw_retain.hip": _CSRC,
           "backuwup_gpu_pack.h": os.path.join(_ROOT, "include")}


# ------------------------------------------------------------------ the kernels' constants, from their sources

def sources():
    out = {}
    for name, where in SOURCES.items():
        with open(os.path.join(where, name)) as f:
            out[name] = f.read()
    return out


def _need(pattern, text, what, count=1):
    found = re.findall(pattern, text)
    if len(found) != count:
        raise RuntimeError("retain_plant: %s no longer matches (%d hits for %r); the planter must be re-derived "
                           "from the source" % (what, len(found), pattern))
    return found


def _body(src, head, name):
    """The text of the function whose signature matches `head`, up to the next line-initial '}'."""
    m = re.search(head, src)
    if not m:
        raise RuntimeError("retain_plant: %s not found; the planter must be re-derived from the source" % name)
    return src[m.end():src.index("\n}", m.end())]


def read_constants(src=None):
    """The constants of the drop and the mark out of the source texts {file name: text} (default: the tree's)."""
    src = sources() if src is None else src
    rh, hh, hip = src["bw_retain.h"], src["bw_retain_host.h"], src["bw_retain.hip"]
    c = {}
    c["batch_sets"] = int(_need(r"constexpr uint64_t RT_DROP_BATCH_SETS = (\d+);", rh, "RT_DROP_BATCH_SETS")[0])
    c["batch_bytes"] = 1 << int(_need(r"constexpr uint64_t RT_DROP_BATCH_BYTES = 1ull << (\d+);", rh, "RT_DROP_BATCH_BYTES")[0])
    c["sums"] = int(_need(r"constexpr uint32_t RT_SUMS = (\d+);", rh, "RT_SUMS")[0])
    c["max_roots"] = int(_need(r"constexpr uint64_t RT_MAX_ROOTS = (\d+);", hh, "RT_MAX_ROOTS")[0])
    _need(r"rt_words\(uint64_t n_roots\) \{ return n_roots \? \(n_roots \+ 63\) / 64 : 1; \}", hh, "rt_words")
    c["nonce"] = int(_need(r"#define BW_BLOB_NONCE_SIZE (\d+)u", src["backuwup_gpu_pack.h"], "BW_BLOB_NONCE_SIZE")[0])
    # the host loop: per, the offsets of a batch, the clear of the sums
    _need(r"per = std::max<uint64_t>\(1, std::min\(\{n_sets, RT_DROP_BATCH_SETS, RT_DROP_BATCH_BYTES / std::max<uint64_t>\(n_e, 1\)\}\)\);",
          hip, "the drop's batch size")
    _need(r"for \(uint64_t q0 = 0; q0 < n_sets; q0 \+= per\) \{", hip, "the drop's batch loop")
    _need(r"hipMemcpyAsync\(d_mask \+ drop_at, drop \+ q0 \* W, 8 \* m \* W,", hip, "a batch's drop sets")
    _need(r"hipMemsetAsync\(d_stat, 0, freed_at \+ 32 \* per, c->stream\)", hip, "the clear of a batch's sums")
    _need(r"hipMemcpyAsync\(live \+ q0 \* n_e, s->rt\[RT_B_LIVE\]\.p, m \* n_e,", hip, "a batch's live rows")
    _need(r"hipMemcpyAsync\(stats \+ q0 \* n_pf, d_stat, 32 \* m \* n_pf,", hip, "a batch's stat rows")
    _need(r"hipMemcpyAsync\(freed \+ q0, d_stat \+ freed_at, 32 \* m,", hip, "a batch's freed records")
    # the kernel: workgroup, wave, the switch between the two accounting shapes
    c["workgroup"] = int(_need(r"__global__ void __launch_bounds__\((\d+)\) k_rt_drop\(", hip, "k_rt_drop's workgroup")[0])
    launch = _need(r"hipLaunchKernelGGL\(k_rt_drop, dim3\(\(uint32_t\)\(\(n_e \+ (\d+)\) / (\d+)\), \(uint32_t\)m\), dim3\((\d+)\)", hip,
                   "k_rt_drop's launch")[0]
    if [int(x) for x in launch] != [c["workgroup"] - 1, c["workgroup"], c["workgroup"]]:
        raise RuntimeError("retain_plant: k_rt_drop is no longer launched in workgroups of its launch bound; the planter "
                           "must be re-derived from the source")
    half = int(_need(r"for \(int d = (\d+); d; d >>= 1\) v \+= __shfl_down", _body(hip, r"uint64_t rt_wave_sum\(uint64_t v\) \{", "rt_wave_sum"),
                     "rt_wave_sum's first step")[0])
    c["wave"] = 2 * half
    drop = _body(hip, r"__global__ void __launch_bounds__\(\d+\) k_rt_drop\(", "k_rt_drop")
    lane0 = _need(r"\(threadIdx\.x & (\d+)\) == 0", drop, "k_rt_drop's lane-0 tests", 2)
    if {int(x) for x in lane0} != {c["wave"] - 1}:
        raise RuntimeError("retain_plant: k_rt_drop's lane-0 tests and rt_wave_sum disagree on the wave; the planter must "
                           "be re-derived from the source")
    _need(r"if \(__all\(!in \|\| p == p0\) && __shfl\(\(int\)in, 0\)\) \{", drop, "the switch between the accounting shapes")
    _need(r"const bool fr = in && any && !lv, kept = in && lv;", drop, "freed and kept")
    _need(r"bytes = BW_BLOB_NONCE_SIZE \+ entries\[e\]\.length;", drop, "an entry's bytes")
    _need(r"if \(live\) live\[q \* n \+ e\] = lv \? 1 : 0;", drop, "the live row's stride")
    _need(r"lv = lv \|\| \(m & ~drop\[q \* W \+ w\]\);", drop, "the drop predicate")
    # the mark
    _need(r"const unsigned long long bit = 1ull << \(i & 63\);", hip, "the seed's bit")
    _need(r"reach\[e \* W \+ \(i >> 6\)\], bit\)", hip, "the seed's word")
    _need(r"const ImEdge ed = edges\[lo \+ i / W\];\n    const uint64_t w = i % W,", hip, "propagate's (edge, word)")
    _need(r"for \(uint64_t w = 0; w < W; w\+\+\) pop \+= __popcll", hip, "the popcount over all words")
    return c


C = read_constants()
BATCH_SETS, BATCH_BYTES, MAX_ROOTS, SUMS = C["batch_sets"], C["batch_bytes"], C["max_roots"], C["sums"]
WORKGROUP, WAVE, NONCE = C["workgroup"], C["wave"], C["nonce"]


def n_words(n_roots):
    return (n_roots + 63) // 64 if n_roots else 1


def per_of(n_sets, n_e):
    """The sets of one batch."""
    return max(1, min(n_sets, BATCH_SETS, BATCH_BYTES // max(n_e, 1)))


def full(n_roots):
    return (1 << n_roots) - 1


def to_words(sets, n_roots):
    """Root sets (Python ints) -> (len, W) u64."""
    W = n_words(n_roots)
    if not len(sets):
        return np.zeros((0, W), dtype=np.uint64)
    return np.frombuffer(b"".join(int(s).to_bytes(8 * W, "little") for s in sets), dtype="<u8").reshape(len(sets), W).copy()


def to_ints(words):
    """(n, W) u64 -> one Python int per row."""
    return [sum(int(x) << (64 * w) for w, x in enumerate(row)) for row in np.asarray(words).tolist()]


def bits_of(s):
    out, r = [], 0
    while s:
        if s & 1:
            out.append(r)
        s >>= 1
        r += 1
    return out


# ------------------------------------------------------------------ flat stores
# group sizes: the entries of each packfile, in order
GEOMETRIES = {
    "lane1": [1, 63, 64, 65, 127, 1, 1, 62, 256, 257, 3],   # first entries at lanes 0 1 0 0 1 0 1 2 0 0 1; 900 entries
    "lane63": [63, 64, 1, 2, 126, 193, 11],                 # first entries at lanes 0 63 63 0 2 0 1; 460 entries
    "ones": [1] * 130,
    "one": [300],
    "bytes_bound": [300] * 14,                              # 4200 entries: RT_DROP_BATCH_BYTES binds before the sets
    "sets_bound": [33, 15],                                 # 48 entries for the family of 65,537 sets
}
WAVE_GEOMETRIES = ("lane1", "lane63", "ones", "one")
SEEDS = {name: 200 + k for k, name in enumerate(GEOMETRIES)}


def first_entries(groups):
    out, f = [], 0
    for g in groups:
        out.append(f)
        f += g
    return out


def first_lanes(groups):
    """The lane of each packfile's first entry, and its workgroup."""
    return [(f % WAVE, f // WORKGROUP) for f in first_entries(groups)]


def finish(b, groups):
    """restore_store.Builder.finish with the packfiles' sizes in blobs chosen -> (packs, index)."""
    from oracle import pack_oracle as po
    assert sum(groups) == len(b.blobs)
    ids = [bytes(b.rng.integers(0, 256, 12, dtype=np.uint8)) for _ in groups]
    packs, index, f = [], [], 0
    for p, n in enumerate(groups):
        packs.append((ids[p], po.serialize_packfile(b.prk, ids[p], b.blobs[f:f + n])))
        index += [(blob[0], ids[p]) for blob in b.blobs[f:f + n]]
        f += n
    return packs, index


def flat_store(groups, seed):
    """Unreferenced file chunks in packfiles of the given sizes, no two packfiles with one byte sum
    -> dict(packs, index, n_entries, groups, hd (prune_ref's headers), pf, length (per entry), slots)."""
    import prune_ref
    import restore_store
    b = restore_store.Builder(seed=seed)
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 200, sum(groups)).tolist()
    seen, f = set(), 0
    for g in groups:                 # one store frame's overhead is the same for every length below 256
        while sum(lens[f:f + g]) in seen:
            lens[f + g - 1] += 1
        seen.add(sum(lens[f:f + g]))
        f += g
    for k, n in enumerate(lens):
        b.add(k.to_bytes(4, "little") + rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    assert len(b.blobs) == sum(groups)
    packs, index = finish(b, groups)
    hd = prune_ref.headers_of(restore_store.PRK, packs)
    ents = prune_ref.flat_entries(hd)
    pf = np.array([e[0] for e in ents], dtype=np.int64)
    length = np.array([e[4] for e in ents], dtype=np.uint64)
    assert pf.tolist() == [p for p, g in enumerate(groups) for _ in range(g)]
    sums = [int(NONCE * g + length[f:f + g].sum()) for f, g in zip(first_entries(groups), groups)]
    if len(set(sums)) != len(sums):
        raise RuntimeError("retain_plant: two packfiles of a flat store have one byte sum")
    return dict(packs=packs, index=index, n_entries=len(ents), groups=list(groups), hd=hd, pf=pf, length=length, slots=16,
                pf_bytes=sums)


@functools.lru_cache(maxsize=None)
def flat(name):
    """A flat store by the name of its geometry, built once per process; nobody changes it."""
    return flat_store(GEOMETRIES[name], SEEDS[name])


# ------------------------------------------------------------------ planted masks: one Python int per entry
PATTERNS = ("empty", "full", "lone_last", "first_and_last_word", "last_word", "random", "orphan_lane0")
ROOT_COUNTS = (1, 64, 65, 4095, 4096)


def last_word_bits(n_roots):
    """(first root of the last word, roots in it)."""
    lo = 64 * (n_words(n_roots) - 1)
    return lo, n_roots - lo


def masks(pattern, n_e, n_roots, seed=0):
    lo, cnt = last_word_bits(n_roots)
    if pattern == "empty":
        return [0] * n_e
    if pattern == "full":
        return [full(n_roots)] * n_e
    if pattern == "lone_last":                       # the last valid position, alone
        return [1 << (n_roots - 1)] * n_e
    if pattern == "first_and_last_word":             # a bit of word 0 and a bit of the last word, moving with the entry
        return [1 << (e % min(64, n_roots)) | 1 << (lo + (e * 7) % cnt) for e in range(n_e)]
    if pattern == "last_word":                       # every root of the last word and no other
        return [(full(cnt) << lo)] * n_e
    if pattern == "orphan_lane0":                    # lane 0 of every wave holds an orphan, the others one root each
        return [0 if e % WAVE == 0 else 1 << ((e * 5) % n_roots) for e in range(n_e)]
    if pattern == "random":                          # a quarter orphans; the others sparse, dense or one word
        rng = np.random.default_rng(1000 * n_roots + seed)
        kind = rng.integers(0, 8, n_e)
        out = []
        for e in range(n_e):
            k = int(kind[e])
            if k < 2:
                out.append(0)
            elif k < 5:
                out.append(sum(1 << int(r) for r in set(rng.integers(0, n_roots, 3).tolist())))
            elif k < 7:
                out.append(int.from_bytes(rng.bytes(8 * n_words(n_roots)), "little") & full(n_roots))
            else:
                w = int(rng.integers(0, n_words(n_roots)))
                out.append((int(rng.integers(1, 1 << 62)) << (64 * w)) & full(n_roots))
            if k >= 2 and not out[-1]:               # an orphan is planted, never drawn
                out[-1] = 1 << (e % n_roots)
        return out
    raise KeyError(pattern)


# ------------------------------------------------------------------ drop-set families: Python ints
BITS_ROOTS, CYCLE_ROOTS = 17, 3
BITS_SETS = (BATCH_SETS - 1, BATCH_SETS, BATCH_SETS + 1, BATCH_SETS + 2)


def bits_of_q(n_sets):
    """Set q is the binary expansion of q: every set distinct, so an offset error of any size shows."""
    assert n_sets <= 1 << BITS_ROOTS
    return list(range(n_sets))


def bits_of_q_words(n_sets):
    return np.arange(n_sets, dtype=np.uint64).reshape(-1, 1)


def cycle(n_sets):
    """Set q is (5 q + 3) mod 8 over three roots: 8 distinct sets, each answered once by the reference."""
    return [(5 * q + 3) % 8 for q in range(n_sets)]


def cycle_sets_for(n_e):
    """n_sets = per + 2 where the byte bound binds; per is no multiple of 8 (a batch begins inside the
    cycle) and is below the set bound."""
    per = BATCH_BYTES // n_e
    if not (per < BATCH_SETS and per % 8 and n_e > BATCH_BYTES // (BATCH_SETS + 1)):
        raise RuntimeError("retain_plant: %d entries give batches of %d sets: the byte bound does not bind, or a batch "
                           "begins where the cycle does" % (n_e, per))
    assert per_of(per + 2, n_e) == per
    return per + 2


def wide(n_roots, seed=0):
    """The empty set, the full set, each single word full, the complement of one bit of word 0 and of the
    last valid bit, eight seeded random sets (for 4096 roots: 76 sets)."""
    W, f = n_words(n_roots), full(n_roots)
    rng = np.random.default_rng(77 + n_roots + seed)
    out = [0, f] + [(M64 << (64 * w)) & f for w in range(W)]
    out += [f & ~(1 << min(5, n_roots - 1)), f & ~(1 << (n_roots - 1))]
    out += [int.from_bytes(rng.bytes(8 * W), "little") & f for _ in range(8)]
    return out


def wide_index(n_roots):
    """Where wide()'s named sets lie: dict(empty, full, word0, last_word)."""
    return dict(empty=0, full=1, word0=2, last_word=2 + n_words(n_roots) - 1)


# ------------------------------------------------------------------ the reference for the drop
STAT_FIELDS = ("live_blobs", "live_bytes", "total_blobs", "total_bytes")
FREED_FIELDS = ("freed_blobs", "freed_bytes", "live_blobs", "live_bytes")


def reference_drop(store, mask_ints, sets):
    """retain_ref.drop, one call per set -> (live (n_sets, n_e) u8, stats (n_sets, n_pf, 4) u64, freed (n_sets, 4) u64)."""
    import retain_ref
    n_e, n_pf = store["n_entries"], len(store["groups"])
    live = np.zeros((len(sets), n_e), dtype=np.uint8)
    stats = np.zeros((len(sets), n_pf, 4), dtype=np.uint64)
    freed = np.zeros((len(sets), 4), dtype=np.uint64)
    for q, s in enumerate(sets):
        lv, st, fr = retain_ref.drop(store["hd"], mask_ints, bits_of(s))
        live[q], stats[q] = lv, st
        freed[q] = [fr[f] for f in FREED_FIELDS]
    return live, stats, freed


def reference_drop_cycled(store, mask_ints, sets, want_live=True):
    """reference_drop where the sets repeat: each distinct set is answered once and indexed."""
    distinct = sorted(set(sets))
    live, stats, freed = reference_drop(store, mask_ints, distinct)
    idx = np.array([distinct.index(s) for s in sets])
    return (live[idx] if want_live else None), stats[idx], freed[idx]


def reference_drop_np(store, mask_words, set_words):
    """retain_ref.drop's rules over numpy, for the family of 65,537 sets: live = a root of the mask is not
    dropped; per packfile live blobs, live bytes, blobs, bytes; freed = reached and not live.  No waves, no
    batches.  tests/test_retain_plant.py holds it equal to retain_ref.drop."""
    n_e, n_pf = store["n_entries"], len(store["groups"])
    size = (store["length"] + np.uint64(NONCE)).astype(np.int64)
    live = np.zeros((set_words.shape[0], n_e), dtype=bool)
    for w in range(mask_words.shape[1]):
        live |= (mask_words[None, :, w] & ~set_words[:, w, None]) != 0
    reached = (mask_words != 0).any(axis=1)
    onehot = (store["pf"][:, None] == np.arange(n_pf)[None, :]).astype(np.int64)
    lv = live.astype(np.int64)
    stats = np.zeros((set_words.shape[0], n_pf, 4), dtype=np.int64)
    stats[:, :, 0] = lv @ onehot
    stats[:, :, 1] = lv @ (onehot * size[:, None])
    stats[:, :, 2] = onehot.sum(axis=0)
    stats[:, :, 3] = (onehot * size[:, None]).sum(axis=0)
    gone = (~live & reached[None, :]).astype(np.int64)
    freed = np.stack([gone.sum(axis=1), gone @ size, lv.sum(axis=1), lv @ size], axis=1)
    return live.astype(np.uint8), stats.astype(np.uint64), freed.astype(np.uint64)


@functools.lru_cache(maxsize=None)
def drop_case(geometry, pattern, n_roots):
    """One planted drop, built and answered once per process: (store, masks as ints, as words, wide()'s sets
    as ints, as words, (live, stats, freed) by reference_drop)."""
    s = flat(geometry)
    m, sets = masks(pattern, s["n_entries"], n_roots), wide(n_roots)
    return s, m, to_words(m, n_roots), sets, to_words(sets, n_roots), reference_drop(s, m, sets)


@functools.lru_cache(maxsize=None)
def sets_bound_case():
    """The family of 65,537 sets over 48 entries and 17 roots: (store, mask words, set words, (live, stats,
    freed) by reference_drop_np); a test takes the first n_sets rows."""
    s = flat("sets_bound")
    mw, sw = to_words(masks("random", s["n_entries"], BITS_ROOTS), BITS_ROOTS), bits_of_q_words(BITS_SETS[-1])
    return s, mw, sw, reference_drop_np(s, mw, sw)


@functools.lru_cache(maxsize=None)
def bytes_bound_case():
    """The cycle over 4,200 entries and 3 roots, per + 2 sets: (store, mask words, set words, (None, stats,
    freed) by reference_drop_cycled, the live rows of the first 16 sets)."""
    s = flat("bytes_bound")
    m, sets = masks("random", s["n_entries"], CYCLE_ROOTS), cycle(cycle_sets_for(s["n_entries"]))
    return (s, to_words(m, CYCLE_ROOTS), to_words(sets, CYCLE_ROOTS), reference_drop_cycled(s, m, sets, want_live=False),
            reference_drop_cycled(s, m, sets[:16])[0])


# ------------------------------------------------------------------ the model of k_rt_drop and its host loop
DROP_MUTANTS = ("live_word0", "any_word0", "no_all_equal", "batch_set_q", "no_clear", "orphans_freed", "no_nonce",
                "live_stride_per")


def _kernel(store, mask_words, rows, mutant):
    """One launch of k_rt_drop over the sets `rows`, the sums taken as cleared -> (live (m, n_e) bool,
    stats (m, n_pf, 4), freed (m, 4), shapes Counter).  A launch is a function of its sets alone, so equal
    rows are computed once."""
    rows, inverse = np.unique(rows, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    n_e, n_pf, m, W = store["n_entries"], len(store["groups"]), rows.shape[0], mask_words.shape[1]
    pf = store["pf"]
    size = store["length"].astype(np.int64) + (0 if mutant == "no_nonce" else NONCE)
    lv = np.zeros((m, n_e), dtype=bool)
    for w in range(1 if mutant == "live_word0" else W):
        lv |= (mask_words[None, :, w] & ~rows[:, w, None]) != 0
    reached = (mask_words[:, :1] if mutant == "any_word0" else mask_words).any(axis=1)
    fr = ~lv if mutant == "orphans_freed" else ~lv & reached[None, :]
    stats, freed, shapes = np.zeros((m, n_pf, 4), dtype=np.int64), np.zeros((m, 4), dtype=np.int64), Counter()
    n_wg = (n_e + WORKGROUP - 1) // WORKGROUP
    for a in range(0, n_wg * WORKGROUP, WAVE):
        b = min(a + WAVE, n_e)
        if b <= a:                                   # no lane of the wave holds an entry: it returns
            shapes["idle"] += 1
            continue
        l, f, sz, p = lv[:, a:b], fr[:, a:b], size[a:b], pf[a:b]
        freed += np.stack([f.sum(axis=1), f @ sz, l.sum(axis=1), l @ sz], axis=1)
        if mutant == "no_all_equal" or (p == p[0]).all():     # lane 0 adds the wave's sums to its own packfile
            shapes["uniform"] += 1
            stats[:, p[0]] += np.stack([l.sum(axis=1), l @ sz, np.full(m, b - a), np.full(m, sz.sum())], axis=1)
        else:                                        # lane by lane
            shapes["by_lane"] += 1
            for k in range(b - a):
                stats[:, p[k], 0] += l[:, k]
                stats[:, p[k], 1] += l[:, k] * sz[k]
                stats[:, p[k], 2] += 1
                stats[:, p[k], 3] += sz[k]
    return lv[inverse], stats[inverse], freed[inverse], shapes


def model_drop(store, mask_words, set_words, want_live=True, mutant=None):
    """bw_retain_drop: batches of per sets through _kernel, the device's sums and live bytes kept between
    the batches as the session's buffers are -> (live or None, stats, freed, info dict(per, n_batches, shapes))."""
    assert mutant is None or mutant in DROP_MUTANTS
    n_e, n_pf, n_sets = store["n_entries"], len(store["groups"]), set_words.shape[0]
    per = per_of(n_sets, n_e)
    live = np.zeros((n_sets, n_e), dtype=np.uint8) if want_live else None
    stats, freed = np.zeros((n_sets, n_pf, 4), dtype=np.int64), np.zeros((n_sets, 4), dtype=np.int64)
    d_stat, d_freed = np.zeros((per, n_pf, 4), dtype=np.int64), np.zeros((per, 4), dtype=np.int64)
    stride = per if mutant == "live_stride_per" else n_e
    assert mutant != "live_stride_per" or per * max(per, n_e) < 1 << 24, "this mutant is for small cases"
    d_live = np.zeros(per * max(stride, n_e) + n_e, dtype=np.uint8)
    info = dict(per=per, n_batches=0, shapes=Counter())
    for q0 in range(0, n_sets, per):
        m = min(per, n_sets - q0)
        rows = set_words[0:m] if mutant == "batch_set_q" else set_words[q0:q0 + m]
        if mutant != "no_clear":
            d_stat[:], d_freed[:] = 0, 0
        lv, st, fr, shapes = _kernel(store, mask_words, rows, mutant)
        d_stat[:m] += st
        d_freed[:m] += fr
        if want_live:
            if stride == n_e:
                d_live[:m * n_e] = lv.reshape(-1)
            else:
                for q in range(m):               # set after set: a later row overwrites an earlier one's tail
                    d_live[q * stride:q * stride + n_e] = lv[q]
            live[q0:q0 + m] = d_live[:m * n_e].reshape(m, n_e)
        stats[q0:q0 + m], freed[q0:q0 + m] = d_stat[:m], d_freed[:m]
        info["n_batches"] += 1
        info["shapes"] = shapes
    return live, stats.astype(np.uint64), freed.astype(np.uint64), info


def wave_shapes(groups):
    """How k_rt_drop's waves lie over the packfiles: Counter(uniform, by_lane, idle), and the entries of
    the last wave that holds any."""
    n = sum(groups)
    pf = [p for p, g in enumerate(groups) for _ in range(g)]
    out = Counter()
    for a in range(0, (n + WORKGROUP - 1) // WORKGROUP * WORKGROUP, WAVE):
        lanes = pf[a:a + WAVE]
        out["idle" if not lanes else "uniform" if len(set(lanes)) == 1 else "by_lane"] += 1
    return out, (n - 1) % WAVE + 1


# ------------------------------------------------------------------ tree stores for the mark
def _tree_case(b, roots, **info):
    n = len(b.blobs)
    packs, index = b.finish(target=4)
    return dict(packs=packs, index=index, roots=list(roots), n_entries=n, verify=False, slots=16, info=info)


def staircase(k=3):
    """Root A reaches the subtrees s1 .. sk directly.  Root B reaches s1 at the bottom of a chain five
    deep (b1 .. b4), and every s_j reaches s_{j+1} at the bottom of a chain four deep of its own (c_j1 ..
    c_j3).  The walk expands every s_j on level 1, so the edge that brings B's bit to s_{j+1} (level 4)
    lies after s_{j+1}'s own out-edges (level 1) in every sweep: B's bit goes one step of the staircase
    per sweep, k + 1 productive sweeps in all, whatever the lanes do inside a launch."""
    import restore_store
    b = restore_store.Builder(seed=190)
    spec = {"x%d" % k: (b"X%d" % k) * 20}
    specs = [spec]
    for j in range(k - 1, 0, -1):
        spec = {"x%d" % j: (b"X%d" % j) * 20, "c%d1" % j: {"c%d2" % j: {"c%d3" % j: {"s%d" % (j + 1): spec}}}}
        specs.insert(0, spec)
    ra = b.add_dir("a", {"s%d" % (j + 1): specs[j] for j in range(k)})
    rb = b.add_dir("b", {"b1": {"b2": {"b3": {"b4": {"s1": specs[0]}}}}})
    return _tree_case(b, [ra, rb], k=k)


CYCLED_DISTINCT = 10
MISSING = b"\x11" * 32
CHUNK = b"the chunk that is given as a root".ljust(48, b".")


def cycled_layout(n, seed=0):
    """which distinct root stands at each of n places: 0 .. 3 exactly once, at 0, 63, 64 and n - 1; the
    missing hash (4) at 65, the chunk's hash (5) at n - 2; 6 twice, at 1 and n - 3 (one bit in the first
    word and one in another); 7 .. 9 everywhere else by a seeded draw."""
    assert n >= 130
    which = np.random.default_rng(500 + n + seed).integers(7, CYCLED_DISTINCT, n).tolist()
    for at, d in ((0, 0), (63, 1), (64, 2), (n - 1, 3), (65, 4), (n - 2, 5), (1, 6), (n - 3, 6)):
        which[at] = d
    return which


@functools.lru_cache(maxsize=None)
def cycled_roots(n):
    """Ten distinct small roots repeated to n: Dirs with a file of their own, some sharing a directory,
    one hash that is a file chunk's (ENOTTREE) and one that is nowhere (ENOTFOUND)
    -> a case with roots (n hashes), distinct (the ten) and which (cycled_layout)."""
    import restore_store
    from oracle import oracle
    b = restore_store.Builder(seed=191)
    sh1, sh2 = {"p": b"P" * 40, "q": b"Q" * 40}, {"u": b"U" * 40}
    own = lambda d: ("own-%d" % d).encode().ljust(24, b".")
    extra = {0: {"sh": sh1}, 1: {"sh2": sh2}, 2: {"c": CHUNK}, 3: {}, 6: {"sh": sh1}, 7: {"sh2": sh2}, 8: {"sh": sh1, "sh2": sh2}, 9: {}}
    distinct = []
    for d in range(CYCLED_DISTINCT):
        if d == 4:
            distinct.append(MISSING)
        elif d == 5:
            distinct.append(oracle.blake3(CHUNK))
        else:
            distinct.append(b.add_dir("d%d" % d, dict({"own": own(d)}, **extra[d])))
    which = cycled_layout(n)
    case = _tree_case(b, [distinct[d] for d in which])
    case.update(distinct=distinct, which=which)
    return case


def expand(which, masks_d, per_root_d, errors_d, info_d):
    """The header's rule that every given root has its own bit, applied to the results over the distinct
    roots: a blob's set holds every place its roots stand at; a root's record is its distinct root's,
    except that it holds a blob alone only when it stands at one place; a root's error is met once per
    place, under that place's index -> (masks, per_root, errors, info)."""
    places = [0] * (max(which) + 1)
    for i, d in enumerate(which):
        places[d] |= 1 << i
    count = Counter(which)
    out = [sum(places[d] for d in bits_of(m)) for m in masks_d]
    per_root = []
    for d in which:
        r = dict(per_root_d[d])
        if count[d] > 1:
            r["unique_blobs"] = r["unique_bytes"] = 0
        per_root.append(r)
    errors = Counter()
    for (h, parent, pos, reason), c in errors_d.items():
        if parent == ZERO and pos != NONE:           # a root's error: child_pos is the root's index
            for i in bits_of(places[pos]):
                errors[(h, parent, i, reason)] += c
        else:
            errors[(h, parent, pos, reason)] += c
    return out, per_root, errors, {k: v for k, v in info_d.items() if k not in ("walk", "n_sweeps")}


def _store_of(case):
    import prune_ref
    import restore_ref
    import restore_store
    return (restore_ref.Store(restore_store.PRK, case["packs"], case["index"], verify=case["verify"]),
            prune_ref.headers_of(restore_store.PRK, case["packs"]))


@functools.lru_cache(maxsize=None)
def cycled_reference(n):
    """(case, headers, masks, damaged, per_root, errors, info) of cycled_roots(n): retain_ref.mark over the
    ten distinct roots, expanded."""
    import retain_ref
    case = cycled_roots(n)
    store, hd = _store_of(case)
    masks_d, damaged, per_root_d, errors_d, info_d = retain_ref.mark(store, hd, case["distinct"])
    m, per_root, errors, info = expand(case["which"], masks_d, per_root_d, errors_d, info_d)
    return case, hd, m, damaged, per_root, errors, info


@functools.lru_cache(maxsize=None)
def staircase_reference(k=3):
    """(case, headers, masks, damaged, per_root, errors, info) of staircase(k), by retain_ref.mark."""
    import retain_ref
    case = staircase(k)
    store, hd = _store_of(case)
    return (case, hd) + tuple(retain_ref.mark(store, hd, case["roots"]))


def walk_of(case):
    import retain_ref
    store, hd = _store_of(case)
    return retain_ref.walk(store, hd, case["roots"]), hd


# ------------------------------------------------------------------ the model of seed, propagate and stats
MARK_MUTANTS = ("word0_only", "seed_and_31", "unique_own_word", "k_sweeps", "leaf_first")
ENOTTREE = 19


def model_mark(w, hd, n_roots, mutant=None, k=3):
    """k_rt_seed, the host's sweeps of k_rt_propagate and k_rt_stats over retain_ref.walk's edges, word by
    word -> (masks, per_root, totals dict, n_sweeps).  Inside a sweep the edges are taken level by level in
    list order, as retain_ref.fixed_point takes them."""
    import prune_ref
    assert mutant is None or mutant in MARK_MUTANTS
    n = w["n_entries"]
    size = [NONCE + ent[4] for ent in prune_ref.flat_entries(hd)]
    reach, opened, status = [0] * n, [0] * n, []
    for i, s in enumerate(w["seeds"]):
        if s is None:
            status.append(w["status"][i])
            continue
        bit = 1 << (64 * (i >> 6) + (i & (31 if mutant == "seed_and_31" else 63)))
        reach[s[0]] |= bit
        if s[1]:
            opened[s[0]] |= bit
        status.append(0 if s[1] else ENOTTREE)
    passed = (lambda p: opened[p] & M64) if mutant == "word0_only" else (lambda p: opened[p])

    def leaves():
        for edges in w["levels"]:
            for p, c, tree in edges:
                if not tree:
                    reach[c] |= passed(p)

    if mutant == "leaf_first":
        leaves()
    sweeps, changed = 0, True
    while changed and not (mutant == "k_sweeps" and sweeps == k):
        changed = False
        sweeps += 1
        for edges in w["levels"]:
            for p, c, tree in edges:
                pv = passed(p)
                if tree and (pv & ~reach[c] or pv & ~opened[c]):
                    reach[c] |= pv
                    opened[c] |= pv
                    changed = True
    if mutant != "leaf_first":
        leaves()
    per_root = [dict(reached_blobs=0, reached_bytes=0, unique_blobs=0, unique_bytes=0, n_damaged=0, status=status[i], pad=0)
                for i in range(n_roots)]
    totals = dict(reached_blobs=0, reached_bytes=0, orphan_blobs=0, orphan_bytes=0)
    for e, m in enumerate(reach):
        totals["reached_blobs" if m else "orphan_blobs"] += 1
        totals["reached_bytes" if m else "orphan_bytes"] += size[e]
        for r in bits_of(m):
            pop = bin((m >> (64 * (r >> 6))) & M64 if mutant == "unique_own_word" else m).count("1")
            rec = per_root[r]
            rec["reached_blobs"] += 1
            rec["reached_bytes"] += size[e]
            if pop == 1:
                rec["unique_blobs"] += 1
                rec["unique_bytes"] += size[e]
            if e in w["damaged"]:
                rec["n_damaged"] += 1
    return reach, per_root, totals, sweeps
