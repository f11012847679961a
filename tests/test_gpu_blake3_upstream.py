"""Every device BLAKE3 path against upstream BLAKE3, through tests/golden/blake3_upstream.json alone
(no oracle, no live library: see tests/test_blake3_upstream.py for how the fixture is pinned).

The SMALL cases walk the quad-lane small-message hash (b3q_message in bw_b3_small.hip: its loader,
the masking of the word that holds the message's end, the level-by-level merge with its odd node
carried up) over every leaf count 1..64 at -1/0/+1 byte and every tail position of the last 16-byte
word, through each of its transports: the persistent hash service with its requests in HBM, the
same with its requests in pinned host memory, and the launched batch.  The batch kernels (k_b3_lines,
k_b3_upper) and the product entry see the same cases plus the TREE ones."""
import ctypes
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import blake3_cases as cases
from backuwup_amd import _lib, make_params
from backuwup_amd._lib import BW_F_NO_DEDUP, BW_OPT_B3_GROUP
from backuwup_amd.synth import splitmix_bytes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "blake3_upstream.json")))
MSG_MAX = 65536  # the small-message path's limit (B3_MSG_MAX); a longer message runs on the caller's context


def _aligned(a, align=128):
    """A copy of uint8 array `a` whose first byte sits on an `align`-byte boundary."""
    raw = np.empty(a.size + align, dtype=np.uint8)
    s = (-raw.ctypes.data) % align
    out = raw[s:s + a.size]
    out[:] = a
    assert out.ctypes.data % align == 0
    return out


@pytest.fixture(scope="module")
def small():
    """(source on a 128-byte boundary, [(off, n)], [digest]): a case's residue mod 16 is its off."""
    src = _aligned(cases.small_source())
    src.setflags(write=False)
    return src, cases.small_cases(), cases.digests(FIX, "small")


@pytest.fixture(scope="module")
def tree():
    src = cases.tree_source()
    src.setflags(write=False)
    return src, cases.tree_cases(), cases.digests(FIX, "tree")


def _check(cs, got, want):
    """Every digest equals the fixture's; a mismatch reports how the failing (off, n) split by block
    tail (a whole last block or a partial one) beside the first of them."""
    assert len(got) == len(want) == len(cs)
    bad = [c for c, g, w in zip(cs, got, want) if g != w]
    if bad:
        whole = [c for c in bad if c[1] % 64 == 0]
        print("mismatches: %d of %d; with n %% 64 == 0: %d %s; first with a partial block: %s"
              % (len(bad), len(cs), len(whole), whole[:40], [c for c in bad if c[1] % 64][:40]))
    assert not bad, (len(bad), bad[:12])


# ------------------------------------------------------------------ the batch path

@pytest.fixture(scope="module")
def packed(small, tree):
    """The SMALL offset-0 cases, then the TREE cases, in one buffer: message i starts where the
    address is (37 * i) % 128 mod 128 (every start offset of k_b3_lines' 128-byte line ring) and
    otherwise right after message i - 1, so that waves straddle blobs; the last one ends exactly at
    the buffer's end.  The gaps hold 0xFF, which a read past a message's end would hash."""
    msgs = [(small[0], off, n, d) for (off, n), d in zip(small[1], small[2]) if off == 0]
    msgs += [(tree[0], off, n, d) for (off, n), d in zip(tree[1], tree[2])]
    offs, pos = [], 0
    for i, (_, _, n, _) in enumerate(msgs):
        pos += (37 * i - pos) % 128
        offs.append(pos)
        pos += n
    buf = _aligned(np.full(pos, 0xFF, dtype=np.uint8))
    for o, (src, off, n, _) in zip(offs, msgs):
        buf[o:o + n] = src[off:off + n]
    assert offs[-1] + msgs[-1][2] == buf.size
    assert all((buf.ctypes.data + o) % 128 == (37 * i) % 128 for i, o in enumerate(offs))
    cs = [(o % 128, n) for o, (_, _, n, _) in zip(offs, msgs)]
    return buf, np.array(offs, dtype=np.uint64), np.array([m[2] for m in msgs], dtype=np.uint64), cs, \
        [m[3] for m in msgs]


@pytest.mark.parametrize("group", [0, 4, 2, 1], ids=["lines", "lines-g4", "lines-g2", "lines-g1"])
def test_batch_path(ctx, packed, group):
    buf, offs, lens, cs, want = packed
    ctx.set_option(BW_OPT_B3_GROUP, group)
    try:
        got = ctx.blake3_many(buf, offs, lens)
    finally:
        ctx.set_option(BW_OPT_B3_GROUP, 0)  # the context default
    _check(cs, [bytes(g) for g in got], want)


# ------------------------------------------------------------------ the single-message entry

def test_single_message_entry(ctx, small):
    src, cs, want = small
    k = [i for i, (off, _) in enumerate(cs) if off == 0]
    assert len(k) == 410
    _check([cs[i] for i in k], [ctx.blake3(src[:cs[i][1]]) for i in k], [want[i] for i in k])


# ------------------------------------------------------------------ the hash service, on the caller's memory

def test_hash_service_one_thread(ctx, small):
    src, cs, want = small
    assert src.ctypes.data % 16 == 0 and {off % 16 for off, _ in cs} == {0, 1, 5, 15}
    _check(cs, [ctx.blake3_at(src, off, n) for off, n in cs], want)


def test_hash_service_four_threads_one_context(ctx, small):
    src, cs, want = small
    got, errors = [None] * len(cs), []
    big = threading.Lock()  # a message over 64 KiB runs on the context, which one thread uses at a time

    def worker(t):
        try:
            for i in range(t, len(cs), 4):
                off, n = cs[i]
                if n > MSG_MAX:
                    with big:
                        got[i] = ctx.blake3_at(src, off, n)
                else:
                    got[i] = ctx.blake3_at(src, off, n)
        except Exception as e:  # reported below
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    assert not errors, errors
    assert not any(x.is_alive() for x in th)
    _check(cs, got, want)


def test_hash_service_dropin_entry_hashes(ctx, small):
    """bw_blake3_hash_dropin with no live chunker: nothing is answered from kept digests."""
    src, cs, want = small
    L = _lib.load()
    hits0 = L.bw_blake3_kept_hits()
    got = [ctx.blake3_at(src, off, n, kept=True) for off, n in cs]
    assert L.bw_blake3_kept_hits() == hits0
    _check(cs, got, want)


def test_hash_service_dropin_device_entry(ctx, small):
    """bw_blake3_hash_dropin_device(0, ...): no context.  By its contract a message over 64 KiB is
    refused with BW_EAGAIN and nothing changed; every other case is hashed."""
    src, cs, want = small
    L = _lib.load()
    out = (ctypes.c_uint8 * 32)()
    got, refused = [], []
    for off, n in cs:
        rc = L.bw_blake3_hash_dropin_device(0, ctypes.c_void_p(src.ctypes.data + off), n, out)
        if n > MSG_MAX:
            refused.append(rc)
            got.append(None)
        else:
            assert rc == _lib.BW_OK, (off, n, rc)
            got.append(bytes(out))
    assert refused == [_lib.BW_EAGAIN] * 16  # 64 KiB + 1 and 65 KiB - 1, + 0, + 1, at the four offsets
    k = [i for i, (_, n) in enumerate(cs) if n <= MSG_MAX]
    _check([cs[i] for i in k], [got[i] for i in k], [want[i] for i in k])


# ------------------------------------------------------------------ the other two transports

_CHILD = """
import sys, threading
sys.path[:0] = [%r, %r]
import numpy as np
import blake3_cases as cases
from backuwup_amd import Context
raw = cases.small_source()
buf = np.empty(raw.size + 128, dtype=np.uint8)
s = (-buf.ctypes.data) %% 128
src = buf[s:s + raw.size]
src[:] = raw
cs = [(off, n) for off, n in cases.small_cases() if off == 5]
got = [None] * len(cs)
big = threading.Lock()
with Context(0) as c:
    def worker(t):
        for i in range(t, len(cs), 4):
            off, n = cs[i]
            if n > 65536:
                with big:
                    got[i] = c.blake3_at(src, off, n).hex()
            else:
                got[i] = c.blake3_at(src, off, n).hex()
    th = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    [x.start() for x in th]
    [x.join() for x in th]
print("@@ " + "".join(got))
"""


@pytest.mark.parametrize("env", [{"BW_SVC_HOST_RING": "1"}, {"BW_DROPIN_SERVICE": "0"}],
                         ids=["host-ring", "launched-batch"])
def test_other_transports(small, env):
    """The hash service with its requests in pinned host memory, and the launched-batch coalescer:
    each in a fresh child process (the library reads the choice once per process), one after the
    other; the child prints its digests and the comparison with the fixture happens here."""
    _, cs, want = small
    k = [i for i, (off, _) in enumerate(cs) if off == 5]
    assert len(k) == 410
    out = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(HERE), HERE)], capture_output=True,
                         text=True, timeout=120, env=dict(os.environ, **env))
    assert out.returncode == 0, (env, out.returncode, out.stderr[-2000:])
    line = [l for l in out.stdout.splitlines() if l.startswith("@@ ")]
    assert line, (out.stdout[-2000:], out.stderr[-2000:])
    raw = bytes.fromhex(line[0][3:])
    assert len(raw) == 32 * len(k)
    _check([cs[i] for i in k], [raw[32 * j:32 * j + 32] for j in range(len(k))], [want[i] for i in k])


# ------------------------------------------------------------------ the product entry

def test_product_entry(ctx, small):
    """One bw_process_files call (BW_F_NO_DEDUP): every SMALL offset-0 message as a file of its own,
    back to back with no padding, each at most 1 MiB and so one blob; a 5 MiB file in the middle is
    chunked, so the CDC and the unit paths share the launch."""
    src, cs, want = small
    k = [i for i, (off, _) in enumerate(cs) if off == 0]
    lens = [cs[i][1] for i in k]
    digs = [want[i] for i in k]
    mid, big_len = len(k) // 2, 5 << 20
    parts = [src[:n] for n in lens]
    parts.insert(mid, splitmix_bytes(4244, big_len))
    lens.insert(mid, big_len)
    digs.insert(mid, None)
    data = np.concatenate(parts)
    fl = np.array(lens, dtype=np.uint64)
    fo = np.concatenate([[0], np.cumsum(fl)[:-1]]).astype(np.uint64)
    assert int(fo[-1] + fl[-1]) == data.size
    got = ctx.process_files(data, fo, fl, make_params(flags=BW_F_NO_DEDUP))
    files = got["file"].astype(np.int64)
    assert np.all(np.diff(files) >= 0) and files[0] == 0 and files[-1] == len(lens) - 1  # canonical order
    per_file = np.bincount(files, minlength=len(lens))
    assert per_file[mid] >= 2 and np.all(np.delete(per_file, mid) == 1)
    bigs = got[files == mid]
    assert int(bigs["length"].sum()) == big_len  # its blobs tile it
    assert np.array_equal(bigs["offset"][1:], np.cumsum(bigs["length"])[:-1]) and bigs["offset"][0] == 0
    ones = got[files != mid]
    assert np.array_equal(ones["length"], np.delete(fl, mid)) and not ones["offset"].any()
    one_cs = [(0, n) for n in np.delete(fl, mid).tolist()]
    _check(one_cs, [bytes(d) for d in ones["digest"]], [d for d in digs if d is not None])
