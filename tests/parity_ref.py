"""Parity in plain numpy: the yardstick of tests/test_parity.py, tests/test_gpu_gf_matmul.py and
tests/test_gpu_parity_shards.py.  GF(2^8) with the polynomial 0x11d (x^8 + x^4 + x^3 + x^2 + 1) and the
generator 2; a systematic Reed-Solomon code whose parity rows are the Cauchy matrix C[i][j] = inv(i ^ (m + j));
the manifest codec of backuwup_amd/parity.py restated from its description."""
import struct

import numpy as np

POLY = 0x11d


def xtime(a):
    a <<= 1
    return (a ^ POLY) & 0xff if a & 0x100 else a


EXP = np.zeros(512, dtype=np.uint8)
LOG = np.zeros(256, dtype=np.int32)
_x = 1
for _i in range(255):
    EXP[_i] = _x
    LOG[_x] = _i
    _x = xtime(_x)
EXP[255:510] = EXP[:255]
# MUL[a][b]: the whole table, so that a matrix product is one fancy index per coefficient
_a = np.arange(256)
MUL = np.where((_a[:, None] == 0) | (_a[None, :] == 0), 0, EXP[(LOG[:, None] + LOG[None, :]) % 255]).astype(np.uint8)


def mul(a, b):
    return 0 if a == 0 or b == 0 else int(EXP[LOG[a] + LOG[b]])


def inv(a):
    assert a != 0
    return int(EXP[255 - LOG[a]])


def cauchy(k, m):
    assert k >= 1 and m >= 1 and k + m <= 256
    return np.array([[inv(i ^ (m + j)) for j in range(k)] for i in range(m)], dtype=np.uint8)


def generator(k, m):
    return np.concatenate([np.eye(k, dtype=np.uint8), cauchy(k, m)])


def matmul(matrix, srcs, length):
    """dst_r[b] = XOR_c mul(M[r][c], src_c[b]) for b < length; src_c (bytes or a uint8 array) reads as zero
    at and beyond its length.  Returns rows x length uint8."""
    matrix = np.asarray(matrix, dtype=np.uint8)
    rows, cols = matrix.shape
    assert cols == len(srcs)
    out = np.zeros((rows, length), dtype=np.uint8)
    for c, s in enumerate(srcs):
        s = np.frombuffer(bytes(s), dtype=np.uint8) if not isinstance(s, np.ndarray) else s
        n = min(len(s), length)
        if not n:
            continue
        for r in range(rows):
            if matrix[r, c]:
                out[r, :n] ^= MUL[matrix[r, c]][s[:n]]
    return out


def gauss_inverse(a):
    """The inverse of a square matrix over GF(2^8) by Gauss-Jordan, or None where it is singular."""
    n = len(a)
    w = np.concatenate([np.asarray(a, dtype=np.uint8).reshape(n, n), np.eye(n, dtype=np.uint8)], axis=1)
    for c in range(n):
        p = next((r for r in range(c, n) if w[r, c]), None)
        if p is None:
            return None
        if p != c:
            w[[c, p]] = w[[p, c]]
        w[c] = MUL[inv(int(w[c, c]))][w[c]]
        for r in range(n):
            if r != c and w[r, c]:
                w[r] ^= MUL[w[r, c]][w[c]]
    return w[:, n:].copy()


def small_matmul(a, b):
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    out = np.zeros((a.shape[0], b.shape[1]), dtype=np.uint8)
    for i in range(a.shape[0]):
        for t in range(a.shape[1]):
            if a[i, t]:
                out[i] ^= MUL[a[i, t]][b[t]]
    return out


class TooFew(Exception):
    pass


def solve(k, m, present):
    """(used, missing, matrix): the inputs are every present data shard, then the lowest-numbered present
    parity shards to make k; matrix (len(missing) x k) times the inputs gives every missing shard."""
    present = [bool(p) for p in present]
    assert len(present) == k + m
    used = [s for s in range(k) if present[s]]
    used += [s for s in range(k, k + m) if present[s]][:k - len(used)]
    missing = [s for s in range(k + m) if not present[s]]
    if len(used) < k:
        raise TooFew(missing)
    g = generator(k, m)
    ainv = gauss_inverse(g[used])
    assert ainv is not None
    return used, missing, small_matmul(g[missing], ainv) if missing else np.zeros((0, k), np.uint8)


def plan(sizes, k, m):
    """[(first_packfile, k, m, shard_len, out_offset)], out_bytes."""
    assert k >= 1 and m >= 1 and k + m <= 256 and all(s > 0 for s in sizes)
    groups, at = [], 0
    for first in range(0, len(sizes), k):
        member = sizes[first:first + k]
        length = (max(member) + 15) & ~15
        groups.append((first, len(member), m, length, at))
        at += m * length
    return groups, at


def encode(packfiles, k, m):
    """The parity shards of a list of packfiles (bytes), group by group: [bytes], with the plan."""
    groups, _ = plan([len(p) for p in packfiles], k, m)
    out = []
    for first, kk, mm, length, _ in groups:
        out += [r.tobytes() for r in matmul(cauchy(kk, mm), packfiles[first:first + kk], length)]
    return out, groups


# ---- the manifest: little-endian; u32 version = 1, u32 n_groups, per group u32 k, u32 m, u64 shard_len,
# k x {id[12], u32 0, u64 size, digest[32]}, m x digest[32]
MANIFEST_VERSION = 1
MANIFEST_INFO_TEXT = b"backuwup parity manifest v1"


def manifest_encode(groups):
    """groups: [dict(k, m, shard_len, ids [12 bytes], sizes, data_digests [32 bytes], parity_digests)]."""
    out = [struct.pack("<II", MANIFEST_VERSION, len(groups))]
    for g in groups:
        assert len(g["ids"]) == len(g["sizes"]) == len(g["data_digests"]) == g["k"] and len(g["parity_digests"]) == g["m"]
        out.append(struct.pack("<IIQ", g["k"], g["m"], g["shard_len"]))
        for i, n, d in zip(g["ids"], g["sizes"], g["data_digests"]):
            assert len(i) == 12 and len(d) == 32
            out.append(bytes(i) + struct.pack("<IQ", 0, n) + bytes(d))
        for d in g["parity_digests"]:
            assert len(d) == 32
            out.append(bytes(d))
    return b"".join(out)


def manifest_decode(buf):
    buf = bytes(buf)
    version, n = struct.unpack_from("<II", buf, 0)
    if version != MANIFEST_VERSION:
        raise ValueError("parity manifest version %d" % version)
    at, groups = 8, []
    for _ in range(n):
        k, m, length = struct.unpack_from("<IIQ", buf, at)
        at += 16
        g = dict(k=k, m=m, shard_len=length, ids=[], sizes=[], data_digests=[], parity_digests=[])
        for _ in range(k):
            pad, size = struct.unpack_from("<IQ", buf, at + 12)
            if pad:
                raise ValueError("parity manifest: nonzero padding")
            g["ids"].append(buf[at:at + 12])
            g["sizes"].append(size)
            g["data_digests"].append(buf[at + 24:at + 56])
            at += 56
        for _ in range(m):
            g["parity_digests"].append(buf[at:at + 32])
            at += 32
        groups.append(g)
    if at != len(buf):
        raise ValueError("parity manifest: %d trailing bytes" % (len(buf) - at))
    return groups
