"""Frames for the decoder tests (tests/test_zstd_decode_host.py on the CPU, tests/test_gpu_zstd_decode.py
on the device): the census corpus compressed by the system libzstd at five levels, the fixed-seed
mutations of its smaller frames, hand-made frames, and the stand-alone host program around the
decoder core (tests/cpp/zstd_dec_host.cpp) built with ASan/UBSan."""
import functools
import os
import random
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import zstd_corpus  # noqa: E402
import zstd_ref  # noqa: E402

LEVELS = (1, 3, 7, 13, 19)
CAP = 3 * 1024 * 1024  # BLOB_MAX_UNCOMPRESSED_SIZE, the capacity unpack.rs:67 decodes into
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
MUTATION_SEED = 20240607
MUTATION_LEVELS = (3, 19)
MUTATION_MAX_BLOB = 300_000
MUTATIONS_PER_FRAME = 8


@functools.lru_cache(maxsize=None)
def blobs():
    """The census corpus: [(name, bytes)], 73 blobs and 12.8 MB."""
    out = [("%s_%d" % (k, n), b) for k, n, b in zstd_corpus.corpus([300, 5000, 70000, 400000], seed=1)]
    out += [("%s_%d_%d" % (k, n, s), b) for k, n, s, b in zstd_corpus.edge_corpus()]
    return out


@functools.lru_cache(maxsize=None)
def frames():
    """[(name, level, source bytes, frame)] for every blob at every level."""
    return [(name, lv, b, zstd_ref.compress(b, lv)) for name, b in blobs() for lv in LEVELS]


@functools.lru_cache(maxsize=None)
def mutations():
    """[(name, kind, frame)]: each frame of the sub-300,000-byte blobs at levels 3 and 19, mutated
    eight ways, cycling through a bit flip anywhere, a truncation, a random byte in the first 12 and
    one byte appended."""
    r = random.Random(MUTATION_SEED)
    out = []
    for name, lv, b, f in frames():
        if lv not in MUTATION_LEVELS or len(b) >= MUTATION_MAX_BLOB:
            continue
        for k in range(MUTATIONS_PER_FRAME):
            m = bytearray(f)
            kind = ("flip", "truncate", "head", "append")[k % 4]
            if kind == "flip":
                m[r.randrange(len(m))] ^= 1 << r.randrange(8)
            elif kind == "truncate":
                del m[r.randrange(len(m)):]
            elif kind == "head":
                m[r.randrange(min(12, len(m)))] = r.randrange(256)
            else:
                m.append(r.randrange(256))
            out.append(("%s_l%d_%d" % (name, lv, k), kind, bytes(m)))
    return out


@functools.lru_cache(maxsize=None)
def libzstd_verdicts():
    """Per mutation: the bytes libzstd decodes (capacity 3 MiB), or None where it returns an error."""
    out = []
    for _, _, m in mutations():
        try:
            out.append(zstd_ref.decompress(m, CAP))
        except ValueError:
            out.append(None)
    return out


# ------------------------------------------------------------------ hand-made frames
def block(btype, body, last, size=None):
    """A block header (RFC 8878 3.1.1.2) + body; size defaults to the body's length."""
    size = len(body) if size is None else size
    return ((size << 3) | (btype << 1) | (1 if last else 0)).to_bytes(3, "little") + body


def frame_3mib_plus_1():
    """24 RLE blocks of 128 KiB and one more byte: regenerates 3 MiB + 1."""
    f = bytearray(b"\x00\x58")
    for _ in range(24):
        f += block(1, b"a", False, 128 * 1024)
    return bytes(f + block(1, b"a", True, 1))


def _back_bits(fields):
    """A backward bitstream: fields [(value, nbits)] in the order the decoder reads them."""
    total = sum(n for _, n in fields)
    acc, at = 0, total
    for v, n in fields:
        at -= n
        acc |= (v & ((1 << n) - 1)) << at
    acc |= 1 << total  # the end mark
    return acc.to_bytes(total // 8 + 1, "little")


def one_sequence_frame(lits, ll, ml_code_value, offset_code, offset_bits):
    """A frame of one compressed block with raw literals `lits` and one sequence (literal length ll < 16, match length 3 + ml_code_value < 35, the given offset
    code and extra bits), every table in RLE mode."""
    assert ll < 16 and ml_code_value < 32 and len(lits) < 32
    body = bytes([len(lits) << 3]) + lits            # raw literals, 1-byte header
    body += bytes([1, 0b01010100, ll, offset_code, ml_code_value])  # 1 sequence; LL, OF, ML tables RLE
    body += _back_bits([(offset_bits, offset_code)])  # RLE tables: states take no bits; LL/ML codes < 16/32: no extra bits
    return b"\x00\x00" + block(2, body, True)


def offset_past_output_frame():
    """8 literals, then a match at offset 9: one past the 8 bytes produced."""
    return one_sequence_frame(b"abcdefgh", 8, 1, 3, (9 + 3) - 8)   # offset_value 12 = (1 << 3) + 4


def offset_at_output_frame():
    """The same with offset 8, the furthest valid one: regenerates abcdefgh + abcd."""
    return one_sequence_frame(b"abcdefgh", 8, 1, 3, (8 + 3) - 8)


def offset_code_31_frame():
    return one_sequence_frame(b"abcdefgh", 8, 1, 31, 5)


# ------------------------------------------------------------------ the host program
def build_host(tmp_dir, sanitize=True):
    """The host program; sanitize=False: a plain -O2 build (the GPU tests' reference for the cause
    of a refusal -- sanitizer builds run in the CPU tests only)."""
    exe = os.path.join(str(tmp_dir), "zstd_dec_host" + ("" if sanitize else "_plain"))
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + (SAN if sanitize else ["-O2"]) +
                          [os.path.join(HERE, "cpp", "zstd_dec_host.cpp"), "-o", exe])
    return exe


def run_host(exe, cases, tmp_dir, tag="cases", sanitized=True):
    """cases: [(frame, dst_cap)] -> [(error, out bytes, canary intact)]; any sanitizer report
    fails the run (-fno-sanitize-recover, abort_on_error).  sanitized=False (a plain build): the
    child runs in the caller's environment, untouched."""
    inp, outp = os.path.join(str(tmp_dir), tag + ".in"), os.path.join(str(tmp_dir), tag + ".out")
    with open(inp, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for frame, cap in cases:
            f.write(struct.pack("<II", len(frame), cap))
            f.write(frame)
    env = None
    if sanitized:
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
        env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe, inp, outp], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    raw = open(outp, "rb").read()
    out, at = [], 0
    for _ in cases:
        e, n, canary = struct.unpack_from("<iII", raw, at)
        at += 12
        out.append((e, raw[at:at + n], bool(canary)))
        at += n
    assert at == len(raw)
    return out
