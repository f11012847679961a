"""Independent BLAKE3 for the parity tests: the upstream C implementation that ROCm's LLVM carries
with prefixed symbols (llvm_blake3_hasher_init / _update / _finalize, llvm_blake3_version), through
ctypes.  Test infrastructure only: the CPU tests and tests/golden/make_blake3_upstream.py use it; no
GPU test does (a GPU host need not have the library), they compare with the committed fixture."""
import ctypes
import glob
import os

KAT = {b"": "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262",
       b"abc": "6437b3ac38465133ffb63b75273a8db548c558465d79db03fd359c6cd5bd9d85",
       b"\x00": "2d3adedff11b61f14c886e35afa036736dcd87a74d27b5c1510225d0f592e213"}

PATTERNS = ("lib/llvm/lib/libclang-cpp.so*", "lib/llvm/lib/libLLVM*.so*")
HASHER_BYTES = 4096  # upstream's blake3_hasher is 1,912 bytes

_lib = None
_path = None
_searched = False


def _find():
    """The first candidate under the ROCm root that exports the hasher, or None."""
    global _lib, _path, _searched
    if _searched:
        return _lib
    _searched = True
    root = os.environ.get("ROCM_PATH") or "/opt/rocm"
    for pat in PATTERNS:
        for p in sorted(glob.glob(os.path.join(root, pat))):
            try:
                L = ctypes.CDLL(p)
            except OSError:
                continue
            if not all(hasattr(L, "llvm_blake3_" + f) for f in ("version", "hasher_init", "hasher_update",
                                                                  "hasher_finalize")):
                continue
            L.llvm_blake3_version.restype = ctypes.c_char_p
            L.llvm_blake3_version.argtypes = []
            L.llvm_blake3_hasher_init.restype = None
            L.llvm_blake3_hasher_init.argtypes = [ctypes.c_void_p]
            L.llvm_blake3_hasher_update.restype = None
            L.llvm_blake3_hasher_update.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
            L.llvm_blake3_hasher_finalize.restype = None
            L.llvm_blake3_hasher_finalize.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
            _lib, _path = L, p
            for m, d in KAT.items():  # a library that is there but wrong is an error, not a skip
                got = _hash(L, m).hex()
                if got != d:
                    raise AssertionError("%s: BLAKE3(%r) = %s, the published answer is %s" % (p, m, got, d))
            return _lib
    return None


def _hash(L, buf):
    if hasattr(buf, "ctypes"):  # a numpy array: hashed in place, by pointer
        import numpy as np
        keep = buf if buf.flags.c_contiguous else np.ascontiguousarray(buf)
        n, ptr = keep.nbytes, ctypes.c_void_p(keep.ctypes.data)
    else:
        keep = bytes(buf)
        n, ptr = len(keep), keep  # (ctypes passes the bytes object's own buffer)
    st = ctypes.create_string_buffer(HASHER_BYTES)  # zeroed
    out = ctypes.create_string_buffer(32)
    L.llvm_blake3_hasher_init(st)
    if n:
        L.llvm_blake3_hasher_update(st, ptr, ctypes.c_size_t(n))
    L.llvm_blake3_hasher_finalize(st, out, ctypes.c_size_t(32))
    return out.raw


def available():
    return _find() is not None


def path():
    return _path if available() else None


def version():
    """The version string the library reports (upstream's BLAKE3_VERSION_STRING)."""
    L = _find()
    if L is None:
        raise RuntimeError("no library exporting llvm_blake3_hasher_init under the ROCm root")
    return L.llvm_blake3_version().decode()


def hash(buf):
    """BLAKE3(buf) -> 32 bytes; buf is bytes-like or a uint8 numpy array (read in place)."""
    L = _find()
    if L is None:
        raise RuntimeError("no library exporting llvm_blake3_hasher_init under the ROCm root")
    return _hash(L, buf)
