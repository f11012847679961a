#!/usr/bin/env python3
"""Generate tests/golden/blake3_upstream.json with upstream BLAKE3 (tests/blake3_upstream.py: the C
implementation inside ROCm's LLVM, nothing this project wrote).  The cases are tests/blake3_cases.py;
the file holds the version the library reports, the sha256 of each source buffer and, per group,
the digests in case order as one hex string.
Run:  python tests/golden/make_blake3_upstream.py   (~1 s; needs the ROCm LLVM libraries)
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)

import blake3_cases as cases  # noqa: E402
import blake3_upstream as up  # noqa: E402

MAX_BYTES = 160 << 10


def build():
    out = {"generator": "tests/golden/make_blake3_upstream.py (upstream BLAKE3 C code, llvm_blake3_* of ROCm's LLVM)",
           "blake3_version": up.version(), "sources": {}}
    for group, src, cs in (("small", cases.small_source(), cases.small_cases()),
                           ("tree", cases.tree_source(), cases.tree_cases())):
        out["sources"][group] = {"sha256": hashlib.sha256(src.tobytes()).hexdigest(), "cases": len(cs)}
        out[group] = "".join(up.hash(src[off:off + n]).hex() for off, n in cs)
    return json.dumps(out, indent=1, sort_keys=True) + "\n"


def main():
    if not up.available():
        sys.exit("no library exporting llvm_blake3_hasher_init under $ROCM_PATH or /opt/rocm")
    text = build()
    assert len(text) < MAX_BYTES, len(text)
    path = os.path.join(HERE, "blake3_upstream.json")
    with open(path, "w") as f:
        f.write(text)
    print("wrote %s (%d bytes, BLAKE3 %s)" % (path, len(text), up.version()), file=sys.stderr)


if __name__ == "__main__":
    main()
