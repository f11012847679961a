"""Restore without a GPU: the reference restatement (tests/restore_ref.py) round-trips the oracle's
write side, its bincode deserializer reads the hand-derived literals of test_tree.py, and the new
entry points check their arguments on the host."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zstd_ref  # noqa: E402

needs_zstd = pytest.mark.skipif(not zstd_ref.available(), reason="system libzstd not found")


def _spec():
    rng = np.random.default_rng(5)
    blob = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    shared = blob(3000)
    return {"a.bin": blob(5000), "empty": b"", "sub": {"deep": {"x": blob(1), "y": shared, "none": b""}, "z.txt": blob(2500)},
            "copy": shared, "été — 日本.txt": blob(700), "emptydir": {}}


@needs_zstd
def test_round_trip_against_the_oracles_write_side(oracle):
    import restore_ref
    import restore_store
    spec = _spec()
    b = restore_store.Builder()
    root = b.add_dir("", spec, mtime=1_600_000_000)
    packs, index = b.finish(target=7)
    assert len(packs) > 3
    nodes, files, errors = restore_ref.unpack(restore_ref.Store(restore_store.PRK, packs, index), root)
    assert not errors
    assert files == restore_store.flatten(spec)
    assert len(files["a.bin"]) == 5000 and len(nodes[1]["tree"].children) > 3  # several chunks
    # the visiting order: the root, its children in order, then the children of "sub", then of "deep"
    assert [n["path"] for n in nodes] == ["", "a.bin", "empty", "sub", "copy", "été — 日本.txt", "emptydir", "sub/deep",
                                          "sub/z.txt", "sub/deep/x", "sub/deep/y", "sub/deep/none"]
    assert all(n["tree"].mtime == 1_600_000_000 for n in nodes)


def test_deserializer_on_the_hand_derived_literals():
    import restore_ref
    lit = bytes.fromhex("00000000" "0100000000000000" "61" "01" "0300000000000000" "00" "01" "0500000000000000"
                        "0100000000000000") + bytes(range(32)) + b"\x00"
    t = restore_ref.deserialize_tree(lit)
    assert (t.kind, t.name, t.size, t.mtime, t.ctime, t.children, t.next_sibling) == \
        (0, "a", 3, None, 5, [bytes(range(32))], None)
    sib = bytes(range(100, 132))
    lit2 = struct.pack("<IQ", 1, 3) + b"dir" + b"\x00\x00\x00" + struct.pack("<Q", 0) + b"\x01" + sib
    t = restore_ref.deserialize_tree(lit2)
    assert (t.kind, t.name, t.size, t.mtime, t.ctime, t.children, t.next_sibling) == (1, "dir", None, None, None, [], sib)
    assert restore_ref.deserialize_tree(lit + b"trailing").name == "a"  # allow_trailing_bytes
    for k in range(len(lit)):
        with pytest.raises(ValueError):
            restore_ref.deserialize_tree(lit[:k])
    for bad in (b"\x02" + lit[1:], lit[:13] + b"\x02" + lit[14:], lit[:4] + struct.pack("<Q", 2**63) + lit[12:],
                lit[:12] + b"\xc0" + lit[13:]):
        with pytest.raises(ValueError):
            restore_ref.deserialize_tree(bad)


def test_deserializer_inverts_the_library_serializer():
    import restore_ref
    from backuwup_amd.context import make_tree, tree_serialize
    sib = bytes(range(7, 39))
    for name in ("", "x" * 300, "été — 日本.txt", "\U0001f600"):
        for meta in ((None, None, None), (1, None, 2**63), (0, 2**64 - 1, None)):
            ch = bytes(range(64))
            t = restore_ref.deserialize_tree(tree_serialize(make_tree(1, name, *meta, ch), next_sibling=sib))
            assert (t.kind, t.name, t.size, t.mtime, t.ctime, b"".join(t.children), t.next_sibling) == (1, name, *meta, ch, sib)


def test_new_entry_points_check_their_arguments_on_the_host():
    from backuwup_amd import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    prk = (ctypes.c_uint8 * 32)()
    assert L.bw_restore_open(None, prk, None, None, None, 0, None, 0, None, 0, 0, ctypes.byref(h)) == _lib.BW_EINVAL
    assert L.bw_restore_open_host(None, prk, None, None, None, 0, None, 0, None, 0, 0, ctypes.byref(h)) == _lib.BW_EINVAL
    assert L.bw_restore_close(None) == _lib.BW_EINVAL
    assert L.bw_restore_locate(None, None, 0, None, None) == _lib.BW_EINVAL
    cnt, err, done = _lib.BwRestoreCounts(), _lib.BwRestoreError(), ctypes.c_uint64()
    assert L.bw_restore_trees(None, prk, 0, None, 0, None, 0, None, 0, ctypes.byref(cnt), ctypes.byref(err)) == _lib.BW_EINVAL
    for fn in (L.bw_restore_files_device, L.bw_restore_files):
        assert fn(None, None, None, 0, 0, None, 0, None, None, None, None, ctypes.byref(done)) == _lib.BW_EINVAL
    # the mirrors' layouts against the header
    from backuwup_amd import restore
    assert ctypes.sizeof(_lib.BwRestoreNode) == restore.NODE_DTYPE.itemsize == 72
    assert ctypes.sizeof(_lib.BwRestoreCounts) == 24 and ctypes.sizeof(_lib.BwRestoreError) == 40
    assert {_lib.BW_RESTORE_ENOTFOUND, _lib.BW_RESTORE_EMISMATCH, _lib.BW_RESTORE_ENOPACKFILE, _lib.BW_RESTORE_ENOTTREE,
            _lib.BW_RESTORE_EFORMAT}.isdisjoint({_lib.BW_UNPACK_OK, _lib.BW_UNPACK_ETAG, _lib.BW_UNPACK_EZSTD,
                                                 _lib.BW_UNPACK_EDIGEST, _lib.BW_UNPACK_ERANGE})


def test_restore_struct_layout_matches_header(tmp_path):
    import subprocess
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "backuwup_gpu.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(bw_restore_node),'
                   ' offsetof(bw_restore_node, parent), offsetof(bw_restore_node, name_len), sizeof(bw_restore_counts),'
                   ' sizeof(bw_restore_error), BW_RESTORE_ENOTFOUND, BW_RESTORE_EFORMAT); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)])
    from backuwup_amd import _lib
    vals = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert vals == [ctypes.sizeof(_lib.BwRestoreNode), _lib.BwRestoreNode.parent.offset, _lib.BwRestoreNode.name_len.offset,
                    ctypes.sizeof(_lib.BwRestoreCounts), ctypes.sizeof(_lib.BwRestoreError), _lib.BW_RESTORE_ENOTFOUND,
                    _lib.BW_RESTORE_EFORMAT]
