"""Small stores for the restore tests, written by the oracle's write side (oracle.fastcdc,
oracle.split_serialize_tree, pack_oracle.write_packfiles).  A helper, not a test."""
import numpy as np

from oracle import oracle
from oracle import pack_oracle as po

PRK = bytes.fromhex("a7" * 32)
CDC = (64, 256, 1024)  # small FastCDC parameters: files of a few KiB have several chunks


class Builder:
    """Blobs in add order -> packfiles and index items.  payload= stores other bytes than the store
    frame of `data` under the hash (damage, forgeries); blob_hash= names the blob freely (headers
    written by pack_oracle accept any hash)."""

    def __init__(self, prk=PRK, seed=1):
        self.prk, self.rng = prk, np.random.default_rng(seed)
        self.blobs, self.seen = [], set()

    def add(self, data, kind=po.KIND_FILE_CHUNK, blob_hash=None, payload=None, again=False):
        h = bytes(blob_hash) if blob_hash is not None else oracle.blake3(data)
        if h in self.seen and not again:
            return h
        self.seen.add(h)
        nonce = bytes(self.rng.integers(0, 256, 12, dtype=np.uint8))
        pl = po.zstd_store(data) if payload is None else bytes(payload)
        self.blobs.append((h, kind, nonce, po.seal_blob_payload(self.prk, h, nonce, pl)))
        return h

    def add_tree(self, kind, name, size, mtime, ctime, children):
        """split_serialize_tree + add_tree_to_blobs: every piece a Tree blob; the first piece's hash."""
        pieces = oracle.split_serialize_tree(kind, name, size, mtime, ctime, b"".join(children))
        for data, h in pieces:
            self.add(data, po.KIND_TREE, blob_hash=h)
        return pieces[0][1]

    def add_raw_tree(self, data, blob_hash=None):
        return self.add(data, po.KIND_TREE, blob_hash=blob_hash)

    def add_file(self, name, data, mtime=None):
        chunks = [self.add(data[o:o + n]) for _, o, n in oracle.fastcdc(data, *CDC)] if data else []
        return self.add_tree(0, name, len(data), mtime, None, chunks)

    def add_dir(self, name, spec, mtime=None):
        """spec: {name: bytes | dict}, children in dict order."""
        kids = [self.add_dir(k, v, mtime) if isinstance(v, dict) else self.add_file(k, v, mtime) for k, v in spec.items()]
        return self.add_tree(1, name, None, mtime, None, kids)

    def finish(self, target=None):
        """-> (packs [(id, bytes)], index [(hash, id)]).  target: blobs per packfile (None: the
        reference's 3 MiB grouping)."""
        n = len(self.blobs)
        if target is None:
            groups = po.plan_packfiles([len(b[3]) for b in self.blobs])
        else:
            groups = [(f, min(target, n - f)) for f in range(0, n, target)]
        ids = [bytes(self.rng.integers(0, 256, 12, dtype=np.uint8)) for _ in groups]
        packs = [(ids[g], po.serialize_packfile(self.prk, ids[g], self.blobs[f:f + c])) for g, (f, c) in enumerate(groups)]
        index = [(self.blobs[i][0], ids[g]) for g, (f, c) in enumerate(groups) for i in range(f, f + c)]
        return packs, index


def flatten(spec, prefix=""):
    """{relative path: bytes} of a directory spec."""
    out = {}
    for k, v in spec.items():
        p = prefix + "/" + k if prefix else k
        if isinstance(v, dict):
            out.update(flatten(v, p))
        else:
            out[p] = v
    return out


def items_array(index):
    return np.frombuffer(b"".join(h + pid for h, pid in index), dtype=np.uint8).reshape(-1, 44) if index \
        else np.zeros((0, 44), dtype=np.uint8)
