"""A literal Python restatement of dir_unpacker.rs (unpack, restore_file, fetch_full_tree, fetch_tree)
over oracle/pack_oracle.get_blob and tests/zstd_ref.py.  A helper, not a test: the GPU restore is
compared with what this returns over the same packfiles.

Store: packs = [(packfile id, bytes)], index = [(hash, packfile id)] in BlobIndex.items order.
Manager::get_blob (unpack.rs:23-83): find_packfile by hash, open that packfile, scan its header,
open the blob, decompress.  Results are cached per hash: the store does not change under a test."""
import struct

import zstd_ref
from oracle import pack_oracle as po

KIND_FILE, KIND_DIR = 0, 1
OK, ETAG, EZSTD, EDIGEST, ERANGE = 0, 1, 2, 3, 4
ENOTFOUND, EMISMATCH, ENOPACKFILE, ENOTTREE, EFORMAT = 16, 17, 18, 19, 20


class RestoreError(Exception):
    def __init__(self, reason, blob_hash):
        super().__init__("%d %s" % (reason, bytes(blob_hash).hex()))
        self.reason, self.hash = reason, bytes(blob_hash)


class Tree:
    def __init__(self, kind, name, size, mtime, ctime, children, next_sibling):
        self.kind, self.name, self.size, self.mtime, self.ctime = kind, name, size, mtime, ctime
        self.children, self.next_sibling = children, next_sibling


def deserialize_tree(buf):
    """bincode::deserialize::<Tree> (bincode 1.3.3's legacy free function: fixint little endian, u32
    enum tag, u64 lengths, one-byte Option tags, trailing bytes allowed).  Raises ValueError."""
    buf = bytes(buf)
    at = 0

    def take(n):
        nonlocal at
        if n > len(buf) - at:
            raise ValueError("unexpected end")
        at += n
        return buf[at - n:at]

    def option(read):
        tag = take(1)[0]
        if tag > 1:
            raise ValueError("Option tag %d" % tag)
        return read() if tag else None

    def u64():
        return struct.unpack("<Q", take(8))[0]

    kind = struct.unpack("<I", take(4))[0]
    if kind > 1:
        raise ValueError("TreeKind tag %d" % kind)
    name = take(u64()).decode("utf-8")  # strict: String::from_utf8
    size, mtime, ctime = option(u64), option(u64), option(u64)
    n = u64()
    if n > (len(buf) - at) // 32:
        raise ValueError("children run past the blob")
    children = [take(32) for _ in range(n)]
    return Tree(kind, name, size, mtime, ctime, children, option(lambda: take(32)))


class Store:
    def __init__(self, prk, packs, index, verify=False):
        self.prk, self.packs, self.verify = prk, dict(packs), verify
        self.where = {}
        for h, pid in index:  # a hash held twice may resolve to any of its items
            self.where.setdefault(bytes(h), bytes(pid))
        self.cache = {}

    def get_blob(self, h):
        """-> (status, kind, data): status OK with the blob, or the code the device reports."""
        h = bytes(h)
        if h not in self.cache:
            self.cache[h] = self._get_blob(h)
        return self.cache[h]

    def _get_blob(self, h):
        pid = self.where.get(h)
        if pid is None:
            return ENOTFOUND, None, None
        if pid not in self.packs:
            return ENOPACKFILE, None, None
        try:
            kind, payload = po.get_blob(self.prk, pid, self.packs[pid], h)
        except po.CryptoError:
            return ETAG, None, None
        except po.FormatError as e:
            assert "IndexHeaderMismatch" in str(e), e
            return EMISMATCH, None, None
        try:
            data = zstd_ref.decompress(payload)
        except ValueError:
            return EZSTD, None, None
        if self.verify:
            from oracle import oracle
            if oracle.blake3(data) != h:
                return EDIGEST, None, None
        return OK, kind, data


def fetch_tree(store, h):
    st, kind, data = store.get_blob(h)
    if st:
        raise RestoreError(st, h)
    if kind != po.KIND_TREE:
        raise RestoreError(ENOTTREE, h)
    try:
        return deserialize_tree(data)
    except ValueError:
        raise RestoreError(EFORMAT, h)


def fetch_full_tree(store, h, max_pieces=None):
    root = fetch_tree(store, h)
    nxt, pieces = root.next_sibling, 1
    while nxt is not None:
        if max_pieces is not None and pieces > max_pieces:  # the reference spins; the device refuses
            raise RestoreError(EFORMAT, nxt)
        part = fetch_tree(store, nxt)
        root.children = root.children + part.children
        nxt, pieces = part.next_sibling, pieces + 1
    return root


def restore_file(store, tree):
    """-> (bytes written, status, bad child): restore_file writes chunk by chunk and bails at the
    first that fails, leaving the partial file."""
    out = []
    for k, h in enumerate(tree.children):
        st, _, data = store.get_blob(h)
        if st:
            return b"".join(out), st, k
        out.append(data)
    return b"".join(out), OK, None


def unpack(store, root_hash, max_pieces=None, max_nodes=1 << 20):
    """-> (nodes, files, errors).  nodes: [dict(kind, name, size, mtime, ctime, parent, path, children)]
    in the reference's visiting order (node 0 the root; the children of each Dir consecutive, parents
    in node order); files: {path: bytes}; errors: {path: (status, bad child)}."""
    root = fetch_full_tree(store, root_hash, max_pieces)
    nodes = [dict(tree=root, parent=None, path="", hash=bytes(root_hash))]
    files, errors = {}, {}
    queue = [0]
    while queue:
        p = queue.pop(0)
        parent = nodes[p]["tree"]
        if parent.kind != KIND_DIR:
            continue
        for h in parent.children:
            a = p
            while a is not None:  # a directory that contains itself: the reference never ends
                if nodes[a]["hash"] == bytes(h):
                    raise RestoreError(EFORMAT, h)
                a = nodes[a]["parent"]
            child = fetch_full_tree(store, h, max_pieces)
            path = (nodes[p]["path"] + "/" if nodes[p]["path"] else "") + child.name
            nodes.append(dict(tree=child, parent=p, path=path, hash=bytes(h)))
            assert len(nodes) <= max_nodes
            if child.kind == KIND_FILE:
                data, st, bad = restore_file(store, child)
                files[path] = data
                if st:
                    errors[path] = (st, bad)
            else:
                queue.append(len(nodes) - 1)
    return nodes, files, errors
