"""A plain Python restatement of prune (include/backuwup_gpu_pack.h, "prune") over tests/restore_ref.py's
Store and oracle/pack_oracle.py.  A helper, not a test: the GPU mark and repack are compared with what
this returns over the same packfiles.  The reference has no prune, so the rules are the header's:

  - a reference is located as Manager::get_blob finds a blob: the index's first item for the hash, then
    the first entry of that packfile's header with the hash;
  - the walk is breadth first over tree references (a root, a child of a Dir piece, a next_sibling);
    every located reference marks its entry live, a tree reference to a Tree entry also queues it, once;
  - the children of a File piece are marked whatever their kind and never opened;
  - errors are collected, never raised."""
import struct
from collections import Counter

import restore_ref as rr
from oracle import oracle
from oracle import pack_oracle as po

NONE = 2**64 - 1
ZERO = bytes(32)


def headers_of(prk, packs):
    """[(packfile id, size, header_len, [(hash, kind, compression, length, offset)])] in packs order."""
    out = []
    for pid, buf in packs:
        hl = struct.unpack_from("<Q", buf, 0)[0]
        pt = oracle.open_blob(prk, b"header", bytes(pid), bytes(buf[8:8 + hl]))
        assert pt is not None
        out.append((bytes(pid), len(buf), hl, po.deserialize_header(pt)))
    return out


def flat_entries(headers):
    """[(packfile position, hash, kind, compression, length, offset)] in entry-index order."""
    return [(p,) + tuple(e) for p, (_, _, _, ents) in enumerate(headers) for e in ents]


def range_ok(size, header_len, offset, length):
    base = 8 + header_len
    return base <= size and offset <= size - base and 12 <= size - base - offset and \
        length <= size - base - offset - 12 and length >= 16


class Locator:
    def __init__(self, store, headers):
        self.store = store
        self.pos = {}
        for p, (pid, _, _, _) in enumerate(headers):
            self.pos.setdefault(pid, p)
        self.first = {}
        e = 0
        for p, (_, _, _, ents) in enumerate(headers):
            for ent in ents:
                self.first.setdefault((p, ent[0]), e)
                e += 1

    def __call__(self, h):
        """-> (status, entry index)"""
        pid = self.store.where.get(bytes(h))
        if pid is None:
            return rr.ENOTFOUND, None
        if pid not in self.pos:
            return rr.ENOPACKFILE, None
        e = self.first.get((self.pos[pid], bytes(h)))
        return (rr.EMISMATCH, None) if e is None else (rr.OK, e)


def mark(store, headers, roots):
    """-> (live set of entry indices, errors Counter of (hash, parent, child_pos, reason), info) with
    info = dict(n_trees_expanded, n_levels, stats [(live blobs, live bytes, blobs, bytes)] per packfile)."""
    locate = Locator(store, headers)
    ents = flat_entries(headers)
    live, queued, errors = set(), set(), Counter()

    def visit(h, tree_ref, parent, pos, nxt):
        st, e = locate(h)
        if st:
            errors[(bytes(h), parent, pos, st)] += 1
            return
        p, eh, kind, _, length, offset = ents[e]
        tree = kind == po.KIND_TREE
        if tree_ref and not tree:
            errors[(bytes(h), parent, pos, rr.ENOTTREE)] += 1
        if e not in live:
            live.add(e)
            if not tree and not range_ok(headers[p][1], headers[p][2], offset, length):
                errors[(eh, ZERO, NONE, rr.ERANGE)] += 1
        if tree_ref and tree and e not in queued:  # the two bits: marked is not queued
            queued.add(e)
            nxt.append(e)

    front = []
    for i, r in enumerate(roots):
        visit(r, True, ZERO, i, front)
    expanded = levels = 0
    while front:
        levels += 1
        nxt = []
        for e in front:
            p, h, _, _, length, offset = ents[e]
            if not range_ok(headers[p][1], headers[p][2], offset, length):
                errors[(h, ZERO, NONE, rr.ERANGE)] += 1
                continue
            st, _, data = open_entry(store, headers, ents[e])
            if st:
                errors[(h, ZERO, NONE, st)] += 1
                continue
            try:
                t = rr.deserialize_tree(data)
            except ValueError:
                errors[(h, ZERO, NONE, rr.EFORMAT)] += 1
                continue
            expanded += 1
            for k, c in enumerate(t.children):
                visit(c, t.kind == rr.KIND_DIR, h, k, nxt)
            if t.next_sibling is not None:
                visit(t.next_sibling, True, h, NONE, nxt)
        front = nxt
    stats = [[0, 0, 0, 0] for _ in headers]
    for e, (p, _, _, _, length, _) in enumerate(ents):
        stats[p][2] += 1
        stats[p][3] += 12 + length
        if e in live:
            stats[p][0] += 1
            stats[p][1] += 12 + length
    return live, errors, dict(n_trees_expanded=expanded, n_levels=levels, stats=[tuple(s) for s in stats])


def open_entry(store, headers, ent):
    """The unpack chain for one entry: (status, kind, data)."""
    import zstd_ref
    p, h, kind, _, length, offset = ent
    buf = store.packs[headers[p][0]]
    at = 8 + headers[p][2] + offset
    payload = oracle.open_blob(store.prk, h, bytes(buf[at:at + 12]), bytes(buf[at + 12:at + 12 + length]))
    if payload is None:
        return rr.ETAG, None, None
    try:
        data = zstd_ref.decompress(payload)
    except ValueError:
        return rr.EZSTD, None, None
    if store.verify and oracle.blake3(data) != h:
        return rr.EDIGEST, None, None
    return rr.OK, kind, data


def serialize_packfile(prk, packfile_id, blobs):
    """pack_oracle.serialize_packfile for blobs [(hash, kind, compression, nonce, sealed)]: the stored
    compression tag is kept."""
    entries, data, written = [], [], 0
    for h, kind, comp, nonce, sealed in blobs:
        entries.append((h, kind, comp, len(sealed), written))
        written += len(sealed) + po.BLOB_NONCE_SIZE
        data.append(bytes(nonce) + bytes(sealed))
    header = oracle.seal_blob(prk, b"header", bytes(packfile_id), po.serialize_header(entries))
    buf = struct.pack("<Q", len(header)) + header + b"".join(data)
    assert len(buf) <= po.PACKFILE_MAX_SIZE
    return buf


def order_of(headers, live, rewrite):
    """The live entries of the rewritten packfiles, ascending by packfile position, then by entry index."""
    return [e for e, ent in enumerate(flat_entries(headers)) if e in live and rewrite[ent[0]]]


def repack(prk, packs, headers, live, rewrite, new_ids):
    """-> (new packs [(id, bytes)], moved index items [(hash, new id)], order, groups [(first, count)])."""
    ents = flat_entries(headers)
    order = order_of(headers, live, rewrite)
    blobs = []
    for e in order:
        p, h, kind, comp, length, offset = ents[e]
        assert range_ok(headers[p][1], headers[p][2], offset, length)
        at = 8 + headers[p][2] + offset
        buf = packs[p][1]
        blobs.append((h, kind, comp, buf[at:at + 12], buf[at + 12:at + 12 + length]))
    groups = po.plan_packfiles([len(b[4]) for b in blobs])
    new = [(bytes(new_ids[g]), serialize_packfile(prk, new_ids[g], blobs[f:f + c])) for g, (f, c) in enumerate(groups)]
    items = [(blobs[i][0], bytes(new_ids[g])) for g, (f, c) in enumerate(groups) for i in range(f, f + c)]
    return new, items, order, groups


def entries_array(headers):
    """The headers as bw_unpack_headers returns them (UNPACK_ENTRY_DTYPE)."""
    import numpy as np
    from backuwup_amd.context import UNPACK_ENTRY_DTYPE
    ents = flat_entries(headers)
    out = np.zeros(len(ents), dtype=UNPACK_ENTRY_DTYPE)
    for k, (p, h, kind, comp, length, offset) in enumerate(ents):
        out[k]["hash"] = np.frombuffer(h, dtype=np.uint8)
        out[k]["packfile"], out[k]["kind"], out[k]["compression"] = p, kind, comp
        out[k]["length"], out[k]["offset"] = length, offset
    return out
