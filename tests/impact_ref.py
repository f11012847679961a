"""A plain Python restatement of impact (include/backuwup_gpu_pack.h, "impact") over tests/restore_ref.py's
Store and tests/prune_ref.py's headers_of / Locator / open_entry.  A helper, not a test: the GPU mark and
report walk are compared with what this returns over the same packfiles.  The reference cannot ask the
question, so the rules are the header's; the fixed point is a naive "repeat until nothing changes" over
sets, the report a recursive descent."""
from collections import Counter

import prune_ref as pr
import restore_ref as rr
from oracle import pack_oracle as po

SELF, BELOW = 1, 2
UNREADABLE, TRUNCATED, CYCLIC = 1, 2, 4
NONE = 2**64 - 1
ZERO = bytes(32)


def _open_tree(store, headers, ent):
    """(status, Tree) of a Tree entry through the unpack chain and the parser."""
    p, h, _, _, length, offset = ent
    if not pr.range_ok(headers[p][1], headers[p][2], offset, length):
        return rr.ERANGE, None
    st, _, data = pr.open_entry(store, headers, ent)
    if st:
        return st, None
    try:
        return rr.OK, rr.deserialize_tree(data)
    except ValueError:
        return rr.EFORMAT, None


def mark(store, headers, roots, bad=None):
    """-> (taint list, one int per entry; root_affected list; errors Counter of (hash, parent, child_pos,
    reason); info dict(n_trees_expanded, n_levels, n_edges, n_sweeps, n_tainted, n_roots_affected))."""
    locate = pr.Locator(store, headers)
    ents = pr.flat_entries(headers)
    bad = [0] * len(ents) if bad is None else [int(b) for b in bad]
    reached, queued, selfs, below, errors = set(), set(), set(), set(), Counter()
    levels = []  # per level the edges (parent entry, child entry, SELF only) its expansions appended

    def visit(h, tree_ref, parent_hash, pos, nxt, parent_e, edges):
        st, e = locate(h)
        if st:
            errors[(bytes(h), parent_hash, pos, st)] += 1
            if parent_e is not None:
                below.add(parent_e)
            return
        p, eh, kind, _, length, offset = ents[e]
        tree = kind == po.KIND_TREE
        lost = bool(bad[e])
        range_bad = not tree and not pr.range_ok(headers[p][1], headers[p][2], offset, length)
        first = e not in reached
        reached.add(e)
        if lost or range_bad:
            selfs.add(e)
        affected = False
        if tree_ref and not tree:
            errors[(bytes(h), parent_hash, pos, rr.ENOTTREE)] += 1
            affected = True
        if range_bad and first:
            errors[(eh, ZERO, NONE, rr.ERANGE)] += 1
        if not tree and (lost or range_bad):
            affected = True
        if parent_e is not None:
            if tree:
                edges.append((parent_e, e, not tree_ref))
            if affected:
                below.add(parent_e)
        if tree_ref and tree and not lost and e not in queued:  # a lost tree blob is never opened
            queued.add(e)
            nxt.append(e)

    front = []
    for i, r in enumerate(roots):
        visit(r, True, ZERO, i, front, None, None)
    expanded = 0
    while front:
        nxt, edges = [], []
        for e in front:
            h = ents[e][1]
            st, t = _open_tree(store, headers, ents[e])
            if st:
                errors[(h, ZERO, NONE, st)] += 1
                selfs.add(e)
                continue
            expanded += 1
            for k, c in enumerate(t.children):
                visit(c, t.kind == rr.KIND_DIR, h, k, nxt, e, edges)
            if t.next_sibling is not None:
                visit(t.next_sibling, True, h, NONE, nxt, e, edges)
        levels.append(edges)
        front = nxt

    # BELOW: repeat until nothing changes; a sweep takes the levels latest first
    sweeps, changed = 0, True
    while changed:
        changed = False
        sweeps += 1
        for edges in reversed(levels):
            for parent, child, self_only in edges:
                hit = child in selfs or (not self_only and child in below)
                if hit and parent not in below:
                    below.add(parent)
                    changed = True
    taint = [0] * len(ents)
    for e in reached:
        taint[e] = (SELF if e in selfs else 0) | (BELOW if e in below else 0)
    assert not (selfs - reached) and not (below - reached)
    affected = [int(tree_ref_affected(locate, ents, taint, r)) for r in roots]
    info = dict(n_trees_expanded=expanded, n_levels=len(levels), n_edges=sum(len(x) for x in levels), n_sweeps=sweeps,
                n_tainted=sum(1 for t in taint if t), n_roots_affected=sum(affected))
    return taint, affected, errors, info


def tree_ref_affected(locate, ents, taint, h):
    st, e = locate(h)
    return bool(st) or ents[e][2] != po.KIND_TREE or bool(taint[e] & (SELF | BELOW))


def paths(store, headers, roots, taint):
    """-> (records, per_root, errors Counter).  records: [dict(level, root, parent, path, hash, name, kind,
    meta_flags, size, mtime, ctime, n_children, n_affected, first_affected, flags)], parent an index into
    records (None for a root), path the tuple of names from the root (b'?' + hash for an unreadable item);
    per_root: [dict(n_records, n_files, n_unreadable, lost_chunk_refs)]."""
    locate = pr.Locator(store, headers)
    ents = pr.flat_entries(headers)
    n_e = len(ents)
    records, errors = [], Counter()
    per_root = [dict(n_records=0, n_files=0, n_unreadable=0, lost_chunk_refs=0) for _ in roots]

    def piece(h, by, pos):
        """One tree reference opened: (Tree or None, whether an error was recorded)."""
        st, e = locate(h)
        if st:
            errors[(bytes(h), by, pos, st)] += 1
            return None
        if ents[e][2] != po.KIND_TREE:
            errors[(bytes(h), by, pos, rr.ENOTTREE)] += 1
            return None
        if taint[e] & SELF:  # never opened, and no error of this walk
            return None
        st, t = _open_tree(store, headers, ents[e])
        if st:
            errors[(bytes(h), by, pos, st)] += 1
            return None
        return t

    def item(root, parent, h, by, pos, ancestors, level, path):
        h = bytes(h)
        rec = dict(level=level, root=root, parent=parent, hash=h, name=b"", kind=0, meta_flags=0, size=0, mtime=0, ctime=0,
                   n_children=0, n_affected=0, first_affected=NONE, flags=0)
        me = len(records)
        records.append(rec)
        per_root[root]["n_records"] += 1
        cyclic = h in ancestors
        if cyclic:
            errors[(h, by, pos, rr.EFORMAT)] += 1
            rec["flags"] |= CYCLIC
        t = piece(h, by, pos)
        if t is None:
            rec["flags"] |= UNREADABLE
            rec["path"] = path + (b"?" + h,)
            per_root[root]["n_unreadable"] += 1
            return
        name = t.name.encode()
        rec.update(name=name, kind=t.kind, size=t.size or 0, mtime=t.mtime or 0, ctime=t.ctime or 0, path=path + (name,),
                   meta_flags=(1 if t.size is not None else 0) | (2 if t.mtime is not None else 0) | (4 if t.ctime is not None else 0))
        rows = []  # (hash, the piece that holds it, its position there)
        if not cyclic:
            cur, cur_hash, rnd = t, h, 1
            rows += [(c, cur_hash, k) for k, c in enumerate(cur.children)]
            while cur.next_sibling is not None:
                nh = bytes(cur.next_sibling)
                if rnd > n_e:  # a chain of more pieces than the store has entries is refused unread
                    errors[(nh, cur_hash, NONE, rr.EFORMAT)] += 1
                    nxt = None
                else:
                    nxt = piece(nh, cur_hash, NONE)
                if nxt is None:
                    rec["flags"] |= TRUNCATED
                    break
                cur, cur_hash, rnd = nxt, nh, rnd + 1
                rows += [(c, cur_hash, k) for k, c in enumerate(cur.children)]
        rec["n_children"] = len(rows)
        hit = []
        for k, (c, by2, pos2) in enumerate(rows):
            if t.kind == rr.KIND_DIR:
                aff = tree_ref_affected(locate, ents, taint, c)
            else:
                st, e = locate(c)
                aff = bool(st) or bool(taint[e] & SELF)
            if aff:
                hit.append((c, by2, pos2))
                rec["first_affected"] = min(rec["first_affected"], k)
        rec["n_affected"] = len(hit)
        if t.kind == rr.KIND_DIR:
            for c, by2, pos2 in hit:
                item(root, me, c, by2, pos2, ancestors | {h}, level + 1, rec["path"])
        else:
            per_root[root]["n_files"] += 1
            per_root[root]["lost_chunk_refs"] += len(hit)

    for i, r in enumerate(roots):
        if tree_ref_affected(locate, ents, taint, r):
            item(i, None, r, ZERO, i, frozenset(), 0, ())
    return records, per_root, errors


FIELDS = ("level", "root", "path", "hash", "name", "kind", "meta_flags", "size", "mtime", "ctime", "n_children", "n_affected",
          "first_affected", "flags")


def resolve(records):
    """The records as a Counter of tuples in FIELDS order: what the device's records are compared by."""
    return Counter(tuple(r[f] for f in FIELDS) for r in records)


def file_paths(records, root):
    """The affected File paths under one root, '/'-joined below the root's own name, sorted."""
    return sorted(b"/".join(r["path"][1:]).decode() for r in records
                  if r["root"] == root and not r["flags"] & UNREADABLE and r["kind"] == rr.KIND_FILE)
