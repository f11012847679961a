"""The parent match, stated in plain Python over tests/restore_ref.py's Store, tests/prune_ref.py's
locator and tests/diff_ref.py's rule for one reference: which nodes of a stat-only scan are the parent
snapshot's as they stand.  A helper, not a test; tests/test_parent.py pins it against hand-written
expectations, tests/test_gpu_parent_match.py holds bw_parent_match equal to it.

The scan is a list of dicts (kind, flags, size, mtime, ctime, child_first, n_children, name bytes):
node 0 is the root, a Dir's children are the nodes [child_first, child_first + n_children), a File has
none.  Every node gets (status, hash); hash is the parent snapshot's child hash, zero for NEW.

  1. Level 0 is the item (scan node 0, parent_root); the roots pair whatever their names.  parent_root
     None: everything NEW, nothing read, no level.  The root's first piece unreadable: NEW and an error.
  2. A pair (scan node, parent tree): kinds differ -> TYPE_CHANGED, and nothing below is matched.  Dir
     against Dir -> DIR, an item of the next level.  File against File -> UNCHANGED when the flags are
     equal and hold HAS_SIZE and HAS_MTIME, size and mtime are equal, ctime is equal where flagged, and
     mtime < trust_before; RACY when only the last fails; CHANGED otherwise.
  3. For an item (scan Dir, hash) the hash's whole next_sibling chain is read and its children rows are
     concatenated in chain order.  A later piece that cannot be read ends the list there, with an error;
     so does a chain of more pieces than the store has entries (EFORMAT).
  4. Of every row the first piece only is read, for its name, kind and metadata; a File's later pieces
     are never opened.  A row that cannot be located, opened, decoded or parsed, or that is a FileChunk,
     gives an error and takes no part in the join.
  5. The join key is (item, name bytes), compared whole.  Among the readable rows of one item with equal
     names the lowest position answers.  Every scan child of the Dir asks; scan children with equal
     names get the same answer; no answer is NEW.  Parent rows nobody asks for are not descended.
  6. Errors are diff_ref's records: (hash, the piece that names it or zero for the root, its position
     there or ~0 for a next_sibling or 0 for the root, reason).
  7. read = the entries opened; n_levels = the levels that hold an item (level 0 holds the roots'
     whatever becomes of it); n_unchanged and unchanged_bytes count the UNCHANGED nodes and their sizes."""
import diff_ref
import restore_ref as rr

NONE = 2**64 - 1
ZERO = bytes(32)
NEW, UNCHANGED, CHANGED, RACY, DIR, TYPE_CHANGED = range(6)
HAS_SIZE, HAS_MTIME, HAS_CTIME = 1, 2, 4


def tree_flags(t):
    return (HAS_SIZE if t.size is not None else 0) | (HAS_MTIME if t.mtime is not None else 0) | \
        (HAS_CTIME if t.ctime is not None else 0)


def verdict(sn, t, trust_before):
    """Rule 2."""
    if sn["kind"] != t.kind:
        return TYPE_CHANGED
    if sn["kind"] == rr.KIND_DIR:
        return DIR
    need = HAS_SIZE | HAS_MTIME
    same = sn["flags"] == tree_flags(t) and sn["flags"] & need == need and sn["size"] == t.size and sn["mtime"] == t.mtime
    if same and sn["flags"] & HAS_CTIME:
        same = sn["ctime"] == t.ctime
    if not same:
        return CHANGED
    return UNCHANGED if sn["mtime"] < trust_before else RACY


def match(store, headers, parent_root, scan, trust_before=NONE):
    """-> (results [(status, hash)] per scan node, errors Counter, read set of entry indices, n_levels,
    n_unchanged, unchanged_bytes)."""
    w = diff_ref.Walk(store, headers)               # piece(): rule 6, and the read set
    res = [(NEW, ZERO)] * len(scan)

    def done(levels):
        unch = [sn["size"] for sn, (st, _) in zip(scan, res) if st == UNCHANGED]
        return res, w.errors, w.read, levels, len(unch), sum(unch)

    if parent_root is None:
        return done(0)
    items = []
    t = w.piece(parent_root, ZERO, 0)
    if t is not None:
        res[0] = (verdict(scan[0], t, trust_before), bytes(parent_root))
        if res[0][0] == DIR:
            items.append((0, bytes(parent_root), t))
    levels = 1
    while True:
        nxt = []
        for s, h, t in items:
            rows, piece_hash, pieces = [], h, 1     # rule 3
            while True:
                rows += [(c, piece_hash, k) for k, c in enumerate(t.children)]
                sib = t.next_sibling
                if sib is None:
                    break
                if pieces > len(w.ents):
                    w.errors[(sib, piece_hash, NONE, rr.EFORMAT)] += 1
                    break
                t = w.piece(sib, piece_hash, NONE)
                if t is None:
                    break
                piece_hash, pieces = sib, pieces + 1
            table = {}                               # rules 4 and 5: rows come in position order
            for c, by, k in rows:
                ct = w.piece(c, by, k)
                if ct is not None:
                    table.setdefault(ct.name.encode(), (bytes(c), ct))
            sn = scan[s]
            for k in range(sn["child_first"], sn["child_first"] + sn["n_children"]):
                hit = table.get(scan[k]["name"])
                if hit is None:
                    continue
                res[k] = (verdict(scan[k], hit[1], trust_before), hit[0])
                if res[k][0] == DIR:
                    nxt.append((k, hit[0], hit[1]))
        if not nxt:
            return done(levels)
        levels += 1
        items = nxt


def scan_invalid(scan, names_len=None):
    """The scan's rules (what bw_parent_match answers BW_EINVAL to): kind in {File, Dir}, a File without
    children, a Dir's children after itself and inside the scan, no node the child of two.  Names are
    bytes here, so their ranges are not in question."""
    seen = [0] * len(scan)
    for i, n in enumerate(scan):
        if n["kind"] not in (rr.KIND_FILE, rr.KIND_DIR):
            return True
        if n["kind"] == rr.KIND_FILE:
            if n["n_children"]:
                return True
            continue
        if not n["n_children"]:
            continue
        if n["child_first"] <= i or n["child_first"] + n["n_children"] > len(scan):
            return True
        for k in range(n["child_first"], n["child_first"] + n["n_children"]):
            seen[k] += 1
            if seen[k] > 1:
                return True
    return False
