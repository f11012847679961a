"""A plain Python restatement of retain (include/backuwup_gpu_pack.h, "retain") over tests/prune_ref.py.  A
helper, not a test: the GPU mark and drop are compared with what this returns over the same packfiles.
The reference cannot ask the question, so the rules are the header's:

  - reach(e) is, by definition, the set of roots r for which prune_ref.mark over the single root r marks e
    live: the masks here are exactly that, one prune mark per root;
  - one more walk over all roots together (prune's rules, each distinct tree blob opened once) gives what
    the definition does not: the edges, the damage, the errors, the levels;
  - the edge rule (reach(c) |= open(p); for a tree reference to a Tree entry also open(c) |= open(p)),
    taken to its fixed point over those edges in forward level order, must give the same masks: fixed_point()
    returns them with the number of sweeps that order needs, and tests/test_retain.py holds the two together.

A root set is a Python int: bit r = root r."""
from collections import Counter

import impact_ref
import prune_ref as pr
import restore_ref as rr
from oracle import pack_oracle as po

NONE = 2**64 - 1
ZERO = bytes(32)


def walk(store, headers, roots):
    """prune's mark over all roots with what retain adds: -> dict(seeds [(entry, tree) or None per root],
    status per root, levels [[(parent, child, tree edge)]], damaged set, errors Counter, expanded, n_levels)."""
    locate = pr.Locator(store, headers)
    ents = pr.flat_entries(headers)
    live, queued, damaged, errors = set(), set(), set(), Counter()

    def visit(h, tree_ref, parent_hash, pos, nxt, parent_e, edges):
        st, e = locate(h)
        if st:
            errors[(bytes(h), parent_hash, pos, st)] += 1
            if parent_e is not None:
                damaged.add(parent_e)
            return st, None
        p, eh, kind, _, length, offset = ents[e]
        tree = kind == po.KIND_TREE
        status = 0
        if tree_ref and not tree:
            errors[(bytes(h), parent_hash, pos, rr.ENOTTREE)] += 1
            status = rr.ENOTTREE
            if parent_e is not None:
                damaged.add(parent_e)
        if e not in live:
            live.add(e)
            if not tree and not pr.range_ok(headers[p][1], headers[p][2], offset, length):
                errors[(eh, ZERO, NONE, rr.ERANGE)] += 1
                damaged.add(e)
        if parent_e is not None:
            edges.append((parent_e, e, tree_ref and tree))
        if tree_ref and tree and e not in queued:
            queued.add(e)
            nxt.append(e)
        return status, e

    front, seeds, status = [], [], []
    for i, r in enumerate(roots):
        st, e = visit(r, True, ZERO, i, front, None, None)
        status.append(st)
        seeds.append(None if e is None else (e, ents[e][2] == po.KIND_TREE))
    expanded, levels = 0, []
    while front:
        nxt, edges = [], []
        for e in front:
            h = ents[e][1]
            st, t = impact_ref._open_tree(store, headers, ents[e])
            if st:
                errors[(h, ZERO, NONE, st)] += 1
                damaged.add(e)
                continue
            expanded += 1
            for k, c in enumerate(t.children):
                visit(c, t.kind == rr.KIND_DIR, h, k, nxt, e, edges)
            if t.next_sibling is not None:
                visit(t.next_sibling, True, h, NONE, nxt, e, edges)
        levels.append(edges)
        front = nxt
    return dict(seeds=seeds, status=status, levels=levels, damaged=damaged, errors=errors, expanded=expanded,
                n_levels=len(levels), n_entries=len(ents))


def fixed_point(w):
    """The edge rule over walk()'s edges: -> (reach list of int, n_sweeps).  A sweep takes the tree edges
    earliest level first, in list order; the one that changes nothing counts.  The other edges pass nothing
    on and are settled once at the end."""
    n = w["n_entries"]
    reach, opened = [0] * n, [0] * n
    for i, s in enumerate(w["seeds"]):
        if s is not None:
            reach[s[0]] |= 1 << i
            if s[1]:
                opened[s[0]] |= 1 << i
    sweeps, changed = 0, True
    while changed:
        changed = False
        sweeps += 1
        for edges in w["levels"]:
            for p, c, tree in edges:
                if tree and (opened[p] & ~reach[c] or opened[p] & ~opened[c]):
                    reach[c] |= opened[p]
                    opened[c] |= opened[p]
                    changed = True
    for edges in w["levels"]:
        for p, c, tree in edges:
            if not tree:
                reach[c] |= opened[p]
    return reach, sweeps


def mark(store, headers, roots):
    """-> (masks list of int per entry, damaged list of 0/1, per_root list of dict, errors Counter, info dict)."""
    ents = pr.flat_entries(headers)
    n = len(ents)
    masks = [0] * n
    for i, r in enumerate(roots):  # the definition: one prune mark per root
        for e in pr.mark(store, headers, [r])[0]:
            masks[e] |= 1 << i
    w = walk(store, headers, roots)
    _, perrors, pinfo = pr.mark(store, headers, roots)
    assert w["errors"] == perrors and w["expanded"] == pinfo["n_trees_expanded"] and w["n_levels"] == pinfo["n_levels"]
    size = [12 + ent[4] for ent in ents]
    per_root = []
    for i in range(len(roots)):
        bit = 1 << i
        mine = [e for e in range(n) if masks[e] & bit]
        alone = [e for e in mine if masks[e] == bit]
        per_root.append(dict(reached_blobs=len(mine), reached_bytes=sum(size[e] for e in mine), unique_blobs=len(alone),
                             unique_bytes=sum(size[e] for e in alone), n_damaged=sum(1 for e in mine if e in w["damaged"]),
                             status=w["status"][i], pad=0))
    reached = [e for e in range(n) if masks[e]]
    info = dict(n_trees_expanded=w["expanded"], n_levels=w["n_levels"], n_edges=sum(len(x) for x in w["levels"]),
                n_sweeps=fixed_point(w)[1], reached_blobs=len(reached), reached_bytes=sum(size[e] for e in reached),
                orphan_blobs=n - len(reached), orphan_bytes=sum(size) - sum(size[e] for e in reached), walk=w)
    return masks, [int(e in w["damaged"]) for e in range(n)], per_root, w["errors"], info


def drop(headers, masks, dropped):
    """One question: -> (live list of 0/1, stats [(live blobs, live bytes, blobs, bytes)] per packfile, freed dict)."""
    ents = pr.flat_entries(headers)
    gone = sum(1 << r for r in set(dropped))
    live = [int(bool(m & ~gone)) for m in masks]
    stats = [[0, 0, 0, 0] for _ in headers]
    freed = dict(freed_blobs=0, freed_bytes=0, live_blobs=0, live_bytes=0)
    for e, ent in enumerate(ents):
        size = 12 + ent[4]
        s = stats[ent[0]]
        s[2] += 1
        s[3] += size
        if live[e]:
            s[0] += 1
            s[1] += size
            freed["live_blobs"] += 1
            freed["live_bytes"] += size
        elif masks[e]:
            freed["freed_blobs"] += 1
            freed["freed_bytes"] += size
    return live, [tuple(s) for s in stats], freed


def words_of(mask, n_roots):
    """A root set as the W u64 words of the ABI."""
    return [(mask >> (64 * w)) & (2**64 - 1) for w in range(max(1, (n_roots + 63) // 64))]
