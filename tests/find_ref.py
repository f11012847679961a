"""A plain Python restatement of find (include/backuwup_gpu_pack.h, "find") over tests/restore_ref.py's
Store and tests/prune_ref.py's headers_of / Locator.  A helper, not a test: the GPU walk is compared with
what walk() returns over the same packfiles.  The reference cannot ask the question, so the rules are the
header's, stated twice and independently:
  to_regex()  a pattern translated to a Python `re` over the path with a '/' behind every component: the
              verdict
  Nfa         a position-set simulation with its own parser: whether a directory can still have a match
              below it (alive), and the verdict again (tests/test_find.py cross-checks the two by
              enumeration)
walk() takes the verdict from the regex and alive from the simulation."""
import re
from collections import Counter

import impact_ref as ir
import prune_ref as pr
import restore_ref as rr
from oracle import pack_oracle as po

HIT, UNREADABLE, TRUNCATED, CYCLIC, PRUNED = 1, 2, 4, 8, 16
NONE = 2**64 - 1
ZERO = bytes(32)
MAX_STATES = 64
U64 = 2**64 - 1


# ------------------------------------------------------------------ the verdict: a regex per pattern
def _lit(ch, icase):
    if icase and ch.isascii() and ch.isalpha():
        return "[" + ch.lower() + ch.upper() + "]"
    return re.escape(ch)


def to_regex(pattern, icase=False):
    """-> (compiled regex to fullmatch against path + '/', dir_only).  ValueError when the pattern is refused
    for its form (the 64-state limit is the automaton's: Nfa)."""
    try:
        s = bytes(pattern).decode("utf-8")
    except UnicodeDecodeError:
        raise ValueError("invalid UTF-8")
    if not s:
        raise ValueError("empty pattern")
    skip = "(?:[^/]*/)*"
    out, i = ("" if s[0] == "/" else skip), (1 if s[0] == "/" else 0)
    comps, cur, raw = [], "", ""
    while True:
        ch = s[i] if i < len(s) else None
        if ch is None or ch == "/":
            comps.append((cur, raw))
            cur, raw = "", ""
            if ch is None:
                break
            i += 1
            continue
        i += 1
        raw += ch
        if ch == "*":
            cur += "[^/]*"
        elif ch == "?":
            cur += "[^/]"
        elif ch == "\\":
            if i == len(s):
                raise ValueError("dangling backslash")
            if s[i] == "/":
                raise ValueError("escaped slash")
            cur += _lit(s[i], icase)
            raw += "x"
            i += 1
        elif ch == "[":
            neg = i < len(s) and s[i] in "!^"
            i += neg
            members, first = set(), True
            while True:
                if i == len(s):
                    raise ValueError("unterminated class")
                lo = s[i]
                i += 1
                if lo == "]" and not first:
                    break
                first = False
                if lo == "\\":
                    if i == len(s):
                        raise ValueError("dangling backslash")
                    lo = s[i]
                    i += 1
                hi = lo
                if i + 1 < len(s) and s[i] == "-" and s[i + 1] != "]":
                    hi = s[i + 1]
                    i += 2
                    if hi == "\\":
                        if i == len(s):
                            raise ValueError("dangling backslash")
                        hi = s[i]
                        i += 1
                if not (lo.isascii() and hi.isascii()):
                    raise ValueError("non-ASCII class member")
                if "/" in (lo, hi):
                    raise ValueError("slash in class")
                if hi < lo:
                    raise ValueError("backwards range")
                for o in range(ord(lo), ord(hi) + 1):
                    m = chr(o)
                    if m != "/":
                        members |= {m.lower(), m.upper()} if icase and m.isalpha() else {m}
            body = "".join(re.escape(m) for m in sorted(members))
            cur += ("[^/" + body + "]") if neg else ("[" + body + "]")
            raw += "x"
        else:
            cur += _lit(ch, icase)
    dir_only = False
    if len(comps) > 1 and comps[-1][1] == "":
        dir_only = True
        comps.pop()
    for frag, rawc in comps:
        if rawc == "":
            raise ValueError("empty component")
        out += skip if rawc == "**" else frag + "/"
    return re.compile(out, re.S), dir_only


# ------------------------------------------------------------------ alive: a position-set simulation
class Nfa:
    """Atoms over bytes, written apart from to_regex: ('set', bytes accepted, wide), ('star',), ('slash',),
    ('dstar',).  Position len(atoms) is the end.  ValueError when the pattern is refused."""

    def __init__(self, pattern, icase=False):
        p = bytes(pattern)
        try:
            p.decode("utf-8")
        except UnicodeDecodeError:
            raise ValueError("invalid UTF-8")
        if not p:
            raise ValueError("empty pattern")
        point = frozenset(b for b in range(256) if b != 0x2F and (b < 0x80 or b >= 0xC0))  # ASCII or a lead byte

        def fold(b):
            if icase and (0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A):
                return {b, b ^ 0x20}
            return {b}

        atoms = [] if p[:1] == b"/" else [("dstar",)]
        i = 1 if p[:1] == b"/" else 0
        self.dir_only = False
        while True:
            comp, start, only_stars = [], i, True
            while i < len(p) and p[i] != 0x2F:
                c = p[i]
                i += 1
                if c == 0x2A:
                    if not comp or comp[-1] != ("star",):
                        comp.append(("star",))
                    continue
                only_stars = False
                if c == 0x3F:
                    comp.append(("set", point, True))
                elif c == 0x5C:
                    if i == len(p):
                        raise ValueError("dangling backslash")
                    if p[i] == 0x2F:
                        raise ValueError("escaped slash")
                    comp.append(("set", frozenset(fold(p[i])), False))
                    i += 1
                elif c == 0x5B:
                    neg = i < len(p) and p[i] in b"!^"
                    i += neg
                    inside, first = set(), True
                    while True:
                        if i == len(p):
                            raise ValueError("unterminated class")
                        lo = p[i]
                        i += 1
                        if lo == 0x5D and not first:
                            break
                        first = False
                        if lo == 0x5C:
                            if i == len(p):
                                raise ValueError("dangling backslash")
                            lo = p[i]
                            i += 1
                        hi = lo
                        if i + 1 < len(p) and p[i] == 0x2D and p[i + 1] != 0x5D:
                            hi = p[i + 1]
                            i += 2
                            if hi == 0x5C:
                                if i == len(p):
                                    raise ValueError("dangling backslash")
                                hi = p[i]
                                i += 1
                        if lo >= 0x80 or hi >= 0x80:
                            raise ValueError("non-ASCII class member")
                        if 0x2F in (lo, hi):
                            raise ValueError("slash in class")
                        if hi < lo:
                            raise ValueError("backwards range")
                        for b in range(lo, hi + 1):
                            if b != 0x2F:
                                inside |= fold(b)
                    comp.append(("set", frozenset(point - inside if neg else inside), neg))
                else:
                    comp.append(("set", frozenset(fold(c)), False))
            if i == start:
                if i < len(p) or start <= 1:
                    raise ValueError("empty component")
                self.dir_only = True
                break
            if only_stars and i - start == 2:
                if not atoms or atoms[-1] != ("dstar",):
                    atoms.append(("dstar",))
            else:
                atoms += comp + [("slash",)]
            if i == len(p):
                break
            i += 1
        self.atoms, self.n_states = atoms, len(atoms)
        if self.n_states > MAX_STATES:
            raise ValueError("needs %d states" % self.n_states)
        self.start = self._close({0}, True)

    def _close(self, s, at_slash):
        s, todo = set(s), list(s)
        while todo:
            q = todo.pop()
            if q < len(self.atoms) and (self.atoms[q][0] == "star" or (at_slash and self.atoms[q][0] == "dstar")) and q + 1 not in s:
                s.add(q + 1)
                todo.append(q + 1)
        return frozenset(s)

    def step(self, s, b):
        t = set()
        for q in s:
            if q == len(self.atoms):
                continue
            a = self.atoms[q]
            if a[0] == "set":
                if b in a[1]:
                    t.add(q + 1)
            elif a[0] == "star":
                if b != 0x2F:
                    t.add(q)
            elif a[0] == "slash":
                if b == 0x2F:
                    t.add(q + 1)
            else:
                t.add(q)
            if q and 0x80 <= b <= 0xBF and self.atoms[q - 1][0] == "set" and self.atoms[q - 1][2]:
                t.add(q)
        return self._close(t, b == 0x2F)

    def run(self, s, name):
        for b in name:
            s = self.step(s, b)
        return s

    def accepts(self, s):
        return len(self.atoms) in self.step(s, 0x2F)

    def after_slash(self, s):
        """What a Dir hands down; empty = nothing below it can match."""
        return frozenset(self.step(s, 0x2F) - {len(self.atoms)})


# ------------------------------------------------------------------ the walk
def walk(store, headers, roots, patterns, icase=False, subtree=False, chunks=False, kinds=0, size=(0, U64), mtime=(0, U64)):
    """-> dict(records, names total, chunks [32-byte rows], per_root, errors Counter, counts).  records in
    the library's order (level after level, a level's items in row order): dict(level, root, parent (index
    or None), path (tuple of names below the root; b'?' + hash ends an unreadable item's), hash, name, kind,
    meta_flags, size, mtime, ctime, child_first, n_children, patterns, flags)."""
    locate = pr.Locator(store, headers)
    ents = pr.flat_entries(headers)
    n_e = len(ents)
    rx = [to_regex(p, icase) for p in patterns]
    nfa = [Nfa(p, icase) for p in patterns]
    records, errors, rows_out = [], Counter(), []
    per_root = [dict(n_records=0, n_hits=0, n_hit_files=0, hit_bytes=0, n_unreadable=0) for _ in roots]
    cnt = dict(n_records=0, name_bytes=0, n_chunks=0, n_levels=0, n_opened=0, n_pruned=0, n_errors=0)

    def piece(h, by, pos):
        st, e = locate(h)
        if st:
            errors[(bytes(h), by, pos, st)] += 1
            return None
        if ents[e][2] != po.KIND_TREE:
            errors[(bytes(h), by, pos, rr.ENOTTREE)] += 1
            return None
        cnt["n_opened"] += 1
        st, t = ir._open_tree(store, headers, ents[e])
        if st:
            errors[(bytes(h), by, pos, st)] += 1
            return None
        return t

    def chain(rec, h, by, pos):
        """The rows of the whole chain, the first piece fetched again: [(row, piece, position)]."""
        rows, cur_hash, rnd = [], h, 0
        cur = piece(h, by, pos)
        assert cur is not None  # the header fetch read it
        while True:
            rows += [(bytes(c), cur_hash, k) for k, c in enumerate(cur.children)]
            if cur.next_sibling is None:
                return rows
            nh, rnd = bytes(cur.next_sibling), rnd + 1
            if rnd > n_e:  # a chain of more pieces than the store has entries is refused unread
                errors[(nh, cur_hash, NONE, rr.EFORMAT)] += 1
                nxt = None
            else:
                nxt = piece(nh, cur_hash, NONE)
            if nxt is None:
                rec["flags"] |= TRUNCATED
                return rows
            cur, cur_hash = nxt, nh

    level = [dict(root=i, parent=None, h=bytes(r), by=ZERO, pos=i, anc=frozenset(), path=(), states=None, inherit=0)
             for i, r in enumerate(roots)]
    depth = 0
    while level:
        cnt["n_levels"] += 1
        base, expand, files = len(records), [], []
        for it in level:
            h = it["h"]
            rec = dict(level=depth, root=it["root"], parent=it["parent"], hash=h, name=b"", kind=0, meta_flags=0, size=0,
                       mtime=0, ctime=0, child_first=0, n_children=0, patterns=0, flags=0, path=it["path"])
            records.append(rec)
            cyclic = h in it["anc"]
            if cyclic:
                errors[(h, it["by"], it["pos"], rr.EFORMAT)] += 1
                rec["flags"] |= CYCLIC
            t = piece(h, it["by"], it["pos"])
            if t is None:
                rec["flags"] |= UNREADABLE
                rec["path"] = it["path"] + (b"?" + h,)
                continue
            name = t.name.encode()
            cnt["name_bytes"] += len(name)
            is_dir = t.kind == rr.KIND_DIR
            rec.update(name=name, kind=t.kind, size=t.size or 0, mtime=t.mtime or 0, ctime=t.ctime or 0,
                       meta_flags=(1 if t.size is not None else 0) | (2 if t.mtime is not None else 0) | (4 if t.ctime is not None else 0))
            if it["parent"] is None:
                carried = [n.start if is_dir else frozenset() for n in nfa]
            else:
                rec["path"] = it["path"] + (name,)
                text = "/".join(x.decode() for x in rec["path"]) + "/"
                carried = []
                for k, ((r, dir_only), n) in enumerate(zip(rx, nfa)):
                    if r.fullmatch(text) and (is_dir or not dir_only):
                        rec["patterns"] |= 1 << k
                    carried.append(n.after_slash(n.run(it["states"][k], name)) if is_dir else frozenset())
                rec["patterns"] |= it["inherit"]
            hit = rec["patterns"] != 0 and (not kinds or (kinds >> t.kind) & 1)
            if size != (0, U64):
                hit = hit and t.size is not None and size[0] <= t.size <= size[1]
            if mtime != (0, U64):
                hit = hit and t.mtime is not None and mtime[0] <= t.mtime <= mtime[1]
            if hit:
                rec["flags"] |= HIT
            if is_dir and not cyclic:
                if not any(carried) and not (subtree and rec["patterns"]):
                    rec["flags"] |= PRUNED
                    cnt["n_pruned"] += 1
                else:
                    expand.append((len(records) - 1, it, carried))
            elif not is_dir and hit and chunks and not cyclic:
                files.append((len(records) - 1, it))
        nxt = []
        for me, it, carried in expand:
            rec = records[me]
            rows = chain(rec, it["h"], it["by"], it["pos"])
            rec["n_children"] = len(rows)
            rec["child_first"] = base + len(level) + len(nxt) if rows else 0
            nxt += [dict(root=it["root"], parent=me, h=c, by=by, pos=pos, anc=it["anc"] | {it["h"]}, path=rec["path"],
                         states=carried, inherit=rec["patterns"] if subtree else 0) for c, by, pos in rows]
        for me, it in files:
            rec = records[me]
            rows = chain(rec, it["h"], it["by"], it["pos"])
            rec["child_first"], rec["n_children"] = len(rows_out), len(rows)
            rows_out += [c for c, _, _ in rows]
        level, depth = nxt, depth + 1
    for rec in records:
        p = per_root[rec["root"]]
        p["n_records"] += 1
        p["n_unreadable"] += bool(rec["flags"] & UNREADABLE)
        if rec["flags"] & HIT:
            p["n_hits"] += 1
            if rec["kind"] == rr.KIND_FILE:
                p["n_hit_files"] += 1
                p["hit_bytes"] += rec["size"]
    cnt.update(n_records=len(records), n_chunks=len(rows_out), n_errors=sum(errors.values()))
    return dict(records=records, chunks=rows_out, per_root=per_root, errors=errors, counts=cnt)


FIELDS = ("level", "root", "parent", "path", "hash", "name", "kind", "meta_flags", "size", "mtime", "ctime", "child_first",
          "n_children", "patterns", "flags")


def resolve(records):
    """The records as a list of tuples in FIELDS order: what the device's records are compared by, in order."""
    return [tuple(r[f] for f in FIELDS) for r in records]


def hit_paths(records, root, kind=None):
    """The '/'-joined paths of the hits under one root, sorted."""
    return sorted(b"/".join(r["path"]).decode() for r in records
                  if r["root"] == root and r["flags"] & HIT and (kind is None or r["kind"] == kind))
