"""A plain Python restatement of check (include/backuwup_gpu_pack.h, "check") over packfile bytes, ids,
parsed header entries and index items.  A helper, not a test: the GPU outputs are compared elementwise
with what this returns.  The reference has no check, so the rules are the header's:

  structure  per entry: RANGE (prune_ref.range_ok fails), ORDER (offset != the sum of 12 + length over
             the earlier entries of the packfile), SHADOWED (an earlier entry of the packfile has the
             hash), UNINDEXED (not shadowed, and no index item is (hash, the packfile's id));
             per item: ENOPACKFILE (the id is not among the ids), EMISMATCH (that packfile's header lacks
             the hash), IDUPLICATE (a resolving item equal in both fields to one at a lower index), OK;
             per packfile: counts, claimed = sum of 12 + length, section = size - 8 - header_len, tail.
  data       per entry: SKIPPED, ERANGE, then AUTH: OK / ETAG by OpenSSL; FULL: ETAG by OpenSSL, EZSTD by
             libzstd, EDIGEST by the oracle's BLAKE3, EFORMAT for a Tree entry restore_ref's parser refuses.

headers: prune_ref.headers_of's [(packfile id, size, header_len, [(hash, kind, compression, length, offset)])]."""
import hashlib
import hmac

import prune_ref
import restore_ref as rr

E_RANGE, E_ORDER, E_UNINDEXED, E_SHADOWED = 1, 2, 4, 8
SKIPPED, IDUPLICATE = 32, 33
STAT_FIELDS = ("n_entries", "n_range", "n_order", "n_unindexed", "n_shadowed", "claimed_bytes", "section_bytes", "tail")


def structure(headers, index):
    """-> (entry flags [int], item statuses [int], stats [dict per packfile], counts dict)"""
    pos = {}
    for p, (pid, _, _, _) in enumerate(headers):
        pos.setdefault(bytes(pid), p)
    indexed = {(bytes(h), bytes(pid)) for h, pid in index}
    flags, stats = [], []
    for p, (pid, size, hl, ents) in enumerate(headers):
        seen, run = set(), 0
        st = dict.fromkeys(STAT_FIELDS, 0)
        for h, _, _, length, offset in ents:
            f = 0
            if not prune_ref.range_ok(size, hl, offset, length):
                f |= E_RANGE
            if offset != run:
                f |= E_ORDER
            if h in seen:
                f |= E_SHADOWED
            elif (h, bytes(pid)) not in indexed or pos[bytes(pid)] != p:
                f |= E_UNINDEXED
            seen.add(h)
            run += 12 + length
            flags.append(f)
            st["n_entries"] += 1
            for bit, name in ((E_RANGE, "n_range"), (E_ORDER, "n_order"), (E_UNINDEXED, "n_unindexed"), (E_SHADOWED, "n_shadowed")):
                st[name] += 1 if f & bit else 0
        st["claimed_bytes"] = run
        st["section_bytes"] = max(size - 8 - hl, 0)
        st["tail"] = st["section_bytes"] - run
        stats.append(st)
    hashes = [{e[0] for e in ents} for _, _, _, ents in headers]
    items, first = [], set()
    for h, pid in index:
        h, pid = bytes(h), bytes(pid)
        if pid not in pos:
            items.append(rr.ENOPACKFILE)
        elif h not in hashes[pos[pid]]:
            items.append(rr.EMISMATCH)
        elif (h, pid) in first:
            items.append(IDUPLICATE)
        else:
            first.add((h, pid))
            items.append(rr.OK)
    counts = {k: sum(st[k] for st in stats) for k in STAT_FIELDS if k != "tail"}
    counts.update(n_items_ok=items.count(rr.OK), n_items_nopackfile=items.count(rr.ENOPACKFILE),
                  n_items_mismatch=items.count(rr.EMISMATCH), n_items_duplicate=items.count(IDUPLICATE),
                  n_packfiles_clean=sum(1 for st in stats if not (st["n_range"] or st["n_order"] or st["n_unindexed"]
                                                                  or st["n_shadowed"] or st["tail"])))
    return flags, items, stats, counts


def _key(prk, info):
    return hmac.new(bytes(prk), bytes(info) + b"\x01", hashlib.sha256).digest()  # HKDF-Expand to 32 bytes: T(1)


def data(prk, packs, headers, mode, select=None):
    """-> statuses [int] per entry.  mode "auth" or "full"."""
    import openssl_ref
    import zstd_ref
    from oracle import oracle
    out, e = [], 0
    for p, (_, size, hl, ents) in enumerate(headers):
        buf = packs[p][1]
        for h, kind, _, length, offset in ents:
            e += 1
            if select is not None and not select[e - 1]:
                out.append(SKIPPED)
                continue
            if not prune_ref.range_ok(size, hl, offset, length):
                out.append(rr.ERANGE)
                continue
            at = 8 + hl + offset
            payload = openssl_ref.gcm_open(_key(prk, h), bytes(buf[at:at + 12]), bytes(buf[at + 12:at + 12 + length]))
            if payload is None:
                out.append(rr.ETAG)
                continue
            if mode == "auth":
                out.append(rr.OK)
                continue
            try:
                blob = zstd_ref.decompress(payload)
            except ValueError:
                out.append(rr.EZSTD)
                continue
            if oracle.blake3(blob) != h:
                out.append(rr.EDIGEST)
                continue
            if kind == 1:
                try:
                    rr.deserialize_tree(blob)
                except ValueError:
                    out.append(rr.EFORMAT)
                    continue
            out.append(rr.OK)
    return out


def bad_packfiles(headers, flags, stats, data_status=None, mark_error_hashes=()):
    """Sorted positions of the packfiles with a flagged entry, a nonzero tail, a data failure, or an
    entry whose hash a mark error names."""
    named = {bytes(h) for h in mark_error_hashes}
    bad, e = set(), 0
    for p, (_, _, _, ents) in enumerate(headers):
        if stats[p]["tail"]:
            bad.add(p)
        for ent in ents:
            if flags[e] or ent[0] in named or (data_status is not None and data_status[e] not in (rr.OK, SKIPPED)):
                bad.add(p)
            e += 1
    return sorted(bad)
