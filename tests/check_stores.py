"""The stores of the check tests (tests/test_check.py on the CPU, tests/test_gpu_check.py on the GPU),
built with restore_store.Builder and damaged by hand.  A helper, not a test.

A store is (packs [(id, bytes)], index [(hash, id)]).  Every structure case carries the finding it must
yield, written down by hand: {"flags": {entry: bits}, "items": {item: status}, "tails": {packfile: tail}};
whatever is not named is clean."""
import struct

import numpy as np

import check_ref as cr
import prune_ref
import restore_ref as rr
import restore_store
from oracle import oracle
from oracle import pack_oracle as po

PRK = restore_store.PRK
PIECE = 8192 * 16  # bw_internal.h PIECE_BLOCKS: ciphertext bytes per GHASH piece


def blob_bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def reheader(pack, edit):
    """The packfile with its header entries replaced by edit(entries) and its blob section kept."""
    pid, buf = pack
    hl = struct.unpack_from("<Q", buf, 0)[0]
    ents = po.deserialize_header(oracle.open_blob(PRK, b"header", pid, bytes(buf[8:8 + hl])))
    header = oracle.seal_blob(PRK, b"header", pid, po.serialize_header(edit([list(e) for e in ents])))
    return pid, struct.pack("<Q", len(header)) + header + bytes(buf[8 + hl:])


def base_store(seed=51):
    """14 chunks of different sizes in packfiles of 5, 5 and 4."""
    rng = np.random.default_rng(seed)
    b = restore_store.Builder(seed=seed)
    for k in range(14):
        b.add(blob_bytes(rng, 40 + 23 * k))
    return b.finish(target=5)


def _set(k, field, fn):
    def edit(ents):
        ents[k][field] = fn(ents[k][field], ents)
        return ents
    return edit


LEN, OFF = 3, 4  # header entry fields: (hash, kind, compression, length, offset)


def structure_cases():
    """name -> (packs, index, expected finding)."""
    out = {}
    packs, index = base_store()
    hd = prune_ref.headers_of(PRK, packs)
    lens = [[e[LEN] for e in ents] for _, _, _, ents in hd]
    out["clean"] = (packs, index, {})

    p = list(packs)
    p[0] = reheader(p[0], _set(4, LEN, lambda v, _: v + 1000))
    out["length past the section"] = (p, index, {"flags": {4: cr.E_RANGE}, "tails": {0: -1000}})

    p = list(packs)
    p[1] = reheader(p[1], _set(4, LEN, lambda v, _: 15))
    out["length 15"] = (p, index, {"flags": {9: cr.E_RANGE}, "tails": {1: lens[1][4] - 15}})

    def swap(ents):
        ents[1][OFF], ents[2][OFF] = ents[2][OFF], ents[1][OFF]
        return ents
    p = list(packs)
    p[0] = reheader(p[0], swap)
    out["offsets swapped"] = (p, index, {"flags": {1: cr.E_ORDER, 2: cr.E_ORDER}})

    p = list(packs)
    p[2] = reheader(p[2], _set(2, OFF, lambda v, _: v - 1))
    out["overlap by one byte"] = (p, index, {"flags": {12: cr.E_ORDER}})

    p = list(packs)
    p[2] = (p[2][0], p[2][1][:-1])
    out["truncated by one byte"] = (p, index, {"flags": {13: cr.E_RANGE}, "tails": {2: -1}})

    p = list(packs)
    p[1] = (p[1][0], p[1][1] + b"\x00" * 5)
    out["five trailing bytes"] = (p, index, {"tails": {1: 5}})

    out["dropped index item"] = (packs, index[:6] + index[7:], {"flags": {6: cr.E_UNINDEXED}})
    out["item with an unknown id"] = (packs, index + [(index[3][0], b"\xee" * 12)], {"items": {14: rr.ENOPACKFILE}})
    out["item naming a packfile that lacks the hash"] = (packs, index + [(index[3][0], packs[1][0])], {"items": {14: rr.EMISMATCH}})
    out["item three times"] = (packs, index[:8] + [index[2]] + index[8:] + [index[2]],
                               {"items": {8: cr.IDUPLICATE, 15: cr.IDUPLICATE}})

    rng = np.random.default_rng(52)
    b = restore_store.Builder(seed=52)
    data = [blob_bytes(rng, 50 + 9 * k) for k in range(8)]
    for k in range(5):
        b.add(data[k])
    b.add(data[1], again=True)               # entry 5 of packfile 0 (target 6): hidden behind entry 1
    for k in range(5, 8):
        b.add(data[k])
    sp, si = b.finish(target=6)
    out["one hash twice in a packfile"] = (sp, si[:5] + si[6:], {"flags": {5: cr.E_SHADOWED}})
    out["one hash twice, indexed twice"] = (sp, si, {"flags": {5: cr.E_SHADOWED}, "items": {5: cr.IDUPLICATE}})

    # all together: every damage above in one store (no two on one entry)
    p = list(packs)
    p[0] = reheader(p[0], lambda ents: _set(4, LEN, lambda v, _: v + 1000)(swap(ents)))
    p[1] = reheader(p[1], _set(4, LEN, lambda v, _: 15))
    p[1] = (p[1][0], p[1][1] + b"\x00" * 5)
    p[2] = reheader(p[2], _set(2, OFF, lambda v, _: v - 1))
    p[2] = (p[2][0], p[2][1][:-1])
    ix = index[:6] + index[7:] + [(index[3][0], b"\xee" * 12), (index[3][0], packs[1][0]), index[2], index[2]]
    out["all together"] = (p, ix, {"flags": {1: cr.E_ORDER, 2: cr.E_ORDER, 4: cr.E_RANGE, 9: cr.E_RANGE, 12: cr.E_ORDER,
                                             13: cr.E_RANGE, 6: cr.E_UNINDEXED},
                                   "items": {13: rr.ENOPACKFILE, 14: rr.EMISMATCH, 15: cr.IDUPLICATE, 16: cr.IDUPLICATE},
                                   "tails": {0: -1000, 1: lens[1][4] - 15 + 5, 2: -1}})
    return out


def expected(headers, index, finding):
    """The finding as full arrays: (flags, item statuses, tails)."""
    n_e = sum(len(h[3]) for h in headers)
    flags, items, tails = [0] * n_e, [rr.OK] * len(index), [0] * len(headers)
    for k, v in finding.get("flags", {}).items():
        flags[k] = v
    for k, v in finding.get("items", {}).items():
        items[k] = v
    for k, v in finding.get("tails", {}).items():
        tails[k] = v
    return flags, items, tails


def one_packfile_of_300():
    rng = np.random.default_rng(53)
    b = restore_store.Builder(seed=53)
    for k in range(300):
        b.add(blob_bytes(rng, 8 + k % 37) + struct.pack("<I", k))
    return b.finish(target=300)


def thousand_packfiles_of_one():
    rng = np.random.default_rng(54)
    b = restore_store.Builder(seed=54)
    for k in range(1000):
        b.add(blob_bytes(rng, 5 + k % 11) + struct.pack("<I", k))
    return b.finish(target=1)


def _flip(packs, hd, h, where, bit=1):
    """One bit of the blob named h flipped: where = "nonce", "tag", or a ciphertext byte position."""
    for p, (_, _, hl, ents) in enumerate(hd):
        for eh, _, _, length, offset in ents:
            if eh == h:
                at = 8 + hl + offset
                at += 3 if where == "nonce" else 12 + length - 5 if where == "tag" else 12 + where
                buf = bytearray(packs[p][1])
                buf[at] ^= bit
                packs[p] = (packs[p][0], bytes(buf))
                return
    raise KeyError(h)


def data_store():
    """-> (packs, index, expected {hash: (auth status, full status)}, names).  22 entries in packfiles of 6;
    everything not named in `expected` is OK in both modes."""
    rng = np.random.default_rng(55)
    b = restore_store.Builder(seed=55)
    good = [b.add(blob_bytes(rng, 300 + 17 * k)) for k in range(4)]
    f_nonce, f_ct, f_tag = (b.add(blob_bytes(rng, 500 + k)) for k in range(3))
    big_data = blob_bytes(rng, PIECE + 9000)  # sealed above 128 KiB: two GHASH pieces, the first ragged
    big = b.add(big_data)
    not_zstd = b.add(blob_bytes(rng, 77), payload=b"\x00\x00\x07\x00\x00")       # sealed properly, not a frame
    other = blob_bytes(rng, 90)
    wrong_hash = b.add(blob_bytes(rng, 91), payload=po.zstd_store(other))        # sealed under another content's hash
    good_tree = b.add_tree(0, "f", 10, None, None, good[:2])
    bad_tree_data = b"\x02not a tree"
    bad_tree = b.add_raw_tree(bad_tree_data)                                     # named by its own hash, refused by the parser
    more = [b.add(blob_bytes(rng, 64 + k)) for k in range(10)]
    packs, index = b.finish(target=6)
    hd = prune_ref.headers_of(PRK, packs)
    _flip(packs, hd, f_nonce, "nonce")
    _flip(packs, hd, f_ct, 0, bit=0x80)
    _flip(packs, hd, f_tag, "tag")
    ct_len = len(po.zstd_store(big_data))
    first = (ct_len + 15) // 16 - 8192       # blocks of the first (ragged) piece: pieces are cut from the end
    _flip(packs, hd, big, 16 * first, bit=4)  # the first byte of the second piece
    exp = {f_nonce: (rr.ETAG, rr.ETAG), f_ct: (rr.ETAG, rr.ETAG), f_tag: (rr.ETAG, rr.ETAG), big: (rr.ETAG, rr.ETAG),
           not_zstd: (rr.OK, rr.EZSTD), wrong_hash: (rr.OK, rr.EDIGEST), bad_tree: (rr.OK, rr.EFORMAT)}
    return packs, index, exp, dict(good=good, more=more, good_tree=good_tree)
