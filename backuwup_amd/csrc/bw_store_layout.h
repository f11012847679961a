// bw_store_layout.h -- where things lie in a store: a packfile's blob section, a blob's nonce and
// sealed bytes, the table's extent, the range rule, and the two layouts the host works out before a
// device call writes anything (rekey's items and gaps, repack's tables).  No device, context or HIP
// header: tests/cpp/store_layout_selftest.cpp.  Off the chunk -> hash -> dedup path
// (backuwup_amd/build.py OFF_PATH), like bw_restore.h.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/backuwup_gpu.h"

#ifdef __HIPCC__
#define BW_HOST_DEVICE __host__ __device__
#else
#define BW_HOST_DEVICE
#endif

namespace bw {

constexpr uint32_t RS_PIECE = 32768;  // bytes of one instance (a blob, a gap) that a wave copies

// What the tree parser reports for one blob (bincode::deserialize::<Tree>, trailing bytes allowed).
struct RsTreeHdr {
    uint32_t status;  // 0, or BW_RESTORE_EFORMAT
    uint32_t kind, flags, has_next;
    uint64_t size, mtime, ctime;
    uint64_t name_pos, name_len;  // the name's bytes inside the blob
    uint64_t ch_pos, n_children;  // the children's 32-byte rows inside the blob
    uint8_t next[32];
};

// BW_UNPACK_ERANGE, the one statement of it (the unpack chain, prune's mark and plan, check, rekey):
// the entry's nonce + sealed bytes lie inside the packfile's blob section, and the sealed bytes hold a tag
BW_HOST_DEVICE static inline bool rs_range_ok(uint64_t size, uint64_t header_len, uint64_t offset, uint64_t length) {
    const uint64_t base = 8 + header_len;
    return !(base > size || offset > size - base || BW_BLOB_NONCE_SIZE > size - base - offset ||
             length > size - base - offset - BW_BLOB_NONCE_SIZE || length < BW_SEAL_TAG_BYTES);
}

// A packfile in buffer coordinates: u64 LE header length | sealed header | blob section.  The section
// is nonce || sealed bytes per blob, at the offsets the header's entries give.
static inline uint64_t section_base(const bw_packfile& f) { return f.offset + 8 + f.header_len; }

struct BlobPlace {
    uint64_t nonce, sealed;  // the 12-byte nonce, and the e.length sealed bytes behind it
};
static inline BlobPlace blob_place(const bw_packfile& f, const bw_unpack_entry& e) {
    const uint64_t nonce = section_base(f) + e.offset;
    return BlobPlace{nonce, nonce + BW_BLOB_NONCE_SIZE};
}

// the bytes a buffer must hold for every file of the table (packfiles, index files) to lie in it
template <typename File>
static inline uint64_t store_extent(const File* files, uint64_t n) {
    uint64_t end = 0;
    for (uint64_t i = 0; i < n; i++) end = std::max<uint64_t>(end, files[i].offset + files[i].size);
    return end;
}

// bincode's varint, and one PackfileHeaderBlob's plaintext (hash, kind, compression, length, offset)
static inline uint32_t pack_varint_len(uint64_t v) { return v < 251 ? 1 : (v < (1ull << 16) ? 3 : (v < (1ull << 32) ? 5 : 9)); }
static inline uint64_t pack_entry_len(uint64_t sealed, uint64_t section_off) {
    return 32 + 1 + 1 + pack_varint_len(sealed) + pack_varint_len(section_off);
}

// ------------------------------------------------------------------ rekey
struct RkGap {
    uint64_t off, len;  // bytes [off, off + len) of the packfile buffer, the same place in both; len <= RS_PIECE
};

static inline void push_gap(std::vector<RkGap>& gaps, uint64_t lo, uint64_t hi) {
    for (; lo < hi; lo += RS_PIECE) gaps.push_back(RkGap{lo, std::min<uint64_t>(RS_PIECE, hi - lo)});
}

// What rekey reseals and what it copies.  The items are the packfile headers that are ok (in packfile
// order, info "header"; their nonces are the packfile ids, which the caller fills in), then the
// in-range entries in `ord`'s order (info = the entry's hash, the nonce at n_off in front of the
// sealed bytes).  Items and gaps together tile every packfile's [offset, offset + size) exactly once.
struct RekeyLayout {
    std::vector<uint64_t> ord;     // the in-range entries by (packfile, offset, index)
    std::vector<uint8_t> hdr_ok;   // per packfile: the header lies inside it and holds a tag
    uint64_t n_hdr = 0;            // headers that are ok: items [0, n_hdr); entry ord[j] is item n_hdr + j
    std::vector<uint64_t> s_off, s_len;  // per item: its sealed bytes
    std::vector<uint8_t> info;     // per item: 32 bytes, info_lens[k] of them used
    std::vector<uint32_t> info_lens;
    std::vector<uint64_t> n_off;   // per entry of ord: its nonce
    std::vector<RkGap> gaps;
};

// BW_OK, or BW_EINVAL with `why` when two in-range entries of one packfile overlap (every entry
// names a packfile of the table: bw_restore_open checked that)
static inline int rekey_layout(const bw_packfile* pf, uint64_t n_pf, const bw_unpack_entry* entries, uint64_t n_e,
                               RekeyLayout& L, std::string& why) {
    L = RekeyLayout();
    std::vector<uint64_t>& ord = L.ord;
    for (uint64_t e = 0; e < n_e; e++) {
        const bw_unpack_entry& en = entries[e];
        if (rs_range_ok(pf[en.packfile].size, pf[en.packfile].header_len, en.offset, en.length)) ord.push_back(e);
    }
    std::sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) {
        const bw_unpack_entry &x = entries[a], &y = entries[b];
        return x.packfile != y.packfile ? x.packfile < y.packfile : (x.offset != y.offset ? x.offset < y.offset : a < b);
    });
    for (uint64_t k = 1; k < ord.size(); k++) {
        const bw_unpack_entry &x = entries[ord[k - 1]], &y = entries[ord[k]];
        if (x.packfile == y.packfile && x.offset + BW_BLOB_NONCE_SIZE + x.length > y.offset) {
            why = "rekey: entries " + std::to_string(ord[k - 1]) + " and " + std::to_string(ord[k]) + " overlap";
            return BW_EINVAL;
        }
    }
    L.hdr_ok.resize(n_pf);
    for (uint64_t p = 0; p < n_pf; p++) {
        const bw_packfile& f = pf[p];
        L.hdr_ok[p] = f.header_len >= BW_SEAL_TAG_BYTES && f.size >= 8 && f.header_len <= f.size - 8;
        L.n_hdr += L.hdr_ok[p];
    }
    const uint64_t n_hdr = L.n_hdr, m = n_hdr + ord.size();
    L.n_off.resize(ord.size());
    L.s_off.resize(m);
    L.s_len.resize(m);
    L.info.resize(32 * m);
    L.info_lens.resize(m);
    uint64_t k = 0, at = 0;  // the next header item, the next entry of ord
    for (uint64_t p = 0; p < n_pf; p++) {
        const bw_packfile& f = pf[p];
        uint64_t cur = f.offset;  // the packfile's bytes before cur are resealed or in a gap
        if (L.hdr_ok[p]) {
            L.s_off[k] = f.offset + 8;
            L.s_len[k] = f.header_len;
            memcpy(&L.info[32 * k], "header", 6);
            L.info_lens[k] = 6;
            k++;
            push_gap(L.gaps, f.offset, f.offset + 8);
            cur = section_base(f);
        }
        for (; at < ord.size() && entries[ord[at]].packfile == p; at++) {
            const bw_unpack_entry& e = entries[ord[at]];
            const BlobPlace b = blob_place(f, e);
            L.n_off[at] = b.nonce;
            L.s_off[n_hdr + at] = b.sealed;
            L.s_len[n_hdr + at] = e.length;
            memcpy(&L.info[32 * (n_hdr + at)], e.hash, 32);
            L.info_lens[n_hdr + at] = 32;
            push_gap(L.gaps, cur, b.sealed);
            cur = b.sealed + e.length;
        }
        push_gap(L.gaps, cur, f.offset + f.size);
    }
    return BW_OK;
}

// ------------------------------------------------------------------ repack
// The tables of bw_prune_repack_device: moved blob i (entry order[i], old packfile old_pf[its
// packfile]) goes to the packfile of `plan` that holds position i.  The seven columns are n words
// each, in this order; RP_PIECE0 has n + 1.
enum { RP_ORDER = 0, RP_SECT, RP_HOFF, RP_SRC, RP_DST, RP_LEN, RP_PIECE0, RP_COLUMNS };

struct RepackTables {
    uint64_t n = 0;
    std::vector<uint64_t> tab;  // order | section offset | header entry's place | src | dst | len | piece prefix
    std::vector<uint64_t> h_off, h_len, h_dst;  // per new packfile: its header plaintext, and where the sealed header goes
    uint64_t hdr_total = 0, pieces = 0;
    const uint64_t* col(int c) const { return tab.data() + (uint64_t)c * n; }
};

static inline RepackTables repack_tables(const uint64_t* order, uint64_t n, const bw_packfile* plan, uint64_t npf,
                                         const bw_packfile* old_pf, const bw_unpack_entry* entries) {
    RepackTables r;
    r.n = n;
    r.tab.resize(RP_COLUMNS * n + 1);
    r.h_off.resize(npf);
    r.h_len.resize(npf);
    r.h_dst.resize(npf);
    uint64_t* t = r.tab.data();
    for (uint64_t p = 0; p < npf; p++) {
        const bw_packfile& f = plan[p];
        r.h_off[p] = r.hdr_total;
        r.h_len[p] = f.header_len - BW_SEAL_TAG_BYTES;
        r.h_dst[p] = f.offset + 8;
        uint64_t entry = r.hdr_total + pack_varint_len(f.n_blobs), section = 0;
        for (uint64_t i = f.first_blob; i < f.first_blob + f.n_blobs; i++) {
            const bw_unpack_entry& e = entries[order[i]];
            const uint64_t len = BW_BLOB_NONCE_SIZE + e.length;
            t[RP_ORDER * n + i] = order[i];
            t[RP_SECT * n + i] = section;
            t[RP_HOFF * n + i] = entry;
            t[RP_SRC * n + i] = blob_place(old_pf[e.packfile], e).nonce;
            t[RP_DST * n + i] = section_base(f) + section;
            t[RP_LEN * n + i] = len;
            t[RP_PIECE0 * n + i] = r.pieces;
            r.pieces += (len + RS_PIECE - 1) / RS_PIECE;
            entry += pack_entry_len(e.length, section);
            section += len;
        }
        r.hdr_total += r.h_len[p];
    }
    t[RP_PIECE0 * n + n] = r.pieces;
    return r;
}

}  // namespace bw
