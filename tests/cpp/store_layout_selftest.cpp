// store_layout_selftest.cpp -- the store's layout rules (backuwup_amd/csrc/bw_store_layout.h) without
// a device.
//
// The header says where a blob lies in the packfile buffer (blob_place, section_base, store_extent),
// what rekey reseals and what it copies (rekey_layout: items and gaps that tile every packfile byte
// exactly once) and what repack uploads (repack_tables).  Here the small rules are compared with
// literals worked out by hand, rekey's layout is painted into a per-byte counter over seeded small
// stores, and repack's tables are compared with one serial restatement that shares no helper with
// the header.  tests/test_store_layout.py builds this with ASan + UBSan and runs it as a program.
#include <stdio.h>
#include <stdlib.h>

#include <tuple>

#include "../../backuwup_amd/csrc/bw_store_layout.h"

using namespace bw;

static int g_failed = 0;
#define CHECK(name, cond)                                                          \
    do {                                                                           \
        if (!(cond)) {                                                             \
            printf("FAIL %s: %s (line %d)\n", (name).c_str(), #cond, __LINE__);    \
            g_failed++;                                                            \
        }                                                                          \
    } while (0)

static uint64_t g_rng;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return rnd() % n; }

static bw_packfile packfile(uint64_t offset, uint64_t size, uint64_t header_len) {
    bw_packfile f;
    memset(&f, 0, sizeof f);
    f.offset = offset;
    f.size = size;
    f.header_len = header_len;
    return f;
}

static bw_unpack_entry entry(uint32_t pf, uint64_t offset, uint64_t length, uint8_t tag) {
    bw_unpack_entry e;
    memset(&e, 0, sizeof e);
    for (int i = 0; i < 32; i++) e.hash[i] = (uint8_t)(tag + 3 * i);
    e.packfile = pf;
    e.offset = offset;
    e.length = length;
    return e;
}

// ------------------------------------------------------------------ the small rules, by hand
static void test_places() {
    const std::string n = "places";
    // a packfile at byte 1000: prefix 1000..1007, a 40-byte header 1008..1047, the section from 1048
    const bw_packfile f = packfile(1000, 300, 40);
    CHECK(n, section_base(f) == 1048);
    // the entry at section offset 70: nonce 1118..1129, sealed bytes from 1130
    const bw_unpack_entry e = entry(0, 70, 33, 1);
    CHECK(n, blob_place(f, e).nonce == 1118);
    CHECK(n, blob_place(f, e).sealed == 1130);
    const bw_unpack_entry e0 = entry(0, 0, 16, 2);
    CHECK(n, blob_place(f, e0).nonce == 1048 && blob_place(f, e0).sealed == 1060);
    // the extent: the furthest end, whatever the order; empty packfiles count by their offset
    const bw_packfile t[3] = {packfile(500, 20, 16), packfile(0, 100, 16), packfile(519, 0, 0)};
    CHECK(n, store_extent(t, 3) == 520);
    CHECK(n, store_extent(t, 2) == 520);
    CHECK(n, store_extent(t + 1, 1) == 100);
    CHECK(n, store_extent(t + 2, 1) == 519);
    CHECK(n, store_extent((const bw_packfile*)nullptr, 0) == 0);
    // the range rule at its borders: a 16-byte blob that ends on the packfile's last byte
    CHECK(n, rs_range_ok(8 + 16 + 28, 16, 0, 16));
    CHECK(n, !rs_range_ok(8 + 16 + 27, 16, 0, 16));
    CHECK(n, !rs_range_ok(8 + 16 + 28, 16, 1, 16));
    CHECK(n, !rs_range_ok(8 + 16 + 28, 16, 0, 15));
    CHECK(n, !rs_range_ok(7, 16, 0, 16));
}

// ------------------------------------------------------------------ rekey's layout against a byte map
struct Store {
    std::vector<bw_packfile> pf;
    std::vector<bw_unpack_entry> en;
};

// the rules restated: what is in range, which headers are ok, the order
static bool naive_in_range(const bw_packfile& f, const bw_unpack_entry& e) {
    const unsigned __int128 first = (unsigned __int128)8 + f.header_len + e.offset;  // the nonce, from the packfile's start
    return e.length >= 16 && first + 12 + e.length <= f.size;
}
static bool naive_hdr_ok(const bw_packfile& f) { return f.header_len >= 16 && (unsigned __int128)8 + f.header_len <= f.size; }

static void check_layout(const std::string& n, const Store& st) {
    RekeyLayout L;
    std::string why;
    const int rc = rekey_layout(st.pf.data(), st.pf.size(), st.en.data(), st.en.size(), L, why);
    CHECK(n, rc == BW_OK && why.empty());
    if (rc) return;
    const uint64_t n_pf = st.pf.size();
    // hdr_ok and the order
    std::vector<std::tuple<uint32_t, uint64_t, uint64_t>> want;
    for (uint64_t e = 0; e < st.en.size(); e++)
        if (naive_in_range(st.pf[st.en[e].packfile], st.en[e])) want.emplace_back(st.en[e].packfile, st.en[e].offset, e);
    std::sort(want.begin(), want.end());
    CHECK(n, L.ord.size() == want.size());
    for (uint64_t k = 0; k < want.size() && k < L.ord.size(); k++) CHECK(n, L.ord[k] == std::get<2>(want[k]));
    uint64_t n_hdr = 0;
    CHECK(n, L.hdr_ok.size() == n_pf);
    for (uint64_t p = 0; p < n_pf; p++) {
        CHECK(n, (L.hdr_ok[p] != 0) == naive_hdr_ok(st.pf[p]));
        n_hdr += naive_hdr_ok(st.pf[p]);
    }
    CHECK(n, L.n_hdr == n_hdr);
    const uint64_t m = n_hdr + want.size();
    CHECK(n, L.s_off.size() == m && L.s_len.size() == m && L.info.size() == 32 * m && L.info_lens.size() == m);
    CHECK(n, L.n_off.size() == want.size());
    if (g_failed) return;
    // the items: headers first, in packfile order; then the entries in that order
    uint64_t k = 0;
    for (uint64_t p = 0; p < n_pf; p++) {
        if (!naive_hdr_ok(st.pf[p])) continue;
        CHECK(n, L.s_off[k] == st.pf[p].offset + 8 && L.s_len[k] == st.pf[p].header_len);
        CHECK(n, L.info_lens[k] == 6 && !memcmp(&L.info[32 * k], "header", 6));
        k++;
    }
    for (uint64_t j = 0; j < want.size(); j++) {
        const bw_unpack_entry& e = st.en[L.ord[j]];
        const bw_packfile& f = st.pf[e.packfile];
        CHECK(n, L.n_off[j] == f.offset + 8 + f.header_len + e.offset);
        CHECK(n, L.s_off[n_hdr + j] == L.n_off[j] + 12 && L.s_len[n_hdr + j] == e.length);
        CHECK(n, L.info_lens[n_hdr + j] == 32 && !memcmp(&L.info[32 * (n_hdr + j)], e.hash, 32));
    }
    // the byte map: items and gaps painted; every packfile byte once, nothing outside
    uint64_t end = 0;
    for (const bw_packfile& f : st.pf) end = std::max(end, f.offset + f.size);
    std::vector<uint32_t> count(end + 64, 0);
    std::vector<uint8_t> in_gap(end + 64, 0), inside(end + 64, 0);
    bool fits = true;
    for (uint64_t i = 0; i < m; i++) {
        fits = fits && L.s_off[i] + L.s_len[i] <= end;
        for (uint64_t b = L.s_off[i]; fits && b < L.s_off[i] + L.s_len[i]; b++) count[b]++;
    }
    for (const RkGap& g : L.gaps) {
        CHECK(n, g.len >= 1 && g.len <= RS_PIECE);
        fits = fits && g.off + g.len <= end;
        for (uint64_t b = g.off; fits && b < g.off + g.len; b++) {
            count[b]++;
            in_gap[b] = 1;
        }
    }
    CHECK(n, fits);
    for (const bw_packfile& f : st.pf)
        for (uint64_t b = f.offset; b < f.offset + f.size; b++) inside[b] = 1;
    uint64_t wrong = 0;
    for (uint64_t b = 0; b < count.size(); b++) wrong += count[b] != (inside[b] ? 1u : 0u);
    CHECK(n, wrong == 0);
    // a blob's nonce is copied, not resealed: its 12 bytes are gap bytes (a gap longer than RS_PIECE
    // is split at multiples of RS_PIECE from its start, so the nonce may lie in two of its parts)
    for (uint64_t j = 0; j < L.n_off.size(); j++)
        for (uint64_t b = L.n_off[j]; b < L.n_off[j] + 12; b++) CHECK(n, b < in_gap.size() && in_gap[b]);
}

// 1 to 4 packfiles of every shape the layout must take, 0 to 12 entries, no two in-range entries of
// one packfile overlapping
static Store seeded_store(uint64_t seed) {
    g_rng = seed;
    Store st;
    const uint64_t n_pf = 1 + below(4), n_en = below(13);
    std::vector<uint64_t> room(n_pf);  // section bytes the packfile has for blobs
    uint64_t at = below(3) ? below(20) : 0;
    for (uint64_t p = 0; p < n_pf; p++) {
        bw_packfile f;
        switch (below(7)) {
            case 0: f = packfile(at, 0, 0); room[p] = 0; break;                     // empty
            case 1: f = packfile(at, below(8), below(4)); room[p] = 0; break;       // size < 8
            case 2: {                                                               // the header runs to the last byte
                const uint64_t hl = 16 + below(20);
                f = packfile(at, 8 + hl, hl);
                room[p] = 0;
                break;
            }
            case 3: {  // a header too short to hold a tag, with a section behind it
                const uint64_t hl = below(16);
                room[p] = 28 + below(90);
                f = packfile(at, 8 + hl + room[p], hl);
                break;
            }
            case 4: {  // a header length that leaves the packfile
                const uint64_t size = 8 + below(40);
                f = packfile(at, size, size - 7 + below(30));
                room[p] = 0;
                break;
            }
            default: {
                const uint64_t hl = 16 + below(30);
                room[p] = below(150);
                f = packfile(at, 8 + hl + room[p], hl);
            }
        }
        st.pf.push_back(f);
        at += f.size + (below(3) ? 0 : below(9));  // back to back, or bytes between them that belong to nobody
    }
    // blobs laid out from the section's start, adjacent or a few bytes apart, while they fit
    std::vector<uint64_t> used(n_pf, 0);
    for (uint64_t i = 0; i < n_en; i++) {
        const uint32_t p = (uint32_t)below(n_pf);
        const uint64_t skip = below(3) ? 0 : 1 + below(5), len = 16 + below(24);
        if (below(5) == 0) {  // out of range: past the section, too short for a tag, or far outside
            const uint64_t kind = below(3);
            st.en.push_back(kind == 0 ? entry(p, room[p] + below(4), len, (uint8_t)i)
                                      : (kind == 1 ? entry(p, used[p], below(16), (uint8_t)i) : entry(p, ~0ull - below(40), len, (uint8_t)i)));
            continue;
        }
        if (used[p] + skip + 12 + len > room[p]) {  // does not fit: one that ends a byte past the packfile
            st.en.push_back(entry(p, room[p] >= 12 + len ? room[p] - 12 - len + 1 : 1, len, (uint8_t)i));
            continue;
        }
        st.en.push_back(entry(p, used[p] + skip, len, (uint8_t)i));
        used[p] += skip + 12 + len;
    }
    // out of offset order, and the entries of one packfile apart
    for (uint64_t i = st.en.size(); i > 1; i--) std::swap(st.en[i - 1], st.en[below(i)]);
    return st;
}

static void test_rekey_seeded() {
    uint64_t in_range = 0, bad_hdr_with_entry = 0, adjacent = 0, unordered = 0, out_of_range = 0, short_pf = 0, full_hdr = 0, empty = 0;
    for (uint64_t seed = 1; seed <= 400; seed++) {
        const Store st = seeded_store(seed);
        check_layout("rekey seed " + std::to_string(seed), st);
        // what the seeds reached
        for (const bw_packfile& f : st.pf) {
            short_pf += f.size && f.size < 8;
            empty += f.size == 0;
            full_hdr += naive_hdr_ok(f) && f.size == 8 + f.header_len;
        }
        for (uint64_t a = 0; a < st.en.size(); a++) {
            const bw_unpack_entry& x = st.en[a];
            const bool ok = naive_in_range(st.pf[x.packfile], x);
            in_range += ok;
            out_of_range += !ok;
            bad_hdr_with_entry += ok && !naive_hdr_ok(st.pf[x.packfile]);
            for (uint64_t b = 0; ok && b < st.en.size(); b++) {
                const bw_unpack_entry& y = st.en[b];
                if (y.packfile != x.packfile || !naive_in_range(st.pf[y.packfile], y)) continue;
                adjacent += x.offset + 12 + x.length == y.offset;
                unordered += a < b && x.offset > y.offset;
            }
        }
    }
    const std::string n = "rekey seeds reach every shape";
    CHECK(n, in_range > 100 && out_of_range > 50 && bad_hdr_with_entry > 10 && adjacent > 50 && unordered > 50);
    CHECK(n, short_pf > 10 && full_hdr > 10 && empty > 10);
}

static void test_rekey_overlap() {
    const std::string n = "rekey overlap";
    Store st;
    st.pf = {packfile(0, 8 + 16 + 200, 16), packfile(224, 8 + 16 + 100, 16)};
    // entries 3 and 1 of packfile 1 share a byte: 1 ends at 10 + 12 + 20 = 42, 3 starts at 41
    st.en = {entry(0, 0, 20, 1), entry(1, 10, 20, 2), entry(0, 32, 20, 3), entry(1, 41, 20, 4)};
    RekeyLayout L;
    std::string why;
    CHECK(n, rekey_layout(st.pf.data(), 2, st.en.data(), 4, L, why) == BW_EINVAL);
    CHECK(n, why == "rekey: entries 1 and 3 overlap");
    // one byte further and they are adjacent
    st.en[3].offset = 42;
    why.clear();
    CHECK(n, rekey_layout(st.pf.data(), 2, st.en.data(), 4, L, why) == BW_OK && why.empty());
    check_layout(n + " (adjacent)", st);
    // the same entry twice overlaps itself; the lower index comes first
    st.en[3] = st.en[1];
    CHECK(n, rekey_layout(st.pf.data(), 2, st.en.data(), 4, L, why) == BW_EINVAL);
    CHECK(n, why == "rekey: entries 1 and 3 overlap");
    // an overlap with an entry that is out of range is none
    st.en[3] = entry(1, 20, 200, 5);
    why.clear();
    CHECK(n, rekey_layout(st.pf.data(), 2, st.en.data(), 4, L, why) == BW_OK && why.empty());
}

static void test_rekey_long_gap() {
    const std::string n = "rekey long gap";
    // bytes no entry claims, then one blob: the gap up to its sealed bytes is 2 * RS_PIECE + 1 long
    const uint64_t gap = 2ull * RS_PIECE + 1, at = 5;
    Store st;
    st.pf = {packfile(at, 8 + 16 + gap + 30, 16)};
    st.en = {entry(0, gap - 12, 30, 9)};
    check_layout(n, st);
    RekeyLayout L;
    std::string why;
    CHECK(n, rekey_layout(st.pf.data(), 1, st.en.data(), 1, L, why) == BW_OK);
    const uint64_t base = at + 8 + 16;
    const RkGap want[4] = {{at, 8}, {base, RS_PIECE}, {base + RS_PIECE, RS_PIECE}, {base + 2ull * RS_PIECE, 1}};
    CHECK(n, L.gaps.size() == 4);
    for (uint64_t g = 0; g < 4 && g < L.gaps.size(); g++) CHECK(n, L.gaps[g].off == want[g].off && L.gaps[g].len == want[g].len);
    CHECK(n, L.s_off.size() == 2 && L.s_off[1] == base + gap && L.n_off[0] == base + gap - 12);
}

// ------------------------------------------------------------------ repack's tables against a serial restatement
static uint64_t naive_varint(uint64_t v) { return v <= 250 ? 1 : (v <= 0xffff ? 3 : (v <= 0xffffffffull ? 5 : 9)); }

static void test_repack() {
    const std::string n = "repack";
    // two old packfiles; five of their seven blobs move, one of them a bare tag and one longer than a piece
    std::vector<bw_packfile> old = {packfile(64, 8 + 40 + 70000, 40), packfile(80000, 8 + 30 + 500, 30)};
    std::vector<bw_unpack_entry> en = {entry(0, 0, 100, 1),     entry(0, 112, 40000, 2), entry(0, 40124, 16, 3), entry(0, 40152, 300, 4),
                                       entry(1, 0, 200, 5),     entry(1, 212, 16, 6),    entry(1, 240, 251, 7)};
    const uint64_t order[5] = {1, 2, 3, 4, 6};
    // the plan: blobs 0..2 in the first new packfile, 3..4 in the second (headers sized as the writer sizes them)
    uint64_t hl[2], sect[2] = {0, 0};
    const uint64_t first[3] = {0, 3, 5};
    for (int p = 0; p < 2; p++) {
        uint64_t h = naive_varint(first[p + 1] - first[p]);
        for (uint64_t i = first[p]; i < first[p + 1]; i++) {
            h += 32 + 1 + 1 + naive_varint(en[order[i]].length) + naive_varint(sect[p]);
            sect[p] += 12 + en[order[i]].length;
        }
        hl[p] = h + 16;
    }
    bw_packfile plan[2] = {packfile(0, 8 + hl[0] + sect[0], hl[0]), packfile(8 + hl[0] + sect[0], 8 + hl[1] + sect[1], hl[1])};
    for (int p = 0; p < 2; p++) {
        plan[p].first_blob = first[p];
        plan[p].n_blobs = first[p + 1] - first[p];
    }
    const RepackTables r = repack_tables(order, 5, plan, 2, old.data(), en.data());
    CHECK(n, r.n == 5 && r.tab.size() == 7 * 5 + 1 && r.h_off.size() == 2 && r.h_len.size() == 2 && r.h_dst.size() == 2);
    if (g_failed) return;
    const uint64_t *t_order = r.col(RP_ORDER), *t_sect = r.col(RP_SECT), *t_hoff = r.col(RP_HOFF), *t_src = r.col(RP_SRC),
                   *t_dst = r.col(RP_DST), *t_len = r.col(RP_LEN), *t_pc = r.col(RP_PIECE0);
    CHECK(n, t_order == r.tab.data() && t_pc == r.tab.data() + 30);
    uint64_t pieces = 0, hdr_total = 0;
    for (int p = 0; p < 2; p++) {
        CHECK(n, r.h_off[p] == hdr_total && r.h_len[p] == hl[p] - 16 && r.h_dst[p] == plan[p].offset + 8);
        uint64_t section = 0, hoff = hdr_total + naive_varint(plan[p].n_blobs);
        for (uint64_t i = first[p]; i < first[p + 1]; i++) {
            const bw_unpack_entry& e = en[order[i]];
            CHECK(n, t_order[i] == order[i]);
            CHECK(n, t_sect[i] == section);
            CHECK(n, t_hoff[i] == hoff);
            CHECK(n, t_src[i] == blob_place(old[e.packfile], e).nonce);
            CHECK(n, t_src[i] == old[e.packfile].offset + 8 + old[e.packfile].header_len + e.offset);
            CHECK(n, t_dst[i] == section_base(plan[p]) + section);
            CHECK(n, t_len[i] == 12 + e.length);
            CHECK(n, t_pc[i] == pieces);
            pieces += (12 + e.length + RS_PIECE - 1) / RS_PIECE;
            hoff += 32 + 1 + 1 + naive_varint(e.length) + naive_varint(section);
            section += 12 + e.length;
        }
        CHECK(n, hoff == hdr_total + hl[p] - 16);  // the entries fill the header's plaintext exactly
        CHECK(n, section_base(plan[p]) + section == plan[p].offset + plan[p].size);
        hdr_total += hl[p] - 16;
    }
    CHECK(n, t_pc[5] == pieces && r.pieces == pieces && pieces == 2 + 1 + 1 + 1 + 1);
    CHECK(n, r.hdr_total == hdr_total);
    CHECK(n, t_len[1] == 28);  // the bare tag: a nonce and 16 bytes
    // nothing moved: empty tables, and the piece prefix's one word
    const RepackTables z = repack_tables(nullptr, 0, nullptr, 0, old.data(), en.data());
    CHECK(n, z.tab.size() == 1 && z.tab[0] == 0 && z.pieces == 0 && z.hdr_total == 0);
    // the sizes of bincode's varint at their borders
    CHECK(n, pack_varint_len(250) == 1 && pack_varint_len(251) == 3 && pack_varint_len(65535) == 3 && pack_varint_len(65536) == 5);
    CHECK(n, pack_varint_len(0xffffffffull) == 5 && pack_varint_len(0x100000000ull) == 9);
    CHECK(n, pack_entry_len(251, 250) == 32 + 2 + 3 + 1);
}

int main() {
    test_places();
    test_rekey_seeded();
    test_rekey_overlap();
    test_rekey_long_gap();
    test_repack();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("store layout selftest ok\n");
    return 0;
}
