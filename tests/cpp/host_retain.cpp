// Retain through the C++ host mirror (backuwup_amd/host/backuwup.hpp: Retain) against the C ABI: the store
// of host_impact.cpp, two snapshots that share a file and a chunk, asked as roots (A, B) and as roots
// (B, A, B); every drop set's live vector and sums are also held against bw_prune_mark over the kept roots.
#include <cstdio>
#include <cstring>

#include "../../backuwup_amd/host/backuwup.hpp"

using namespace backuwup;

static std::vector<uint8_t> tree_bytes(uint32_t kind, const std::string& name, bool has_mtime, uint64_t mtime,
                                       const std::vector<BlobHash>& children, uint64_t size = 0) {
    std::vector<uint8_t> ch;
    for (const auto& h : children) ch.insert(ch.end(), h.begin(), h.end());
    bw_tree t{};
    t.kind = kind;
    t.flags = has_mtime ? BW_TREE_HAS_MTIME | BW_TREE_HAS_SIZE : 0;
    t.mtime = mtime;
    t.size = size;
    t.name = (const uint8_t*)name.data();
    t.name_len = name.size();
    t.children = ch.data();
    t.n_children = children.size();
    uint64_t n = 0;
    bw_tree_serialize(&t, nullptr, nullptr, 0, &n);
    std::vector<uint8_t> out(n);
    check(bw_tree_serialize(&t, nullptr, out.data(), n, &n));
    return out;
}

int main() {
    Context ctx(0);
    std::array<uint8_t, 32> prk;
    prk.fill(0x3c);
    std::vector<std::vector<uint8_t>> datas;
    for (int k = 0; k < 4; k++) {
        std::vector<uint8_t> d(1000 + 37 * k);
        for (size_t i = 0; i < d.size(); i++) d[i] = (uint8_t)(i * 7 + k * 13);
        datas.push_back(d);
    }
    std::vector<std::pair<std::vector<uint8_t>, uint8_t>> blobs;  // bytes, kind
    for (auto& d : datas) blobs.push_back({d, BW_BLOB_FILE_CHUNK});
    auto hash_of = [&](const std::vector<uint8_t>& d) {
        BlobHash h;
        check(bw_blake3_hash(ctx.get(), d.data(), d.size(), h.data()), ctx.get());
        return h;
    };
    std::vector<BlobHash> ch;
    for (auto& d : datas) ch.push_back(hash_of(d));
    // A: a.bin, sub/b.bin.  B: a.bin as it was, sub/b.bin with another chunk and a later mtime, and new.bin
    const auto fa = tree_bytes(BW_TREE_FILE, "a.bin", true, 1500000000, {ch[0], ch[1]}, 2037);
    const auto fb_a = tree_bytes(BW_TREE_FILE, "b.bin", true, 1500000001, {ch[2]}, 1074);
    const auto fb_b = tree_bytes(BW_TREE_FILE, "b.bin", true, 1500000002, {ch[2], ch[3]}, 2185);
    const auto fn = tree_bytes(BW_TREE_FILE, "new.bin", true, 1500000003, {ch[2]}, 1074);
    const auto sub_a = tree_bytes(BW_TREE_DIR, "sub", false, 0, {hash_of(fb_a)});
    const auto sub_b = tree_bytes(BW_TREE_DIR, "sub", false, 0, {hash_of(fb_b)});
    const auto root_a = tree_bytes(BW_TREE_DIR, "", false, 0, {hash_of(fa), hash_of(sub_a)});
    const auto root_b = tree_bytes(BW_TREE_DIR, "", false, 0, {hash_of(fa), hash_of(sub_b), hash_of(fn)});
    for (auto* t : {&fa, &fb_a, &fb_b, &fn, &sub_a, &sub_b, &root_a, &root_b}) blobs.push_back({*t, BW_BLOB_TREE});

    // write: store frames sealed into one packfile, by the C ABI directly
    const uint64_t n = blobs.size();
    std::vector<uint8_t> src, hashes, kinds, nonces(12 * n);
    std::vector<uint64_t> off, len;
    for (uint64_t i = 0; i < n; i++) {
        off.push_back(src.size());
        len.push_back(blobs[i].first.size());
        src.insert(src.end(), blobs[i].first.begin(), blobs[i].first.end());
        const BlobHash h = hash_of(blobs[i].first);
        hashes.insert(hashes.end(), h.begin(), h.end());
        kinds.push_back(blobs[i].second);
        for (int k = 0; k < 12; k++) nonces[12 * i + k] = (uint8_t)(i * 12 + k);
    }
    uint64_t npf = 0, total = 0;
    int rc = bw_pack_plan(len.data(), n, BW_PACK_ZSTD_STORE, nullptr, 0, &npf, &total);
    if (rc != BW_ENOSPC) check(rc);
    std::vector<bw_packfile> plan(npf);
    check(bw_pack_plan(len.data(), n, BW_PACK_ZSTD_STORE, plan.data(), npf, &npf, &total));
    std::vector<uint8_t> ids(12 * npf, 0x77), out(total);
    check(bw_pack_build(ctx.get(), prk.data(), src.data(), off.data(), len.data(), n, hashes.data(), kinds.data(),
                        nonces.data(), BW_PACK_ZSTD_STORE, plan.data(), npf, ids.data(), out.data()),
          ctx.get());
    PackfileTable t;
    t.data = out;
    t.ids = ids;
    t.tab = plan;
    for (auto& f : t.tab) {
        f.header_len = 0;
        for (int k = 0; k < 8; k++) f.header_len |= (uint64_t)out[f.offset + k] << (8 * k);
    }
    std::vector<uint8_t> items;
    for (uint64_t i = 0; i < n; i++) {
        items.insert(items.end(), hashes.begin() + 32 * i, hashes.begin() + 32 * i + 32);
        items.insert(items.end(), ids.begin(), ids.begin() + 12);
    }
    const auto entries = unpack_headers(ctx, prk, t);
    // entries: chunks 0-3, a.bin 4, b.bin of A 5, b.bin of B 6, new.bin 7, sub of A 8, sub of B 9, root A 10, root B 11
    const std::vector<BlobHash> roots = {hash_of(root_a), hash_of(root_b)};
    Restore r(ctx, prk, t, entries, items, 2);
    Retain rt(ctx, r, entries, t.tab.size());
    const BlobHash A = hash_of(root_a), B = hash_of(root_b);
    auto show = [&](const char* what, const std::vector<BlobHash>& roots, const std::vector<std::vector<uint64_t>>& sets) {
        const Retain::Mark m = rt.mark(roots, true);
        std::printf("%s masks", what);
        for (uint64_t x : m.masks) std::printf(" %llu", (unsigned long long)x);
        std::printf(" | %llu %llu %llu %d %zu | %llu %llu\n", (unsigned long long)m.counts.n_trees_expanded,
                    (unsigned long long)m.counts.n_levels, (unsigned long long)m.counts.n_edges, m.counts.n_sweeps >= 1, m.errors.size(),
                    (unsigned long long)m.counts.reached_blobs, (unsigned long long)m.counts.orphan_blobs);
        for (size_t k = 0; k < roots.size(); k++) {
            uint64_t reached = 0, unique = 0;  // the bytes, from the masks and the headers
            for (size_t e = 0; e < entries.size(); e++) {
                bool alone = m.reaches(k, e);
                for (size_t o = 0; o < roots.size(); o++) alone = alone && (o == k || !m.reaches(o, e));
                if (m.reaches(k, e)) reached += 12 + entries[e].length;
                if (alone) unique += 12 + entries[e].length;
            }
            const bw_retain_root& p = m.per_root[k];
            std::printf("%s root %zu %llu %llu %llu %u %d %d\n", what, k, (unsigned long long)p.reached_blobs,
                        (unsigned long long)p.unique_blobs, (unsigned long long)p.n_damaged, p.status, m.complete(k),
                        p.reached_bytes == reached && p.unique_bytes == unique);
        }
        const Retain::Drop d = rt.drop(m, sets);
        for (size_t q = 0; q < sets.size(); q++) {
            // bw_prune_mark over the kept roots on the same session
            std::vector<uint8_t> kept, live(entries.size() + 1);
            for (size_t k = 0; k < roots.size(); k++)
                if (std::find(sets[q].begin(), sets[q].end(), (uint64_t)k) == sets[q].end()) kept.insert(kept.end(), roots[k].begin(), roots[k].end());
            const uint64_t n_kept = kept.size() / 32;
            kept.push_back(0);
            std::vector<bw_prune_packfile_stat> stats(t.tab.size() + 1);
            bw_prune_counts pc{};
            bw_prune_error errs[4];
            check(bw_prune_mark(r.get(), kept.data(), n_kept, BW_UNPACK_VERIFY, live.data(), stats.data(), &pc, errs, 4), ctx.get());
            const bool same = !memcmp(live.data(), d.live.data() + q * entries.size(), entries.size()) &&
                              !memcmp(stats.data(), d.stats.data() + q * t.tab.size(), sizeof(bw_prune_packfile_stat) * t.tab.size());
            std::printf("%s drop %zu freed %llu live %llu bytes %d prune %d\n", what, q, (unsigned long long)d.freed[q].freed_blobs,
                        (unsigned long long)d.freed[q].live_blobs,
                        d.freed[q].live_bytes == pc.live_bytes && d.freed[q].freed_bytes + d.freed[q].live_bytes == m.counts.reached_bytes, same);
        }
    };
    show("ab", {A, B}, {{}, {0}, {1}, {0, 1}});
    show("bab", {B, A, B}, {{0}, {0, 2}, {1}});
    return 0;
}
