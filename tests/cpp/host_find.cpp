// Find through the C++ host mirror (backuwup_amd/host/backuwup.hpp: Find) against the C ABI: the store of
// host_impact.cpp, two snapshots that share a file; a floating pattern, and an anchored one with chunk rows.
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
    Find fd(ctx, r);
    auto show = [&](const char* what, const std::string& pattern, uint32_t flags) {
        Find::Query q;
        q.patterns = {pattern};
        const Find::Paths p = fd.paths(roots, q, flags);
        for (size_t i = 0; i < p.records.size(); i++) {
            const bw_find_record& x = p.records[i];
            std::printf("%s rec %llu '%s' %u %u %u %llu %llu\n", what, (unsigned long long)x.root, p.path(i).c_str(), x.kind, x.patterns,
                        x.flags, (unsigned long long)x.child_first, (unsigned long long)x.n_children);
        }
        for (size_t k = 0; k < p.per_root.size(); k++)
            std::printf("%s root %zu %llu %llu %llu %llu %llu\n", what, k, (unsigned long long)p.per_root[k].n_records,
                        (unsigned long long)p.per_root[k].n_hits, (unsigned long long)p.per_root[k].n_hit_files,
                        (unsigned long long)p.per_root[k].hit_bytes, (unsigned long long)p.per_root[k].n_unreadable);
        std::printf("%s counts %llu %llu %llu %llu %llu %zu\n", what, (unsigned long long)p.counts.n_records,
                    (unsigned long long)p.counts.n_levels, (unsigned long long)p.counts.n_opened, (unsigned long long)p.counts.n_pruned,
                    (unsigned long long)p.counts.n_chunks, p.errors.size());
        if (p.counts.n_chunks == 1) std::printf("%s chunk %d\n", what, (int)std::equal(ch[2].begin(), ch[2].end(), p.chunks.begin()));
    };
    show("float", "*.bin", BW_UNPACK_VERIFY);
    show("anchored", "/new.bin", BW_FIND_CHUNKS);
    show("icase", "/SUB/", BW_FIND_ICASE | BW_FIND_SUBTREE);
    return 0;
}
