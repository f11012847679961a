// Prune through the C++ host mirror (backuwup_amd/host/backuwup.hpp: Prune) against the C ABI: a store
// with one blob no root reaches is marked, planned and repacked, and the pruned store restored.
#include <cstdio>
#include <cstring>
#include <map>

#include "../../backuwup_amd/host/backuwup.hpp"

using namespace backuwup;

static std::vector<uint8_t> tree_bytes(uint32_t kind, const std::string& name, bool has_mtime, uint64_t mtime,
                                       const std::vector<BlobHash>& children) {
    std::vector<uint8_t> ch;
    for (const auto& h : children) ch.insert(ch.end(), h.begin(), h.end());
    bw_tree t{};
    t.kind = kind;
    t.flags = has_mtime ? BW_TREE_HAS_MTIME : 0;
    t.mtime = mtime;
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
    // four chunks, two files (one chunk shared, one file empty-named directory apart), one directory
    std::vector<std::vector<uint8_t>> datas;
    for (int k = 0; k < 4; k++) {  // the fourth chunk is in no file
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
    const auto fa = tree_bytes(BW_TREE_FILE, "a.bin", true, 1500000000, {ch[0], ch[1], ch[0]});
    const auto fb = tree_bytes(BW_TREE_FILE, "b.bin", false, 0, {ch[2]});
    const auto sub = tree_bytes(BW_TREE_DIR, "sub", false, 0, {hash_of(fb)});
    const auto root = tree_bytes(BW_TREE_DIR, "", false, 0, {hash_of(fa), hash_of(sub)});
    for (auto* t : {&fa, &fb, &sub, &root}) blobs.push_back({*t, BW_BLOB_TREE});

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
    const BlobHash root_hash = hash_of(root);
    std::vector<std::pair<PackfileId, std::vector<uint8_t>>> packs;
    std::vector<uint8_t> new_items;
    {
        Restore r(ctx, prk, t, entries, items, 2);
        Prune p(ctx, r, t, entries);
        const auto none = p.mark({});
        const auto m = p.mark({root_hash, BlobHash{}}, true);  // the second root is nowhere: one error, the walk goes on
        uint64_t dead = 0;
        for (size_t e = 0; e < entries.size(); e++)
            if (!m.live[e]) dead += !std::memcmp(entries[e].hash, ch[3].data(), 32);
        std::printf("mark %llu %llu %llu %llu %zu %u %llu\n", (unsigned long long)none.counts.live_blobs,
                    (unsigned long long)m.counts.live_blobs, (unsigned long long)m.counts.total_blobs,
                    (unsigned long long)m.counts.n_trees_expanded, m.errors.size(), m.errors.empty() ? 0 : m.errors[0].reason,
                    (unsigned long long)dead);
        const auto rw = Prune::choose_rewrite(m.stats);
        const auto pl = p.plan(m.live, rw);
        PackfileId nid;
        nid.fill(0x55);
        packs = p.repack(pl, {nid});
        std::printf("plan %zu %zu %d\n", pl.order.size(), pl.plan.size(), pl.total_bytes == packs[0].second.size());
        for (uint64_t e : pl.order) {
            new_items.insert(new_items.end(), entries[e].hash, entries[e].hash + 32);
            new_items.insert(new_items.end(), nid.begin(), nid.end());
        }
    }
    // the pruned store: the kept root restores, the dropped chunk is gone
    const PackfileTable t2 = packfile_table(packs);
    const auto e2 = unpack_headers(ctx, prk, t2);
    Restore r2(ctx, prk, t2, e2, new_items, 2);
    const auto files = r2.unpack(root_hash, uint64_t(64) << 20, true);
    std::vector<uint8_t> want_a = datas[0];
    want_a.insert(want_a.end(), datas[1].begin(), datas[1].end());
    want_a.insert(want_a.end(), datas[0].begin(), datas[0].end());
    const auto st = r2.locate({ch[1], ch[3]});
    std::printf("pruned %zu %zu %d %d %d %d\n", e2.size(), files.size(), files[0].data == want_a, files[1].data == datas[2], st[0],
                st[1]);
    Prune p2(ctx, r2, t2, e2);
    const auto again = p2.mark({root_hash});
    std::printf("again %llu %llu\n", (unsigned long long)(again.counts.total_bytes - again.counts.live_bytes),
                (unsigned long long)p2.plan(again.live, Prune::choose_rewrite(again.stats)).order.size());
    return 0;
}
