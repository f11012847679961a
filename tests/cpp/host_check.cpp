// Check through the C++ host mirror (backuwup_amd/host/backuwup.hpp: Check) against the C ABI: a clean
// store checks clean in every layer; with one tag byte flipped and one index item dropped, each layer
// reports exactly that.
#include <cstdio>
#include <cstring>

#include "../../backuwup_amd/host/backuwup.hpp"

using namespace backuwup;

static std::vector<uint8_t> tree_bytes(uint32_t kind, const std::string& name, const std::vector<BlobHash>& children) {
    std::vector<uint8_t> ch;
    for (const auto& h : children) ch.insert(ch.end(), h.begin(), h.end());
    bw_tree t{};
    t.kind = kind;
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

static size_t count(const std::vector<uint8_t>& v, uint8_t x) {
    size_t n = 0;
    for (uint8_t b : v) n += b == x;
    return n;
}

int main() {
    Context ctx(0);
    std::array<uint8_t, 32> prk;
    prk.fill(0x3c);
    auto hash_of = [&](const std::vector<uint8_t>& d) {
        BlobHash h;
        check(bw_blake3_hash(ctx.get(), d.data(), d.size(), h.data()), ctx.get());
        return h;
    };
    // five chunks, one file over them, one directory: seven blobs in one packfile
    std::vector<std::pair<std::vector<uint8_t>, uint8_t>> blobs;  // bytes, kind
    std::vector<BlobHash> ch;
    for (int k = 0; k < 5; k++) {
        std::vector<uint8_t> d(900 + 41 * k);
        for (size_t i = 0; i < d.size(); i++) d[i] = (uint8_t)(i * 5 + k * 11);
        ch.push_back(hash_of(d));
        blobs.push_back({d, BW_BLOB_FILE_CHUNK});
    }
    const auto file = tree_bytes(BW_TREE_FILE, "f.bin", ch);
    const auto root = tree_bytes(BW_TREE_DIR, "", {hash_of(file)});
    blobs.push_back({file, BW_BLOB_TREE});
    blobs.push_back({root, BW_BLOB_TREE});

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
        for (int k = 0; k < 12; k++) nonces[12 * i + k] = (uint8_t)(i * 12 + k + 1);
    }
    uint64_t npf = 0, total = 0;
    int rc = bw_pack_plan(len.data(), n, BW_PACK_ZSTD_STORE, nullptr, 0, &npf, &total);
    if (rc != BW_ENOSPC) check(rc);
    std::vector<bw_packfile> plan(npf);
    check(bw_pack_plan(len.data(), n, BW_PACK_ZSTD_STORE, plan.data(), npf, &npf, &total));
    std::vector<uint8_t> ids(12 * npf, 0x77), out(total);
    check(bw_pack_build(ctx.get(), prk.data(), src.data(), off.data(), len.data(), n, hashes.data(), kinds.data(), nonces.data(),
                        BW_PACK_ZSTD_STORE, plan.data(), npf, ids.data(), out.data()),
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
    {
        Restore r(ctx, prk, t, entries, items, 4);  // seven entries through four slots
        Check c(ctx, r, t, entries, n);
        const auto s = c.structure();
        std::printf("structure %llu %llu %llu %llu %llu %llu %llu %lld\n", (unsigned long long)s.counts.n_entries,
                    (unsigned long long)s.counts.n_range, (unsigned long long)s.counts.n_order,
                    (unsigned long long)s.counts.n_unindexed, (unsigned long long)s.counts.n_shadowed,
                    (unsigned long long)s.counts.n_items_ok, (unsigned long long)s.counts.n_packfiles_clean,
                    (long long)s.stats[0].tail);
        std::printf("data %zu %zu\n", count(c.data(BW_CHECK_AUTH), BW_UNPACK_OK), count(c.data(BW_CHECK_FULL), BW_UNPACK_OK));
    }
    // the last tag byte of the last blob flipped, the first index item dropped
    PackfileTable bad = t;
    bad.data[bad.data.size() - 1] ^= 1;
    const std::vector<uint8_t> fewer(items.begin() + BW_INDEX_ENTRY_BYTES, items.end());
    {
        Restore r(ctx, prk, bad, entries, fewer, 4);
        Check c(ctx, r, bad, entries, n - 1);
        const auto s = c.structure();
        std::vector<uint8_t> sel(n, 1);
        sel[1] = 0;
        const auto a = c.data(BW_CHECK_AUTH, sel), f = c.data(BW_CHECK_FULL, sel);
        std::printf("damaged %d %llu %llu %zu %zu %d %d %d\n", s.entry_flags[0], (unsigned long long)s.counts.n_unindexed,
                    (unsigned long long)s.counts.n_items_ok, count(a, BW_UNPACK_ETAG), count(f, BW_UNPACK_ETAG), a[n - 1], f[n - 1],
                    a[1] == BW_CHECK_SKIPPED && f[1] == BW_CHECK_SKIPPED);
    }
    // auth() over a host buffer: three sealed items, the second with a flipped ciphertext bit
    std::vector<uint64_t> so{0, 100, 300}, sl{50, 133, 0}, dof{0, 100, 300};
    std::vector<uint8_t> pt(400, 0x42), sealed(400), info(3 * 32, 9), nn(36, 3);
    check(bw_seal(ctx.get(), prk.data(), pt.data(), so.data(), sl.data(), 3, info.data(), 32, nn.data(), sealed.data(), dof.data()),
          ctx.get());
    sealed[100 + 64] ^= 0x10;
    for (auto& x : sl) x += 16;
    const auto ok = Check::auth(ctx, prk, sealed, dof, sl, info, 32, nn);
    std::printf("auth %d %d %d\n", ok[0], ok[1], ok[2]);
    return 0;
}
