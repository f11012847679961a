// Rekey through the C++ host mirror (backuwup_amd/host/backuwup.hpp: Rekey) against the C ABI: a store
// rekeyed from one PRK to another has the same table and headers, authenticates under the new PRK and
// not under the old one; resealed items open under the new PRK, and a damaged one stays refused.
#include <cstdio>
#include <cstring>

#include "../../backuwup_amd/host/backuwup.hpp"

using namespace backuwup;

static size_t count(const std::vector<uint8_t>& v, uint8_t x) {
    size_t n = 0;
    for (uint8_t b : v) n += b == x;
    return n;
}

int main() {
    Context ctx(0);
    std::array<uint8_t, 32> a, b;
    a.fill(0x3c);
    b.fill(0x91);
    // seven chunks in one packfile
    const uint64_t n = 7;
    std::vector<uint8_t> src, hashes, kinds, nonces(12 * n);
    std::vector<uint64_t> off, len;
    for (uint64_t i = 0; i < n; i++) {
        std::vector<uint8_t> d(700 + 53 * i);
        for (size_t k = 0; k < d.size(); k++) d[k] = (uint8_t)(k * 7 + i * 13);
        off.push_back(src.size());
        len.push_back(d.size());
        src.insert(src.end(), d.begin(), d.end());
        BlobHash h;
        check(bw_blake3_hash(ctx.get(), d.data(), d.size(), h.data()), ctx.get());
        hashes.insert(hashes.end(), h.begin(), h.end());
        kinds.push_back(BW_BLOB_FILE_CHUNK);
        for (int k = 0; k < 12; k++) nonces[12 * i + k] = (uint8_t)(i * 12 + k + 1);
    }
    uint64_t npf = 0, total = 0;
    int rc = bw_pack_plan(len.data(), n, BW_PACK_ZSTD_STORE, nullptr, 0, &npf, &total);
    if (rc != BW_ENOSPC) check(rc);
    std::vector<bw_packfile> plan(npf);
    check(bw_pack_plan(len.data(), n, BW_PACK_ZSTD_STORE, plan.data(), npf, &npf, &total));
    std::vector<uint8_t> ids(12 * npf, 0x77), out(total);
    check(bw_pack_build(ctx.get(), a.data(), src.data(), off.data(), len.data(), n, hashes.data(), kinds.data(), nonces.data(),
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
    const auto entries = unpack_headers(ctx, a, t);
    // the same store built under b: what the rekeyed store must equal
    std::vector<uint8_t> want(total);
    check(bw_pack_build(ctx.get(), b.data(), src.data(), off.data(), len.data(), n, hashes.data(), kinds.data(), nonces.data(),
                        BW_PACK_ZSTD_STORE, plan.data(), npf, ids.data(), want.data()),
          ctx.get());
    PackfileTable t2 = t;
    {
        Restore r(ctx, a, t, entries, items, 4);
        const auto s = Rekey::store(ctx, r, t, entries.size(), b);
        std::printf("store %zu %zu %zu %d\n", s.entry_status.size(), count(s.entry_status, BW_UNPACK_OK),
                    count(s.packfile_status, BW_UNPACK_OK), s.data == want && s.data != t.data);
        t2.data = s.data;
    }
    const auto entries2 = unpack_headers(ctx, b, t2);
    {
        Restore rb(ctx, b, t2, entries2, items, 4);
        Check cb(ctx, rb, t2, entries2, n);
        Restore ra(ctx, a, t2, entries2, items, 4);
        Check ca(ctx, ra, t2, entries2, n);
        std::printf("after %zu %zu %zu %zu\n", entries2.size(), count(cb.data(BW_CHECK_AUTH), BW_UNPACK_OK),
                    count(cb.data(BW_CHECK_FULL), BW_UNPACK_OK), count(ca.data(BW_CHECK_AUTH), BW_UNPACK_OK));
    }
    // one blob damaged: its status alone, and still refused under b
    PackfileTable bad = t;
    bad.data[bad.data.size() - 20] ^= 1;
    {
        Restore r(ctx, a, bad, entries, items, 4);
        const auto s = Rekey::store(ctx, r, bad, entries.size(), b);
        PackfileTable t3 = t;
        t3.data = s.data;
        Restore rb(ctx, b, t3, entries, items, 4);
        Check cb(ctx, rb, t3, entries, n);
        const auto st = cb.data(BW_CHECK_AUTH);
        std::printf("damaged %zu %d %zu %d\n", count(s.entry_status, BW_UNPACK_ETAG), s.entry_status[n - 1], count(st, BW_UNPACK_ETAG),
                    st[n - 1]);
    }
    // reseal() over a host buffer: three sealed items, the second with a flipped ciphertext bit, new nonces
    std::vector<uint64_t> so{0, 100, 300}, sl{50, 133, 0}, dof{0, 100, 300};
    std::vector<uint8_t> pt(400), sealed(400), info(3 * 32, 9), nn(36, 3), nn2(36, 5), opened(400);
    for (size_t k = 0; k < pt.size(); k++) pt[k] = (uint8_t)(k * 3 + 1);
    check(bw_seal(ctx.get(), a.data(), pt.data(), so.data(), sl.data(), 3, info.data(), 32, nn.data(), sealed.data(), dof.data()),
          ctx.get());
    sealed[100 + 64] ^= 0x10;
    for (auto& x : sl) x += 16;
    const auto rs = Rekey::reseal(ctx, a, b, sealed, dof, sl, info, 32, nn, nn2, dof, 400);
    std::vector<uint8_t> ok(3);
    check(bw_open(ctx.get(), b.data(), rs.data.data(), dof.data(), sl.data(), 3, info.data(), 32, nn2.data(), opened.data(), so.data(),
                  ok.data()),
          ctx.get());
    std::printf("reseal %d %d %d  %d %d %d  %d\n", rs.ok[0], rs.ok[1], rs.ok[2], ok[0], ok[1], ok[2],
                std::memcmp(opened.data(), pt.data(), 50) == 0);
    return 0;
}
