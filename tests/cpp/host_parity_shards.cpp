// Parity through the C++ host mirror (backuwup_amd/host/backuwup.hpp: Parity) against the C ABI: a small
// store of five packfiles is protected with k = 3, m = 2, damaged (one packfile gone, one with a flipped
// byte, one parity shard gone) and repaired; the rebuilt bytes are compared with the originals.
#include <cstdio>
#include <cstring>

#include "../../backuwup_amd/host/backuwup.hpp"

using namespace backuwup;

int main() {
    Context ctx(0);
    const std::vector<uint64_t> sizes{5000, 17, 4096, 1, 2100};
    PackfileTable t;
    for (size_t p = 0; p < sizes.size(); p++) {
        bw_packfile f{};
        f.offset = t.data.size();
        f.size = sizes[p];
        t.tab.push_back(f);
        for (uint64_t i = 0; i < sizes[p]; i++) t.data.push_back((uint8_t)(1 + (i * 7 + p * 31) % 255));
    }
    const auto plan = Parity::plan(sizes, 3, 2);
    std::printf("plan %zu %llu %u %u %llu\n", plan.groups.size(), (unsigned long long)plan.out_bytes, plan.groups[1].k,
                plan.groups[1].m, (unsigned long long)plan.groups[0].shard_len);
    const auto built = Parity::build(ctx, t, plan);
    // the digests are the library's own BLAKE3 of the shards
    int digests_ok = 1;
    for (size_t p = 0; p < 3; p++) {
        BlobHash h = blake3::hash(ctx, t.data.data() + t.tab[p].offset, t.tab[p].size);
        digests_ok &= !std::memcmp(h.data(), &built.digests[32 * p], 32);
    }
    const bw_parity_group& g = plan.groups[0];
    BlobHash hp = blake3::hash(ctx, built.parity.data() + g.out_offset, g.shard_len);
    digests_ok &= !std::memcmp(hp.data(), &built.digests[32 * 3], 32);
    std::printf("digests %d\n", digests_ok);

    // group 0: packfile 0 gone, packfile 2 damaged, parity shard 1 present, parity shard 0 present
    const uint32_t n = g.k + g.m;
    std::vector<uint8_t> shards, present{0, 1, 1, 1, 1};
    std::vector<uint64_t> off(n), size(n), out_off(n);
    for (uint32_t s = 0; s < n; s++) {
        size[s] = s < g.k ? sizes[s] : g.shard_len;
        out_off[s] = s * g.shard_len;
        off[s] = shards.size();
        if (!present[s]) continue;
        const uint8_t* src = s < g.k ? t.data.data() + t.tab[s].offset : built.parity.data() + g.out_offset + (s - g.k) * g.shard_len;
        shards.insert(shards.end(), src, src + size[s]);
    }
    shards[off[2] + 100] ^= 0x40;
    const std::vector<uint8_t> dig(built.digests.begin(), built.digests.begin() + 32 * n);
    const auto r = Parity::repair(ctx, g, present, shards, off, size, dig, out_off, n * g.shard_len);
    std::printf("repair %d %d %d %d %d  %d %d\n", r.status[0], r.status[1], r.status[2], r.status[3], r.status[4],
                !std::memcmp(&r.data[out_off[0]], t.data.data() + t.tab[0].offset, sizes[0]),
                !std::memcmp(&r.data[out_off[2]], t.data.data() + t.tab[2].offset, sizes[2]));
    // without digests the damaged shard is used: the rebuilt packfile 0 differs at byte 100
    const auto r2 = Parity::repair(ctx, g, present, shards, off, size, {}, out_off, n * g.shard_len);
    size_t diff = 0;
    for (uint64_t i = 0; i < sizes[0]; i++) diff += r2.data[out_off[0] + i] != t.data[t.tab[0].offset + i];
    std::printf("nodigest %d %zu\n", r2.status[0], diff);
    // three gone and the damaged one among the rest: lost, and solve says so
    present = {0, 0, 1, 0, 1};
    const auto r3 = Parity::repair(ctx, g, present, shards, off, size, dig, out_off, n * g.shard_len);
    int rc = 0;
    try {
        Parity::solve(3, 2, present);
    } catch (const Error& e) {
        rc = e.rc;
    }
    std::printf("lost %d %d %d %d %d  %d\n", r3.status[0], r3.status[1], r3.status[2], r3.status[3], r3.status[4], rc == BW_ETOOFEW);
    // the primitive: the Cauchy rows of (3, 2) times the group's packfiles is its parity
    const auto s = Parity::solve(3, 2, {0, 1, 1, 1, 0});
    std::printf("solve %u %u %u  %u %u  %zu\n", s.used[0], s.used[1], s.used[2], s.missing[0], s.missing[1], s.matrix.size());
    const auto mm = Parity::matmul(ctx, {142, 244, 71, 244, 142, 167}, t.data, {t.tab[0].offset, t.tab[1].offset, t.tab[2].offset},
                                   {sizes[0], sizes[1], sizes[2]}, {0, g.shard_len}, g.shard_len, 2 * g.shard_len);
    std::printf("matmul %d\n", !std::memcmp(mm.data(), built.parity.data() + g.out_offset, 2 * g.shard_len));
    return 0;
}
