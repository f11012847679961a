// The read side of the C++ host mirror (backuwup_amd/host/backuwup.hpp): write_packfiles_zstd, then
// unpack_headers + unpack_blobs (with the verify flag) and zstd_decompress over what it wrote, the
// way Manager::get_blob reads a packfile (unpack.rs:23-83).  tests/test_cpp_host_unpack.py checks
// the printed lines.
#include <cstdio>
#include <vector>

#include "../../backuwup_amd/host/backuwup.hpp"

int main() {
    using namespace backuwup;
    Context ctx(0);
    std::array<uint8_t, 32> prk;
    for (int k = 0; k < 32; k++) prk[k] = (uint8_t)(0x40 + k);
    std::vector<Blob> blobs;
    std::vector<BlobNonce> nonces;
    const size_t sizes[5] = {0, 5000, 200000, (1u << 20) + 17, 3u << 20};
    for (size_t j = 0; j < 5; j++) {
        Blob bl;
        bl.data.resize(sizes[j]);
        for (size_t i = 0; i < sizes[j]; i++) bl.data[i] = (uint8_t)('a' + ((i * (j + 3)) / 7) % 26);
        bl.hash = blake3::hash(ctx, bl.data.data(), bl.data.size());
        bl.kind = j == 2 ? BlobKind::Tree : BlobKind::FileChunk;
        blobs.push_back(bl);
        BlobNonce nn;
        for (int k = 0; k < 12; k++) nn[k] = (uint8_t)(3 * j + k + 1);
        nonces.push_back(nn);
    }
    std::vector<PackfileId> ids(40);
    for (size_t p = 0; p < ids.size(); p++)
        for (int k = 0; k < 12; k++) ids[p][k] = (uint8_t)(0x30 + 5 * p + k);
    auto packs = write_packfiles_zstd(ctx, prk, blobs, nonces, ids);
    PackfileTable t = packfile_table(packs);
    auto entries = unpack_headers(ctx, prk, t);
    std::vector<uint8_t> st;
    auto got = unpack_blobs(ctx, prk, t, entries, true, &st);
    size_t same = 0;
    for (size_t i = 0; i < got.size() && i < blobs.size(); i++)
        same += st[i] == BW_UNPACK_OK && got[i].data == blobs[i].data && got[i].hash == blobs[i].hash &&
                got[i].kind == blobs[i].kind;
    printf("unpack %zu %zu %zu %zu\n", packs.size(), entries.size(), got.size(), same);
    // one damaged blob: its status alone changes
    t.data[t.tab[0].offset + 8 + t.tab[0].header_len + entries[1].offset + 12 + 5] ^= 1;
    unpack_blobs(ctx, prk, t, entries, false, &st);
    printf("damaged");
    for (auto s : st) printf(" %d", (int)s);
    printf("\n");
    // frames alone: a store frame of "hello" and a broken one
    std::vector<bool> ok;
    auto dec = zstd_decompress(ctx, {{0x00, 0x00, 0x29, 0x00, 0x00, 'h', 'e', 'l', 'l', 'o'}, {0x00, 0x00, 0x07, 0x00, 0x00}}, &ok);
    printf("frames %d %d %.*s\n", (int)ok[0], (int)ok[1], (int)dec[0].size(), (const char*)dec[0].data());
    return 0;
}
