// bw_rekey.hip -- rekey (include/backuwup_gpu_pack.h, "rekey"): the store of an open restore session
// under a new PRK, with the same packfile table.  The reference cannot change its backup secret.
// Every packfile header (info "header", nonce = the packfile id) and every in-range blob (info = the
// entry's hash, the nonce in front of it) goes through one bw_reseal_items call (k_reseal_ctr,
// k_reseal_tag: bw_seal.hip), which stores no plaintext; k_rekey_gaps copies what lies between the
// resealed ranges (the length prefix, the nonces, bytes no in-range entry claims) as it is.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/backuwup_gpu.h"
#include "bw_device.h"
#include "bw_internal.h"
#include "bw_seal.h"
#include "bw_ctx.h"
#include "bw_unpack.h"
#include "bw_restore.h"

using namespace bw;

namespace {

struct RkGap {
    uint64_t off, len;  // bytes [off, off + len) of the packfile buffer, the same place in both; len <= RS_PIECE
};

// one wave per gap: a byte-exact copy that loads nothing outside the gap
__global__ __launch_bounds__(256) void k_rekey_gaps(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                    const RkGap* __restrict__ gaps, uint64_t n) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < n; g += (uint64_t)gridDim.x * 4) {
        const RkGap x = gaps[g];
        rs_copy_piece<true>(src + x.off, dst + x.off, x.len, lane);
    }
}

void push_gap(std::vector<RkGap>& gaps, uint64_t lo, uint64_t hi) {
    for (; lo < hi; lo += RS_PIECE) gaps.push_back(RkGap{lo, std::min<uint64_t>(RS_PIECE, hi - lo)});
}

}  // namespace

extern "C" int bw_rekey_store_device(bw_restore* s, const uint8_t new_prk[32], uint8_t* d_out, uint8_t* entry_status,
                                     uint8_t* packfile_status) {
    if (!s || !new_prk) return BW_EINVAL;
    bw_ctx* c = s->c;
    const uint64_t n_pf = s->pf.size(), n_e = s->entries.size();
    if ((n_pf && (!d_out || !packfile_status)) || (n_e && !entry_status)) return BW_EINVAL;
    hipSetDevice(c->device);
    if (!n_pf) return BW_OK;

    // the in-range entries by (packfile, offset); two of one packfile must not overlap
    std::vector<uint64_t> ord;
    for (uint64_t e = 0; e < n_e; e++) {
        const bw_unpack_entry& en = s->entries[e];
        if (rs_range_ok(s->pf[en.packfile].size, s->pf[en.packfile].header_len, en.offset, en.length)) ord.push_back(e);
    }
    std::sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) {
        const bw_unpack_entry &x = s->entries[a], &y = s->entries[b];
        return x.packfile != y.packfile ? x.packfile < y.packfile : (x.offset != y.offset ? x.offset < y.offset : a < b);
    });
    for (uint64_t k = 1; k < ord.size(); k++) {
        const bw_unpack_entry &x = s->entries[ord[k - 1]], &y = s->entries[ord[k]];
        if (x.packfile == y.packfile && x.offset + BW_BLOB_NONCE_SIZE + x.length > y.offset) {
            c->err = "rekey: entries " + std::to_string(ord[k - 1]) + " and " + std::to_string(ord[k]) + " overlap";
            return BW_EINVAL;
        }
    }

    // the items (headers, then entries in that order) and the gaps between them
    std::vector<uint8_t> hdr_ok(n_pf);
    uint64_t n_hdr = 0;
    for (uint64_t p = 0; p < n_pf; p++) {
        const bw_packfile& f = s->pf[p];
        hdr_ok[p] = f.header_len >= BW_SEAL_TAG_BYTES && f.size >= 8 && f.header_len <= f.size - 8;
        n_hdr += hdr_ok[p];
    }
    const uint64_t m = n_hdr + ord.size();
    std::vector<uint64_t> n_off(ord.size()), s_off(m), s_len(m);
    std::vector<uint8_t> info(32 * m), nonces(12 * m), ok(m), ids(12 * n_pf);
    std::vector<uint32_t> info_lens(m);
    std::vector<RkGap> gaps;
    HIPCHK(c, hipMemcpyAsync(ids.data(), s->ids.p, 12 * n_pf, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t k = 0, at = 0;  // the next item, the next entry of ord
    for (uint64_t p = 0; p < n_pf; p++) {
        const bw_packfile& f = s->pf[p];
        uint64_t cur = 0;  // the packfile's bytes before cur are resealed or in a gap
        if (hdr_ok[p]) {
            s_off[k] = f.offset + 8;
            s_len[k] = f.header_len;
            memcpy(&info[32 * k], "header", 6);
            info_lens[k] = 6;
            memcpy(&nonces[12 * k], &ids[12 * p], 12);
            k++;
            push_gap(gaps, f.offset, f.offset + 8);
            cur = 8 + f.header_len;
        }
        for (; at < ord.size() && s->entries[ord[at]].packfile == p; at++) {
            const bw_unpack_entry& e = s->entries[ord[at]];
            const uint64_t sealed = 8 + f.header_len + e.offset + BW_BLOB_NONCE_SIZE;
            n_off[at] = f.offset + sealed - BW_BLOB_NONCE_SIZE;
            s_off[n_hdr + at] = f.offset + sealed;
            s_len[n_hdr + at] = e.length;
            memcpy(&info[32 * (n_hdr + at)], e.hash, 32);
            info_lens[n_hdr + at] = 32;
            push_gap(gaps, f.offset + cur, f.offset + sealed);
            cur = sealed + e.length;
        }
        push_gap(gaps, f.offset + cur, f.offset + f.size);
    }
    // the blob nonces come out of the packfiles, 12 bytes each (as check's AUTH pass fetches them)
    const uint64_t ne = ord.size(), ng = gaps.size();
    const uint64_t gap_at = (8 * ne + 12 * ne + 15) & ~15ull;
    if (int rc = ensure(c, s->rk_buf, gap_at + sizeof(RkGap) * ng + 16)) return rc;
    uint8_t* b = P<uint8_t>(s->rk_buf);
    if (ne) {
        HIPCHK(c, hipMemcpyAsync(b, n_off.data(), 8 * ne, hipMemcpyHostToDevice, c->stream));
        launch_gather12(c->stream, s->d_pf, (const uint64_t*)b, ne, b + 8 * ne);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&nonces[12 * n_hdr], b + 8 * ne, 12 * ne, hipMemcpyDeviceToHost, c->stream));
    }
    if (ng) HIPCHK(c, hipMemcpyAsync(b + gap_at, gaps.data(), sizeof(RkGap) * ng, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));

    // every check that can refuse the call is made before this writes its first byte
    if (int rc = bw_reseal_items(c, s->prk, new_prk, s->d_pf, s_off.data(), s_len.data(), m, info.data(), 32, info_lens.data(),
                                 nonces.data(), nullptr, d_out, s_off.data(), ok.data()))
        return rc;
    if (ng) {
        const uint64_t grid = std::min<uint64_t>((ng + 3) / 4, 4096);
        hipLaunchKernelGGL(k_rekey_gaps, dim3((unsigned)grid), dim3(256), 0, c->stream, s->d_pf, d_out, (const RkGap*)(b + gap_at),
                           ng);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }

    for (uint64_t e = 0; e < n_e; e++) entry_status[e] = BW_UNPACK_ERANGE;
    for (uint64_t j = 0; j < ne; j++) entry_status[ord[j]] = ok[n_hdr + j] ? BW_UNPACK_OK : BW_UNPACK_ETAG;
    k = 0;
    for (uint64_t p = 0; p < n_pf; p++) packfile_status[p] = !hdr_ok[p] ? BW_UNPACK_ERANGE : (ok[k++] ? BW_UNPACK_OK : BW_UNPACK_ETAG);
    return BW_OK;
}

// the new store is built in a device buffer of the table's extent; only the packfiles' ranges come back
extern "C" int bw_rekey_store(bw_restore* s, const uint8_t new_prk[32], uint8_t* out, uint8_t* entry_status,
                              uint8_t* packfile_status) {
    if (!s || !new_prk) return BW_EINVAL;
    bw_ctx* c = s->c;
    if (s->pf.empty()) return BW_OK;
    if (!out) return BW_EINVAL;
    hipSetDevice(c->device);
    uint64_t end = 0;
    for (const bw_packfile& f : s->pf) end = std::max(end, f.offset + f.size);
    DevBuf buf;
    if (int rc = ensure(c, buf, end + 16)) return rc;
    int rc = bw_rekey_store_device(s, new_prk, P<uint8_t>(buf), entry_status, packfile_status);
    for (const bw_packfile& f : s->pf)
        if (!rc && f.size && hipMemcpyAsync(out + f.offset, P<uint8_t>(buf) + f.offset, f.size, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            rc = BW_EHIP;
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = BW_EHIP;
    free_dev(buf);
    return rc;
}
