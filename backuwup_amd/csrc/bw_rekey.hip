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
#include "bw_restore.h"

using namespace bw;

namespace {

// one wave per gap: a byte-exact copy that loads nothing outside the gap
__global__ __launch_bounds__(256) void k_rekey_gaps(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                    const RkGap* __restrict__ gaps, uint64_t n) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < n; g += (uint64_t)gridDim.x * 4) {
        const RkGap x = gaps[g];
        rs_copy_piece<true>(src + x.off, dst + x.off, x.len, lane);
    }
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

    // what is resealed and what is copied as it is; two in-range entries of one packfile must not overlap
    RekeyLayout L;
    if (int rc = rekey_layout(s->pf.data(), n_pf, s->entries.data(), n_e, L, c->err)) return rc;
    const uint64_t n_hdr = L.n_hdr, ne = L.ord.size(), ng = L.gaps.size(), m = n_hdr + ne;
    std::vector<uint8_t> nonces(12 * m), ok(m), ids(12 * n_pf);
    // a header's nonce is its packfile's id
    HIPCHK(c, hipMemcpyAsync(ids.data(), s->ids.p, 12 * n_pf, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint64_t p = 0, k = 0; p < n_pf; p++)
        if (L.hdr_ok[p]) memcpy(&nonces[12 * k++], &ids[12 * p], 12);
    // a blob's nonce lies in front of it; the gap list goes up behind the fetch's scratch
    const uint64_t gap_at = (20 * ne + 15) & ~15ull;
    if (int rc = ensure(c, s->rk_buf, gap_at + sizeof(RkGap) * ng + 16)) return rc;
    const RkGap* d_gaps = (const RkGap*)(P<uint8_t>(s->rk_buf) + gap_at);
    if (ng) HIPCHK(c, hipMemcpyAsync((void*)d_gaps, L.gaps.data(), sizeof(RkGap) * ng, hipMemcpyHostToDevice, c->stream));
    if (int rc = rs_fetch_nonces(c, s->d_pf, L.n_off.data(), ne, s->rk_buf, nonces.data() + 12 * n_hdr)) return rc;

    // every check that can refuse the call is made before this writes its first byte
    if (int rc = bw_reseal_items(c, s->prk, new_prk, s->d_pf, L.s_off.data(), L.s_len.data(), m, L.info.data(), 32, L.info_lens.data(),
                                 nonces.data(), nullptr, d_out, L.s_off.data(), ok.data()))
        return rc;
    if (ng) {
        const uint64_t grid = std::min<uint64_t>((ng + 3) / 4, 4096);
        hipLaunchKernelGGL(k_rekey_gaps, dim3((unsigned)grid), dim3(256), 0, c->stream, s->d_pf, d_out, d_gaps, ng);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }

    for (uint64_t e = 0; e < n_e; e++) entry_status[e] = BW_UNPACK_ERANGE;
    for (uint64_t j = 0; j < ne; j++) entry_status[L.ord[j]] = ok[n_hdr + j] ? BW_UNPACK_OK : BW_UNPACK_ETAG;
    for (uint64_t p = 0, k = 0; p < n_pf; p++) packfile_status[p] = !L.hdr_ok[p] ? BW_UNPACK_ERANGE : (ok[k++] ? BW_UNPACK_OK : BW_UNPACK_ETAG);
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
    const uint64_t end = store_extent(s->pf.data(), s->pf.size());
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
