// bw_check.hip -- check (include/backuwup_gpu_pack.h, "check"): is a store sound before prune shrinks
// it, is a packfile a peer handed back the packfile that was sent.  The reference has no check.  Two
// parts over an open restore session: the structure (headers against index items in both directions
// and the layout of every blob section, from the session's device tables alone: k_check_scan,
// k_check_carry, k_check_items, k_check_item_dups, k_check_entries) and the data (every selected
// entry's bytes, either authenticated in place through bw_auth_device, or through the unpack chain
// with BW_UNPACK_VERIFY and the tree parser, rs_decode and k_rs_tree_parse unchanged).
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/backuwup_gpu.h"
#include "bw_device.h"
#include "bw_internal.h"
#include "bw_ctx.h"
#include "bw_restore.h"
#include "bw_prune.h"
#include "bw_check.h"

using namespace bw;

// ------------------------------------------------------------------ the segmented sum
// Inclusive segmented scan of CK_SCAN (value, head flag) pairs in LDS, Hillis-Steele:
// (v1, f1) + (v2, f2) = (f2 ? v2 : v1 + v2, f1 | f2).  Afterwards s_v[t] = the sum from the last head
// at or before t (or from 0), s_f[t] = whether there is one.
__device__ static inline void ck_seg_scan(uint64_t* s_v, uint32_t* s_f, uint32_t t) {
    __syncthreads();
    for (uint32_t d = 1; d < CK_SCAN; d <<= 1) {
        const uint64_t a = t >= d ? s_v[t - d] : 0;
        const uint32_t fa = t >= d ? s_f[t - d] : 0;
        __syncthreads();
        if (!s_f[t]) s_v[t] += a;
        s_f[t] |= fa;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(CK_SCAN) k_check_scan(const bw_unpack_entry* entries, uint64_t n, uint64_t* excl,
                                                        uint8_t* open, uint64_t* blk_sum, uint32_t* blk_head) {
    __shared__ uint64_t s_v[CK_SCAN];
    __shared__ uint32_t s_f[CK_SCAN];
    const uint32_t t = threadIdx.x;
    const uint64_t e = (uint64_t)blockIdx.x * CK_SCAN + t;
    const bool in = e < n;
    const uint64_t v = in ? BW_BLOB_NONCE_SIZE + entries[e].length : 0;
    s_v[t] = v;
    s_f[t] = in && (e == 0 || entries[e].packfile != entries[e - 1].packfile);
    ck_seg_scan(s_v, s_f, t);
    if (in) {
        excl[e] = s_v[t] - v;
        open[e] = !s_f[t];
    }
    if (t == CK_SCAN - 1) {  // the lanes past n add nothing and start nothing
        blk_sum[blockIdx.x] = s_v[t];
        blk_head[blockIdx.x] = s_f[t];
    }
}

// carry[b] = the segmented sum over the ranges before b: one workgroup, CK_SCAN ranges at a time
__global__ void __launch_bounds__(CK_SCAN) k_check_carry(const uint64_t* blk_sum, const uint32_t* blk_head, uint64_t nb,
                                                         uint64_t* carry) {
    __shared__ uint64_t s_v[CK_SCAN];
    __shared__ uint32_t s_f[CK_SCAN];
    const uint32_t t = threadIdx.x;
    uint64_t run = 0;  // the sum behind the last head of the ranges taken so far
    for (uint64_t lo = 0; lo < nb; lo += CK_SCAN) {
        const uint64_t b = lo + t;
        s_v[t] = b < nb ? blk_sum[b] : 0;
        s_f[t] = b < nb ? blk_head[b] : 0;
        ck_seg_scan(s_v, s_f, t);
        if (b < nb) carry[b] = t == 0 ? run : (s_f[t - 1] ? s_v[t - 1] : run + s_v[t - 1]);
        run = s_f[CK_SCAN - 1] ? s_v[CK_SCAN - 1] : run + s_v[CK_SCAN - 1];
        __syncthreads();  // the arrays are refilled by the next round
    }
}

void bw::launch_check_scan(hipStream_t st, const bw_unpack_entry* entries, uint64_t n, uint64_t* excl, uint8_t* open,
                           uint64_t* blk_sum, uint32_t* blk_head, uint64_t* carry) {
    if (!n) return;
    const uint64_t nb = (n + CK_SCAN - 1) / CK_SCAN;
    hipLaunchKernelGGL(k_check_scan, dim3((uint32_t)nb), dim3(CK_SCAN), 0, st, entries, n, excl, open, blk_sum, blk_head);
    hipLaunchKernelGGL(k_check_carry, dim3(1), dim3(CK_SCAN), 0, st, blk_sum, blk_head, nb, carry);
}

// ------------------------------------------------------------------ items against headers
// the entry item i names: the first entry with its hash in the packfile its id resolves to
__device__ static inline uint8_t ck_item_entry(const RsLocator& L, uint64_t i, uint32_t& e) {
    e = RS_EMPTY;
    const uint32_t pos = L.item_pos[i];
    if (pos == RS_EMPTY) return BW_RESTORE_ENOPACKFILE;
    if (L.entry_cap)
        e = rs_find(L.entry_tab, L.entry_cap, RsKeys{(const uint8_t*)L.entries, (uint32_t)sizeof(bw_unpack_entry), 32, 32},
                    L.items + i * BW_INDEX_ENTRY_BYTES, pos);
    return e == RS_EMPTY ? BW_RESTORE_EMISMATCH : BW_RESTORE_OK;
}

// Two items with the same hash and id name the same entry, and only such items do: the entry's owner
// is the lowest of them, whatever order the lanes run in.
__global__ void __launch_bounds__(256) k_check_items(RsLocator L, uint64_t n, uint32_t* owner, uint8_t* status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t e;
    const uint8_t st = ck_item_entry(L, i, e);
    status[i] = st;
    if (!st) atomicMin(&owner[e], (uint32_t)i);
}

__global__ void __launch_bounds__(256) k_check_item_dups(RsLocator L, uint64_t n, const uint32_t* owner, uint8_t* status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || status[i]) return;
    uint32_t e;
    ck_item_entry(L, i, e);
    if (owner[e] != (uint32_t)i) status[i] = BW_CHECK_IDUPLICATE;
}

void bw::launch_check_items(hipStream_t st, const RsLocator& loc, uint64_t n_items, uint32_t* owner, uint8_t* status) {
    if (n_items) hipLaunchKernelGGL(k_check_items, dim3((uint32_t)((n_items + 255) / 256)), dim3(256), 0, st, loc, n_items, owner, status);
}
void bw::launch_check_item_dups(hipStream_t st, const RsLocator& loc, uint64_t n_items, const uint32_t* owner, uint8_t* status) {
    if (n_items)
        hipLaunchKernelGGL(k_check_item_dups, dim3((uint32_t)((n_items + 255) / 256)), dim3(256), 0, st, loc, n_items, owner, status);
}

// ------------------------------------------------------------------ entries
__device__ static inline uint64_t ck_wave_sum(uint64_t v) {
    for (int d = 32; d; d >>= 1) v += __shfl_down((unsigned long long)v, d);
    return v;  // lane 0 holds the sum
}

// One lane per entry.  The per-packfile sums as k_prune_account takes them: a wave that lies in one
// packfile adds each sum once, by lane 0; a wave that spans packfiles adds lane by lane.
__global__ void __launch_bounds__(256) k_check_entries(RsLocator L, uint64_t n, const PrPackfile* pf, const uint64_t* excl,
                                                       const uint8_t* open, const uint64_t* carry, const uint32_t* owner,
                                                       uint8_t* flags, uint64_t* sums) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = e < n;
    uint32_t p = 0, fl = 0;
    uint64_t v[CK_S_COUNT] = {0, 0, 0, 0, 0, 0};
    if (in) {
        const bw_unpack_entry& en = L.entries[e];
        p = en.packfile;
        if (!rs_range_ok(pf[p].size, pf[p].header_len, en.offset, en.length)) fl |= BW_CHECK_E_RANGE;
        if (en.offset != excl[e] + (open[e] ? carry[e / CK_SCAN] : 0)) fl |= BW_CHECK_E_ORDER;
        // the table holds the lowest entry of (packfile, hash): any other one is hidden behind it
        const uint32_t first = rs_find(L.entry_tab, L.entry_cap, RsKeys{(const uint8_t*)L.entries, (uint32_t)sizeof(bw_unpack_entry), 32, 32},
                                       en.hash, p);
        if (first != (uint32_t)e) fl |= BW_CHECK_E_SHADOWED;
        else if (owner[e] == RS_EMPTY) fl |= BW_CHECK_E_UNINDEXED;
        flags[e] = (uint8_t)fl;
        v[CK_S_ENTRIES] = 1;
        v[CK_S_RANGE] = fl & BW_CHECK_E_RANGE ? 1 : 0;
        v[CK_S_ORDER] = fl & BW_CHECK_E_ORDER ? 1 : 0;
        v[CK_S_UNINDEXED] = fl & BW_CHECK_E_UNINDEXED ? 1 : 0;
        v[CK_S_SHADOWED] = fl & BW_CHECK_E_SHADOWED ? 1 : 0;
        v[CK_S_CLAIMED] = BW_BLOB_NONCE_SIZE + en.length;
    }
    if (!__any(in)) return;
    const uint32_t p0 = __shfl(p, 0);  // lane 0 holds the wave's lowest entry
    unsigned long long* s = (unsigned long long*)sums;
    if (__all(!in || p == p0)) {
#pragma unroll
        for (int k = 0; k < CK_S_COUNT; k++) {
            const uint64_t a = ck_wave_sum(v[k]);
            if ((threadIdx.x & 63) == 0 && a) atomicAdd(&s[(uint64_t)CK_S_COUNT * p0 + k], a);
        }
    } else if (in) {
#pragma unroll
        for (int k = 0; k < CK_S_COUNT; k++)
            if (v[k]) atomicAdd(&s[(uint64_t)CK_S_COUNT * p + k], v[k]);
    }
}

void bw::launch_check_entries(hipStream_t st, const RsLocator& loc, uint64_t n, const PrPackfile* pf, const uint64_t* excl,
                              const uint8_t* open, const uint64_t* carry, const uint32_t* owner, uint8_t* flags, uint64_t* sums) {
    if (n)
        hipLaunchKernelGGL(k_check_entries, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, loc, n, pf, excl, open, carry, owner,
                           flags, sums);
}

// ------------------------------------------------------------------ bw_check_structure
static uint64_t ck_up16(uint64_t v) { return (v + 15) & ~15ull; }

extern "C" int bw_check_structure(bw_restore* s, uint8_t* entry_flags, uint8_t* item_status, bw_check_packfile_stat* stats,
                                  bw_check_counts* counts) {
    if (!s || !counts) return BW_EINVAL;
    const uint64_t n_e = s->entries.size(), n_pf = s->pf.size(), n_i = s->n_items;
    if ((n_e && !entry_flags) || (n_i && !item_status) || (n_pf && !stats)) return BW_EINVAL;
    bw_ctx* c = s->c;
    for (uint64_t e = 1; e < n_e; e++)
        if (s->entries[e].packfile < s->entries[e - 1].packfile) {
            c->err = "check: the session's entries are not in packfile order at entry " + std::to_string(e);
            return BW_EINVAL;
        }
    hipSetDevice(c->device);
    memset(counts, 0, sizeof(*counts));

    // one buffer: excl | carry | blk_sum | sums | packfile sizes | owner | blk_head | open | flags | item statuses
    const uint64_t nb = (n_e + CK_SCAN - 1) / CK_SCAN, sum_bytes = 8 * CK_S_COUNT * n_pf;
    const uint64_t at_excl = 0, at_carry = at_excl + ck_up16(8 * n_e), at_bsum = at_carry + ck_up16(8 * nb),
                   at_sums = at_bsum + ck_up16(8 * nb), at_pf = at_sums + ck_up16(sum_bytes),
                   at_owner = at_pf + ck_up16(n_pf * sizeof(PrPackfile)), at_bhead = at_owner + ck_up16(4 * n_e),
                   at_open = at_bhead + ck_up16(4 * nb), at_flags = at_open + ck_up16(n_e), at_ist = at_flags + ck_up16(n_e),
                   total = at_ist + ck_up16(n_i);
    if (int rc = ensure(c, s->ck_buf, total + 16)) return rc;
    uint8_t* b = P<uint8_t>(s->ck_buf);
    const std::vector<PrPackfile> hpf = rs_packfile_table(s);
    if (n_pf) {
        HIPCHK(c, hipMemsetAsync(b + at_sums, 0, sum_bytes, c->stream));
        HIPCHK(c, hipMemcpyAsync(b + at_pf, hpf.data(), n_pf * sizeof(PrPackfile), hipMemcpyHostToDevice, c->stream));
    }
    if (n_e) HIPCHK(c, hipMemsetAsync(b + at_owner, 0xff, 4 * n_e, c->stream));

    const RsLocator loc = rs_locator(s);
    uint32_t* owner = (uint32_t*)(b + at_owner);
    launch_check_scan(c->stream, loc.entries, n_e, (uint64_t*)(b + at_excl), b + at_open, (uint64_t*)(b + at_bsum),
                      (uint32_t*)(b + at_bhead), (uint64_t*)(b + at_carry));
    launch_check_items(c->stream, loc, n_i, owner, b + at_ist);
    launch_check_item_dups(c->stream, loc, n_i, owner, b + at_ist);
    launch_check_entries(c->stream, loc, n_e, (const PrPackfile*)(b + at_pf), (const uint64_t*)(b + at_excl), b + at_open,
                         (const uint64_t*)(b + at_carry), owner, b + at_flags, (uint64_t*)(b + at_sums));
    HIPCHK(c, hipGetLastError());
    std::vector<uint64_t> sums(CK_S_COUNT * n_pf);
    if (n_e) HIPCHK(c, hipMemcpyAsync(entry_flags, b + at_flags, n_e, hipMemcpyDeviceToHost, c->stream));
    if (n_i) HIPCHK(c, hipMemcpyAsync(item_status, b + at_ist, n_i, hipMemcpyDeviceToHost, c->stream));
    if (n_pf) HIPCHK(c, hipMemcpyAsync(sums.data(), b + at_sums, sum_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));

    for (uint64_t p = 0; p < n_pf; p++) {
        const uint64_t* v = &sums[CK_S_COUNT * p];
        bw_check_packfile_stat& st = stats[p];
        st.n_entries = v[CK_S_ENTRIES];
        st.n_range = v[CK_S_RANGE];
        st.n_order = v[CK_S_ORDER];
        st.n_unindexed = v[CK_S_UNINDEXED];
        st.n_shadowed = v[CK_S_SHADOWED];
        st.claimed_bytes = v[CK_S_CLAIMED];
        const uint64_t base = 8 + hpf[p].header_len;
        st.section_bytes = hpf[p].size >= base ? hpf[p].size - base : 0;
        st.tail = (int64_t)(st.section_bytes - st.claimed_bytes);
        counts->n_entries += st.n_entries;
        counts->n_range += st.n_range;
        counts->n_order += st.n_order;
        counts->n_unindexed += st.n_unindexed;
        counts->n_shadowed += st.n_shadowed;
        counts->claimed_bytes += st.claimed_bytes;
        counts->section_bytes += st.section_bytes;
        if (!st.n_range && !st.n_order && !st.n_unindexed && !st.n_shadowed && !st.tail) counts->n_packfiles_clean++;
    }
    for (uint64_t i = 0; i < n_i; i++) switch (item_status[i]) {
            case BW_RESTORE_OK: counts->n_items_ok++; break;
            case BW_RESTORE_ENOPACKFILE: counts->n_items_nopackfile++; break;
            case BW_RESTORE_EMISMATCH: counts->n_items_mismatch++; break;
            default: counts->n_items_duplicate++; break;
        }
    return BW_OK;
}

// ------------------------------------------------------------------ bw_check_data
// AUTH: every chosen blob's tag recomputed where the blob lies; one bw_auth_device call
static int ck_auth(bw_restore* s, const std::vector<uint64_t>& idx, uint8_t* status) {
    bw_ctx* c = s->c;
    const uint64_t m = idx.size();
    std::vector<uint64_t> n_off(m), s_off(m), s_len(m);
    std::vector<uint8_t> hashes(32 * m), nonces(12 * m), ok(m);
    for (uint64_t k = 0; k < m; k++) {
        const bw_unpack_entry& e = s->entries[idx[k]];
        const BlobPlace at = blob_place(s->pf[e.packfile], e);
        n_off[k] = at.nonce;
        s_off[k] = at.sealed;
        s_len[k] = e.length;
        memcpy(&hashes[32 * k], e.hash, 32);
    }
    if (int rc = rs_fetch_nonces(c, s->d_pf, n_off.data(), m, s->ck_buf, nonces.data())) return rc;
    if (int rc = bw_auth_device(c, s->prk, s->d_pf, s_off.data(), s_len.data(), m, hashes.data(), 32, nonces.data(), ok.data()))
        return rc;
    for (uint64_t k = 0; k < m; k++) status[idx[k]] = ok[k] ? BW_UNPACK_OK : BW_UNPACK_ETAG;
    return BW_OK;
}

// FULL: the unpack chain with BW_UNPACK_VERIFY, `slots` blobs at a time; tree blobs that pass are parsed in their slots
static int ck_full(bw_restore* s, const std::vector<uint64_t>& idx, uint8_t* status) {
    bw_ctx* c = s->c;
    std::vector<uint64_t> eidx;
    std::vector<uint8_t> bst;
    std::vector<RsTreeHdr> hd;
    for (uint64_t lo = 0; lo < idx.size(); lo += s->slots) {
        const uint64_t m = std::min<uint64_t>(s->slots, idx.size() - lo);
        eidx.assign(idx.begin() + lo, idx.begin() + lo + m);
        RsTables t;
        if (int rc = rs_tree_decode(s, eidx, BW_UNPACK_VERIFY, m, t, bst)) return rc;
        bool trees = false;
        for (uint64_t k = 0; k < m; k++) {
            status[eidx[k]] = bst[k];
            trees = trees || (!bst[k] && s->entries[eidx[k]].kind == BW_BLOB_TREE);
        }
        // a blob the chain refused has length 0 on the device: the parser reads nothing of it
        if (trees)
            if (int rc = rs_tree_parse(s, t, m, &hd)) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));  // the slots and the tables are reused by the next sub-batch
        if (trees)
            for (uint64_t k = 0; k < m; k++)
                if (!bst[k] && s->entries[eidx[k]].kind == BW_BLOB_TREE && hd[k].status) status[eidx[k]] = (uint8_t)hd[k].status;
    }
    return BW_OK;
}

extern "C" int bw_check_data(bw_restore* s, uint32_t mode, const uint8_t* select, uint8_t* status) {
    if (!s || (mode != BW_CHECK_AUTH && mode != BW_CHECK_FULL)) return BW_EINVAL;
    const uint64_t n_e = s->entries.size();
    if (n_e && !status) return BW_EINVAL;
    hipSetDevice(s->c->device);
    std::vector<uint64_t> idx;
    for (uint64_t e = 0; e < n_e; e++) {
        const bw_unpack_entry& en = s->entries[e];
        if (select && !select[e]) {
            status[e] = BW_CHECK_SKIPPED;
        } else if (!rs_range_ok(s->pf[en.packfile].size, s->pf[en.packfile].header_len, en.offset, en.length)) {
            status[e] = BW_UNPACK_ERANGE;
        } else {
            status[e] = BW_UNPACK_OK;
            idx.push_back(e);
        }
    }
    if (idx.empty()) return BW_OK;
    return mode == BW_CHECK_AUTH ? ck_auth(s, idx, status) : ck_full(s, idx, status);
}
