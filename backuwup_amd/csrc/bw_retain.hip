// bw_retain.hip -- retain (include/backuwup_gpu_pack.h, "retain"): which snapshots keep each blob alive,
// and what forgetting a set of them frees.  The reference cannot ask it.  One walk for all roots:
//   the mark   impact's walk under the RtReach policy (im_walk, bw_impact.hip: each distinct tree blob through
//              the unpack chain once, an edge for every reference that locates), then a set of roots per
//              entry pushed down the edges: k_rt_seed (a root's bit into the entry it locates to),
//              k_rt_propagate (the tree edges to their least fixed point, one forward sweep per launch
//              series, repeated by the host until a sweep changes nothing; then the leaf edges once),
//              k_rt_stats (per root what it reaches, what it alone holds, what of it is damaged)
//   the drop   k_rt_drop: for each question "forget these roots" the live vector and the per-packfile
//              sums bw_prune_mark over the kept roots would give, with no tree read
// All sums are integers: every result is exact whatever the order of the atomics.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/backuwup_gpu.h"
#include "bw_device.h"
#include "bw_internal.h"
#include "bw_ctx.h"
#include "bw_restore.h"
#include "bw_retain.h"

using namespace bw;

static_assert(RT_MAX_ROOTS == BW_RETAIN_MAX_ROOTS, "the host header's limit is the ABI's");
static_assert(sizeof(bw_retain_root) == 8 * RT_SUMS + 8, "five sums, then status and pad");
static_assert(sizeof(bw_retain_freed) == 32 && sizeof(bw_prune_packfile_stat) == 32, "four sums each");

__device__ static inline uint64_t rt_wave_sum(uint64_t v) {
    for (int d = 32; d; d >>= 1) v += __shfl_down((unsigned long long)v, d);
    return v;  // lane 0 holds the sum
}

// ------------------------------------------------------------------ the mark
// One lane per root: its bit into reach, and into open when it locates to a Tree entry.  The walk's root
// kernel appends no edge, so the roots are seeded here; the walk itself recorded the error.
__global__ void __launch_bounds__(256) k_rt_seed(RsLocator loc, const uint8_t* roots, uint64_t n, uint64_t W, uint64_t* reach,
                                                 uint64_t* open, bw_retain_root* per_root) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t e;
    const uint8_t st = rs_locate_one(loc, roots + 32 * i, e);
    if (st) {
        per_root[i].status = st;
        return;
    }
    const unsigned long long bit = 1ull << (i & 63);
    atomicOr((unsigned long long*)&reach[e * W + (i >> 6)], bit);
    if (loc.entries[e].kind == BW_BLOB_TREE) atomicOr((unsigned long long*)&open[e * W + (i >> 6)], bit);
    else per_root[i].status = BW_RESTORE_ENOTTREE;
}

// One lane per (edge, word) of the edges [lo, hi): the parent's open word gives the child's reach word the
// bits it lacks, and on a tree edge its open word too.  The bits only ever grow, so a stale read costs a
// sweep, never an answer.
__global__ void __launch_bounds__(256) k_rt_propagate(uint64_t* reach, uint64_t* open, const ImEdge* edges, uint64_t lo, uint64_t hi,
                                                      uint64_t W, int tree, uint64_t* changed) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (hi - lo) * W) return;
    const ImEdge ed = edges[lo + i / W];
    const uint64_t w = i % W, child = ed.child & ~IM_EDGE_SELF_ONLY;
    const uint64_t pv = __atomic_load_n(&open[(uint64_t)ed.parent * W + w], __ATOMIC_RELAXED);
    if (!pv) return;
    bool did = false;
    const uint64_t mr = pv & ~__atomic_load_n(&reach[child * W + w], __ATOMIC_RELAXED);
    if (mr) {
        atomicOr((unsigned long long*)&reach[child * W + w], (unsigned long long)mr);
        did = true;
    }
    if (tree) {
        const uint64_t mo = pv & ~__atomic_load_n(&open[child * W + w], __ATOMIC_RELAXED);
        if (mo) {
            atomicOr((unsigned long long*)&open[child * W + w], (unsigned long long)mo);
            did = true;
        }
    }
    if (did) *changed = 1;
}

// Workgroup (b, y): entries b * 256 + t, word y of their masks.  64 roots x RT_SUMS sums in LDS; each lane
// walks the set bits of its word, the workgroup flushes once.  Word 0's workgroups also write the damaged
// bytes and add up the reached and orphan totals.
__global__ void __launch_bounds__(256) k_rt_stats(const bw_unpack_entry* entries, uint64_t n, uint64_t W, uint64_t n_roots,
                                                  const uint64_t* reach, const uint32_t* bits, uint8_t* damaged,
                                                  bw_retain_root* per_root, uint64_t* totals) {
    __shared__ unsigned long long sums[64 * RT_SUMS];
    for (uint32_t k = threadIdx.x; k < 64 * RT_SUMS; k += 256) sums[k] = 0;
    __syncthreads();
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    const bool in = e < n;
    uint64_t bytes = 0, pop = 0;
    if (in) {
        bytes = BW_BLOB_NONCE_SIZE + entries[e].length;
        for (uint64_t w = 0; w < W; w++) pop += __popcll((unsigned long long)reach[e * W + w]);
        const bool dmg = (bits[e >> 2] >> (8 * (uint32_t)(e & 3))) & (IM_SELF | IM_BELOW);
        if (y == 0) damaged[e] = dmg ? 1 : 0;
        uint64_t word = reach[e * W + y];
        while (word) {
            const uint32_t b = (uint32_t)__ffsll((unsigned long long)word) - 1;
            word &= word - 1;
            unsigned long long* s = &sums[b * RT_SUMS];
            atomicAdd(&s[0], 1ull);
            atomicAdd(&s[1], (unsigned long long)bytes);
            if (pop == 1) {
                atomicAdd(&s[2], 1ull);
                atomicAdd(&s[3], (unsigned long long)bytes);
            }
            if (dmg) atomicAdd(&s[4], 1ull);
        }
    }
    if (y == 0) {  // uniform over the workgroup
        const bool r = in && pop, o = in && !pop;
        const uint64_t a = rt_wave_sum(r ? 1 : 0), b = rt_wave_sum(r ? bytes : 0), c = rt_wave_sum(o ? 1 : 0), d = rt_wave_sum(o ? bytes : 0);
        if ((threadIdx.x & 63) == 0) {
            unsigned long long* t = (unsigned long long*)totals;
            if (a) atomicAdd(&t[RT_T_REACHED_BLOBS], (unsigned long long)a);
            if (b) atomicAdd(&t[RT_T_REACHED_BYTES], (unsigned long long)b);
            if (c) atomicAdd(&t[RT_T_ORPHAN_BLOBS], (unsigned long long)c);
            if (d) atomicAdd(&t[RT_T_ORPHAN_BYTES], (unsigned long long)d);
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < 64 * RT_SUMS; k += 256) {
        const uint64_t r = 64 * y + k / RT_SUMS;
        if (r < n_roots && sums[k]) atomicAdd((unsigned long long*)&per_root[r] + k % RT_SUMS, sums[k]);
    }
}

// ------------------------------------------------------------------ the drop
// Workgroup (b, q): entries b * 256 + t against drop set q.  Entries come in packfile order, so a wave
// usually lies in one packfile: its sums then take one atomic each, by lane 0 (k_prune_account's shape); a
// wave that spans packfiles adds lane by lane.  live may be null.
__global__ void __launch_bounds__(256) k_rt_drop(const bw_unpack_entry* entries, uint64_t n, uint64_t n_pf, uint64_t W,
                                                 const uint64_t* masks, const uint64_t* drop, uint8_t* live, uint64_t* stats,
                                                 uint64_t* freed) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
    bool in = e < n;
    uint32_t p = 0;
    uint64_t bytes = 0;
    bool lv = false, any = false;
    if (in) {
        p = entries[e].packfile;
        bytes = BW_BLOB_NONCE_SIZE + entries[e].length;
        for (uint64_t w = 0; w < W; w++) {
            const uint64_t m = masks[e * W + w];
            any = any || m;
            lv = lv || (m & ~drop[q * W + w]);
        }
        if (live) live[q * n + e] = lv ? 1 : 0;
        in = p < n_pf;  // the session's tables say so; a sum has a place only then
    }
    if (!__any(in)) return;
    const bool fr = in && any && !lv, kept = in && lv;
    const uint64_t fa = rt_wave_sum(fr ? 1 : 0), fb = rt_wave_sum(fr ? bytes : 0), la = rt_wave_sum(kept ? 1 : 0), lb = rt_wave_sum(kept ? bytes : 0);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* f = (unsigned long long*)freed + 4 * q;
        if (fa) atomicAdd(&f[0], (unsigned long long)fa);
        if (fb) atomicAdd(&f[1], (unsigned long long)fb);
        if (la) atomicAdd(&f[2], (unsigned long long)la);
        if (lb) atomicAdd(&f[3], (unsigned long long)lb);
    }
    const uint32_t p0 = __shfl(p, 0);  // lane 0 holds the wave's lowest entry
    unsigned long long* s = (unsigned long long*)stats + 4 * q * n_pf;
    if (__all(!in || p == p0) && __shfl((int)in, 0)) {
        const uint64_t c = rt_wave_sum(in ? 1 : 0), d = rt_wave_sum(in ? bytes : 0);
        if ((threadIdx.x & 63) == 0) {
            if (la) atomicAdd(&s[4ull * p0], (unsigned long long)la);
            if (lb) atomicAdd(&s[4ull * p0 + 1], (unsigned long long)lb);
            atomicAdd(&s[4ull * p0 + 2], (unsigned long long)c);
            atomicAdd(&s[4ull * p0 + 3], (unsigned long long)d);
        }
    } else if (in) {
        if (lv) {
            atomicAdd(&s[4ull * p], 1ull);
            atomicAdd(&s[4ull * p + 1], (unsigned long long)bytes);
        }
        atomicAdd(&s[4ull * p + 2], 1ull);
        atomicAdd(&s[4ull * p + 3], (unsigned long long)bytes);
    }
}

static int rt_refuse(bw_ctx* c, const char* why) { return wk_refuse(c, "retain", why); }

// One walk with a device error list of dev_cap <= err_cap records; *n_dev_out = the errors the kernels met.
static int rt_mark_once(bw_restore* s, const uint8_t* roots, uint64_t n_roots, uint32_t flags, uint64_t* masks, uint8_t* damaged,
                        bw_retain_root* per_root, bw_retain_counts* counts, bw_prune_error* errs, uint64_t err_cap,
                        uint64_t dev_cap, uint64_t* n_dev_out) {
    const uint64_t n_e = s->entries.size(), W = rt_words(n_roots);
    bw_ctx* c = s->c;
    memset(counts, 0, sizeof(*counts));
    ImWalked wd;
    if (int rc = im_walk<RtReach>(s, roots, n_roots, nullptr, flags, dev_cap, 0, &s->rt[RT_B_LEAF], wd)) return rc;
    const ImMark& w = wd.w;

    const uint64_t mask_bytes = 8 * n_e * W, root_bytes = n_roots * sizeof(bw_retain_root);
    if (int rc = ensure(c, s->rt[RT_B_REACH], mask_bytes + 16)) return rc;
    if (int rc = ensure(c, s->rt[RT_B_OPEN], mask_bytes + 16)) return rc;
    if (int rc = ensure(c, s->rt[RT_B_ROOT], root_bytes + 8 * RT_T_COUNT + 16)) return rc;
    if (int rc = ensure(c, s->rt[RT_B_DMG], n_e + 16)) return rc;
    uint64_t *d_reach = P<uint64_t>(s->rt[RT_B_REACH]), *d_open = P<uint64_t>(s->rt[RT_B_OPEN]);
    bw_retain_root* d_root = P<bw_retain_root>(s->rt[RT_B_ROOT]);
    uint64_t* d_tot = (uint64_t*)(P<uint8_t>(s->rt[RT_B_ROOT]) + root_bytes);
    HIPCHK(c, hipMemsetAsync(d_reach, 0, mask_bytes + 16, c->stream));
    HIPCHK(c, hipMemsetAsync(d_open, 0, mask_bytes + 16, c->stream));
    HIPCHK(c, hipMemsetAsync(d_root, 0, root_bytes + 8 * RT_T_COUNT, c->stream));
    if (n_roots) hipLaunchKernelGGL(k_rt_seed, wk_grid(n_roots), dim3(256), 0, c->stream, w.loc, wd.d_roots, n_roots, W, d_reach, d_open, d_root);
    HIPCHK(c, hipGetLastError());

    // the root sets to their least fixed point: sweeps over the tree edges, earliest level first, until one changes nothing
    uint64_t n_sweeps = 0, changed = 1;
    const auto ranges = rt_sweep(wd.levels);
    while (changed) {
        if (n_sweeps > n_e + 1) return rt_refuse(c, "more sweeps than the store has entries");  // a sweep that changes something carries a set one entry further
        HIPCHK(c, hipMemsetAsync(&w.ctr[IM_C_CHANGED], 0, 8, c->stream));
        for (const auto& r : ranges)
            hipLaunchKernelGGL(k_rt_propagate, wk_grid((r.second - r.first) * W), dim3(256), 0, c->stream, d_reach, d_open, w.edges,
                               r.first, r.second, W, 1, &w.ctr[IM_C_CHANGED]);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&changed, &w.ctr[IM_C_CHANGED], 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        n_sweeps++;
    }
    // the leaf edges pass nothing on: one pass now that every open set is final
    const uint64_t n_leaf = wd.ctr[IM_C_LEAF];
    if (n_leaf)
        hipLaunchKernelGGL(k_rt_propagate, wk_grid(n_leaf * W), dim3(256), 0, c->stream, d_reach, d_open, w.leaf, 0, n_leaf, W, 0,
                           &w.ctr[IM_C_CHANGED]);
    if (n_e)
        hipLaunchKernelGGL(k_rt_stats, dim3((uint32_t)((n_e + 255) / 256), (uint32_t)W), dim3(256), 0, c->stream,
                           P<bw_unpack_entry>(s->d_entries), n_e, W, n_roots, d_reach, w.bits, P<uint8_t>(s->rt[RT_B_DMG]), d_root, d_tot);
    HIPCHK(c, hipGetLastError());

    // results: reach is the public mask as it stands (no bit at or past n_roots was ever seeded)
    uint64_t tot[RT_T_COUNT];
    if (n_e) HIPCHK(c, hipMemcpyAsync(masks, d_reach, mask_bytes, hipMemcpyDeviceToHost, c->stream));
    if (n_e) HIPCHK(c, hipMemcpyAsync(damaged, s->rt[RT_B_DMG].p, n_e, hipMemcpyDeviceToHost, c->stream));
    if (n_roots) HIPCHK(c, hipMemcpyAsync(per_root, d_root, root_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    counts->n_trees_expanded = wd.ctr[IM_C_EXPANDED];
    counts->n_levels = wd.levels.n_levels();
    counts->n_edges = wd.levels.n_edges() + n_leaf;
    counts->n_sweeps = n_sweeps;
    counts->reached_blobs = tot[RT_T_REACHED_BLOBS];
    counts->reached_bytes = tot[RT_T_REACHED_BYTES];
    counts->orphan_blobs = tot[RT_T_ORPHAN_BLOBS];
    counts->orphan_bytes = tot[RT_T_ORPHAN_BYTES];
    return im_errors_out(s, wd, "retain", errs, err_cap, dev_cap, n_dev_out, &counts->n_errors);
}

extern "C" int bw_retain_mark(bw_restore* s, const uint8_t* roots, uint64_t n_roots, uint32_t flags, uint64_t* masks,
                              uint8_t* damaged, bw_retain_root* per_root, bw_retain_counts* counts, bw_prune_error* errs,
                              uint64_t err_cap) {
    if (n_roots > RT_MAX_ROOTS) return s ? wk_too_large(s->c, "retain", "more than 4096 roots") : BW_ENOMEM;
    if (!s || !counts || (flags & ~BW_UNPACK_VERIFY) || (n_roots && (!roots || !per_root)) || (err_cap && !errs))
        return BW_EINVAL;
    if (!s->entries.empty() && (!masks || !damaged)) return BW_EINVAL;
    hipSetDevice(s->c->device);
    if (s->entries.size() >= IM_MAX_ENTRIES) return wk_too_large(s->c, "retain", "2^31 entries or more");
    // the device's error list and the second walk when it was too short: bw_prune_mark's rule
    uint64_t dev_cap = std::min<uint64_t>(err_cap, IM_ERR_DEVICE);
    for (;;) {
        uint64_t n_dev = 0;
        const int rc = rt_mark_once(s, roots, n_roots, flags, masks, damaged, per_root, counts, errs, err_cap, dev_cap, &n_dev);
        if ((rc != BW_OK && rc != BW_ENOSPC) || n_dev <= dev_cap || dev_cap >= err_cap) return rc;
        dev_cap = std::min(err_cap, n_dev);
    }
}

extern "C" int bw_retain_drop(bw_restore* s, const uint64_t* masks, uint64_t n_roots, const uint64_t* drop, uint64_t n_sets,
                              uint8_t* live, bw_prune_packfile_stat* stats, bw_retain_freed* freed) {
    if (n_roots > RT_MAX_ROOTS) return s ? wk_too_large(s->c, "retain", "more than 4096 roots") : BW_ENOMEM;
    if (!s || (n_sets && (!drop || !freed)) || (!s->entries.empty() && !masks)) return BW_EINVAL;
    bw_ctx* c = s->c;
    hipSetDevice(c->device);
    const uint64_t n_e = s->entries.size(), n_pf = s->pf.size(), W = rt_words(n_roots);
    if (n_e >= IM_MAX_ENTRIES) return wk_too_large(c, "retain", "2^31 entries or more");
    if (rt_foreign(masks, n_e, W, n_roots) != ~0ull || rt_foreign(drop, n_sets, W, n_roots) != ~0ull) {
        c->err = "retain: a mask or a drop set holds a bit of a root that was not given";
        return BW_EINVAL;
    }
    if (!n_sets) return BW_OK;
    const uint64_t mask_bytes = 8 * n_e * W, per = std::max<uint64_t>(1, std::min({n_sets, RT_DROP_BATCH_SETS, RT_DROP_BATCH_BYTES / std::max<uint64_t>(n_e, 1)}));
    const uint64_t drop_at = (mask_bytes + 15) & ~15ull, stat_bytes = 32 * per * n_pf, freed_at = stat_bytes;
    if (int rc = ensure(c, s->rt[RT_B_MASK], drop_at + 8 * per * W + 16)) return rc;
    if (int rc = ensure(c, s->rt[RT_B_LIVE], (live ? per * n_e : 0) + 16)) return rc;
    if (int rc = ensure(c, s->rt[RT_B_STAT], freed_at + 32 * per + 16)) return rc;
    uint8_t *d_mask = P<uint8_t>(s->rt[RT_B_MASK]), *d_stat = P<uint8_t>(s->rt[RT_B_STAT]);
    if (n_e) HIPCHK(c, hipMemcpyAsync(d_mask, masks, mask_bytes, hipMemcpyHostToDevice, c->stream));
    for (uint64_t q0 = 0; q0 < n_sets; q0 += per) {
        const uint64_t m = std::min(per, n_sets - q0);
        HIPCHK(c, hipMemcpyAsync(d_mask + drop_at, drop + q0 * W, 8 * m * W, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(d_stat, 0, freed_at + 32 * per, c->stream));
        if (n_e)
            hipLaunchKernelGGL(k_rt_drop, dim3((uint32_t)((n_e + 255) / 256), (uint32_t)m), dim3(256), 0, c->stream,
                               P<bw_unpack_entry>(s->d_entries), n_e, n_pf, W, (const uint64_t*)d_mask, (const uint64_t*)(d_mask + drop_at),
                               live ? P<uint8_t>(s->rt[RT_B_LIVE]) : nullptr, (uint64_t*)d_stat, (uint64_t*)(d_stat + freed_at));
        HIPCHK(c, hipGetLastError());
        if (live && n_e) HIPCHK(c, hipMemcpyAsync(live + q0 * n_e, s->rt[RT_B_LIVE].p, m * n_e, hipMemcpyDeviceToHost, c->stream));
        // a batch's sums lie set after set, n_pf records each, as the caller's do
        if (stats && n_pf) HIPCHK(c, hipMemcpyAsync(stats + q0 * n_pf, d_stat, 32 * m * n_pf, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(freed + q0, d_stat + freed_at, 32 * m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return BW_OK;
}
