// bw_prune.hip -- prune (include/backuwup_gpu_pack.h, "prune"): which header entries a set of roots
// reaches, and packfiles made of the live ones.  The reference has no prune.  Three parts: the mark
// (a level-synchronous walk over the restore session's tables and decode slots: k_prune_roots,
// k_prune_expand, k_prune_account), the plan (host only, write_packfiles' grouping) and the repack
// (k_pack_meta_sealed in bw_pack.hip writes the header entries, k_prune_move copies the sealed blobs verbatim).  Opening
// and decoding tree blobs goes through the unpack chain unchanged (rs_decode, bw_restore.hip).
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

using namespace bw;

// ------------------------------------------------------------------ the mark
__device__ static void pr_error(const PrWalk& w, const uint8_t* hash, const uint8_t* parent, uint64_t child_pos,
                                uint32_t reason) {
    const uint64_t at = atomicAdd((unsigned long long*)&w.ctr[PR_C_ERRORS], 1ull);
    if (at >= w.err_cap) return;
    bw_prune_error& e = w.errs[at];
    for (int i = 0; i < 32; i++) {
        e.hash[i] = hash[i];
        e.parent[i] = parent ? parent[i] : 0;
    }
    e.child_pos = child_pos;
    e.reason = reason;
    e.pad = 0;
}

// One reference per lane; every lane of the wave calls this (active = the lane has a reference), so
// that the frontier is compacted per wave: a ballot of the lanes that queue an entry, one atomic by
// the first of them for the wave's place in the next frontier, each lane's place from the ballot.
__device__ static void pr_visit(const PrWalk& w, bool active, const uint8_t* key, bool tree_ref, const uint8_t* parent,
                                uint64_t child_pos) {
    bool push = false;
    uint64_t e = ~0ull;
    if (active) {
        const uint8_t st = rs_locate_one(w.loc, key, e);
        if (st) {
            pr_error(w, key, parent, child_pos, st);
        } else {
            const bw_unpack_entry& en = w.loc.entries[e];
            const bool tree = en.kind == BW_BLOB_TREE;
            const uint32_t sh = 8 * (uint32_t)(e & 3);
            const uint32_t want = (PR_LIVE | (tree_ref && tree ? PR_QUEUED : 0u)) << sh;
            const uint32_t old = atomicOr(&w.bits[e >> 2], want);
            if (tree_ref && !tree) pr_error(w, key, parent, child_pos, BW_RESTORE_ENOTTREE);
            // a chunk is never opened here: its range is checked once, by the lane that marks it
            if (!tree && !(old & (PR_LIVE << sh)) &&
                !rs_range_ok(w.pf[en.packfile].size, w.pf[en.packfile].header_len, en.offset, en.length))
                pr_error(w, en.hash, nullptr, ~0ull, BW_UNPACK_ERANGE);
            push = (want & (PR_QUEUED << sh)) && !(old & (PR_QUEUED << sh));
        }
    }
    const uint64_t bal = __ballot(push);
    if (!bal) return;
    const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__ffsll((unsigned long long)bal) - 1;
    uint64_t base = 0;
    if (lane == leader) base = atomicAdd((unsigned long long*)&w.ctr[PR_C_NEXT], (unsigned long long)__popcll(bal));
    const uint32_t lo = __shfl((uint32_t)base, leader), hi = __shfl((uint32_t)(base >> 32), leader);
    base = ((uint64_t)hi << 32) | lo;
    if (push) w.next[base + __popcll(bal & ((1ull << lane) - 1))] = e;  // at most one slot per entry: the list holds n_entries
}

__global__ void __launch_bounds__(256) k_prune_roots(PrWalk w, const uint8_t* roots, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    pr_visit(w, i < n, roots + 32 * (i < n ? i : 0), true, nullptr, i);
}

// Workgroup (b, y): tree blob b of the sub-batch, its references y * 256 + t, stepping by
// PR_EXPAND_Y * 256.  The rows are read where the parser found them in the decode slot; the parser
// bounded them by the blob.
__global__ void __launch_bounds__(256) k_prune_expand(PrWalk w, const uint64_t* front, const uint8_t* slots,
                                                      const uint64_t* off, const RsTreeHdr* hdr, const uint32_t* cst,
                                                      uint64_t m) {
    const uint64_t b = blockIdx.x;
    if (b >= m || cst[b]) return;  // the chain refused the blob: the host reports it
    const RsTreeHdr& h = hdr[b];
    const uint8_t* self = w.loc.entries[front[b]].hash;
    const bool first = blockIdx.y == 0 && threadIdx.x == 0;
    if (h.status) {
        if (first) pr_error(w, self, nullptr, ~0ull, h.status);
        return;
    }
    if (first) atomicAdd((unsigned long long*)&w.ctr[PR_C_EXPANDED], 1ull);
    const uint64_t nch = h.n_children, nrefs = nch + (h.has_next ? 1 : 0);
    const uint8_t* rows = slots + off[b] + h.ch_pos;
    const bool dir = h.kind == BW_TREE_DIR;
    for (uint64_t r0 = (uint64_t)blockIdx.y * 256; r0 < nrefs; r0 += (uint64_t)PR_EXPAND_Y * 256) {
        const uint64_t r = r0 + threadIdx.x;
        const bool child = r < nch;
        pr_visit(w, r < nrefs, child ? rows + 32 * r : h.next, dir || !child, self, child ? r : ~0ull);
    }
}

__device__ static inline uint64_t pr_wave_sum(uint64_t v) {
    for (int d = 32; d; d >>= 1) v += __shfl_down((unsigned long long)v, d);
    return v;  // lane 0 holds the sum
}

// One lane per entry.  Entries come in packfile order, so a wave usually lies in one packfile: its
// four sums then take one atomic each, by lane 0; a wave that spans packfiles adds lane by lane.
__global__ void __launch_bounds__(256) k_prune_account(const bw_unpack_entry* entries, uint64_t n, const uint32_t* bits,
                                                       uint8_t* live, uint64_t* stats) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = e < n;
    uint32_t p = 0;
    uint64_t bytes = 0, lv = 0;
    if (in) {
        p = entries[e].packfile;
        bytes = BW_BLOB_NONCE_SIZE + entries[e].length;
        lv = (bits[e >> 2] >> (8 * (e & 3))) & PR_LIVE;
        live[e] = (uint8_t)lv;
    }
    if (!__any(in)) return;
    const uint32_t p0 = __shfl(p, 0);  // lane 0 holds the wave's lowest entry
    unsigned long long* s = (unsigned long long*)stats;
    if (__all(!in || p == p0)) {
        const uint64_t a = pr_wave_sum(lv), b = pr_wave_sum(lv ? bytes : 0), c = pr_wave_sum(in ? 1 : 0), d = pr_wave_sum(bytes);
        if ((threadIdx.x & 63) == 0) {
            if (a) atomicAdd(&s[4ull * p0], a);
            if (b) atomicAdd(&s[4ull * p0 + 1], b);
            atomicAdd(&s[4ull * p0 + 2], c);
            atomicAdd(&s[4ull * p0 + 3], d);
        }
    } else if (in) {
        if (lv) {
            atomicAdd(&s[4ull * p], 1ull);
            atomicAdd(&s[4ull * p + 1], bytes);
        }
        atomicAdd(&s[4ull * p + 2], 1ull);
        atomicAdd(&s[4ull * p + 3], bytes);
    }
}

void bw::launch_prune_roots(hipStream_t st, const PrWalk& w, const uint8_t* roots, uint64_t n) {
    if (n) hipLaunchKernelGGL(k_prune_roots, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, w, roots, n);
}
void bw::launch_prune_expand(hipStream_t st, const PrWalk& w, const uint64_t* front, const uint8_t* slots,
                             const uint64_t* off, const RsTreeHdr* hdr, const uint32_t* cst, uint64_t m) {
    if (m) hipLaunchKernelGGL(k_prune_expand, dim3((uint32_t)m, PR_EXPAND_Y), dim3(256), 0, st, w, front, slots, off, hdr, cst, m);
}
void bw::launch_prune_account(hipStream_t st, const bw_unpack_entry* entries, uint64_t n, const uint32_t* bits,
                              uint8_t* live, uint64_t* stats) {
    if (n) hipLaunchKernelGGL(k_prune_account, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, entries, n, bits, live, stats);
}

static void pr_host_error(std::vector<bw_prune_error>& v, const uint8_t* hash, uint32_t reason) {
    bw_prune_error e;
    memset(&e, 0, sizeof(e));
    memcpy(e.hash, hash, 32);
    e.child_pos = ~0ull;
    e.reason = reason;
    v.push_back(e);
}

// One walk with a device error list of dev_cap <= err_cap records; *n_dev = the errors the kernels met.
// im_walk (bw_impact.hip) is this loop's twin with a taint beside the live bit and an edge list, shared by impact and
// retain: a fix to either belongs in both.
static int pr_mark_once(bw_restore* s, const uint8_t* roots, uint64_t n_roots, uint32_t flags, uint8_t* live,
                        bw_prune_packfile_stat* stats, bw_prune_counts* counts, bw_prune_error* errs, uint64_t err_cap,
                        uint64_t dev_cap, uint64_t* n_dev_out) {
    const uint64_t n_e = s->entries.size(), n_pf = s->pf.size();
    bw_ctx* c = s->c;
    memset(counts, 0, sizeof(*counts));

    // device state: the bits, two frontiers (an entry is queued once, so n_e places each), the
    // counters, the error list, and behind the per-packfile sums the live bytes and the packfile sizes
    const uint64_t words = (n_e + 3) / 4, stat_bytes = 32 * n_pf, live_at = stat_bytes, pf_at = (live_at + n_e + 15) & ~15ull;
    if (int rc = ensure(c, s->pr_bits, 4 * words + 16)) return rc;
    for (int k = 0; k < 2; k++)
        if (int rc = ensure(c, s->pr_front[k], 8 * n_e + 16)) return rc;
    if (int rc = ensure(c, s->pr_ctr, 8 * PR_C_COUNT)) return rc;
    if (int rc = ensure(c, s->pr_err, dev_cap * sizeof(bw_prune_error) + 16)) return rc;
    if (int rc = ensure(c, s->pr_stat, pf_at + n_pf * sizeof(PrPackfile) + 16)) return rc;
    if (int rc = ensure(c, s->q, std::max<uint64_t>(32 * n_roots, sizeof(RsTreeHdr) * (uint64_t)s->slots) + 16)) return rc;
    const std::vector<PrPackfile> hpf = rs_packfile_table(s);
    uint8_t* d_stat = P<uint8_t>(s->pr_stat);
    HIPCHK(c, hipMemsetAsync(s->pr_bits.p, 0, 4 * words + 16, c->stream));
    HIPCHK(c, hipMemsetAsync(s->pr_ctr.p, 0, 8 * PR_C_COUNT, c->stream));
    HIPCHK(c, hipMemsetAsync(d_stat, 0, stat_bytes + 8, c->stream));
    if (n_pf) HIPCHK(c, hipMemcpyAsync(d_stat + pf_at, hpf.data(), n_pf * sizeof(PrPackfile), hipMemcpyHostToDevice, c->stream));
    if (n_roots) HIPCHK(c, hipMemcpyAsync(s->q.p, roots, 32 * n_roots, hipMemcpyHostToDevice, c->stream));

    PrWalk w;
    w.loc = rs_locator(s);
    w.pf = (const PrPackfile*)(d_stat + pf_at);
    w.bits = P<uint32_t>(s->pr_bits);
    w.ctr = P<uint64_t>(s->pr_ctr);
    w.errs = P<bw_prune_error>(s->pr_err);
    w.err_cap = dev_cap;
    int cur = 0;
    w.next = P<uint64_t>(s->pr_front[cur]);
    launch_prune_roots(c->stream, w, P<uint8_t>(s->q), n_roots);
    HIPCHK(c, hipGetLastError());

    std::vector<bw_prune_error> herr;  // what the chain refused: the host knows it first
    std::vector<uint64_t> fr, eidx;
    std::vector<uint8_t> bst;
    std::vector<uint32_t> cst;
    uint64_t n_front = 0, n_levels = 0;
    HIPCHK(c, hipMemcpyAsync(&n_front, &w.ctr[PR_C_NEXT], 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    while (n_front) {
        if (n_front > n_e) {
            c->err = "prune: a frontier longer than the entry table";
            return BW_EHIP;
        }
        n_levels++;
        // the chain takes host entry tables: the frontier's entry indices come back, 8 bytes per tree blob
        fr.resize(n_front);
        const uint64_t* d_front = P<uint64_t>(s->pr_front[cur]);
        HIPCHK(c, hipMemcpyAsync(fr.data(), d_front, 8 * n_front, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemsetAsync(&w.ctr[PR_C_NEXT], 0, 8, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        w.next = P<uint64_t>(s->pr_front[cur ^ 1]);
        for (uint64_t lo = 0; lo < n_front; lo += s->slots) {
            const uint64_t m = std::min<uint64_t>(s->slots, n_front - lo);
            eidx.assign(fr.begin() + lo, fr.begin() + lo + m);
            for (uint64_t k = 0; k < m; k++)
                if (eidx[k] >= n_e) {
                    c->err = "prune: a frontier names an entry outside the table";
                    return BW_EHIP;
                }
            RsTables t;
            if (int rc = rs_tree_decode(s, eidx, flags, m, t, bst)) return rc;  // the first instance words hold the chain statuses
            cst.assign(m, 0);
            for (uint64_t k = 0; k < m; k++)
                if (bst[k]) {
                    cst[k] = bst[k];
                    pr_host_error(herr, s->entries[eidx[k]].hash, bst[k]);
                }
            uint32_t* d_cst = (uint32_t*)t.dst_off;
            HIPCHK(c, hipMemcpyAsync(d_cst, cst.data(), 4 * m, hipMemcpyHostToDevice, c->stream));
            if (int rc = rs_tree_parse(s, t, m, nullptr)) return rc;  // the headers stay in s->q, sized above
            launch_prune_expand(c->stream, w, d_front + lo, P<uint8_t>(s->slot_buf), t.slot_off, P<RsTreeHdr>(s->q), d_cst, m);
            HIPCHK(c, hipGetLastError());
            // the slots and the tables are reused by the next sub-batch
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        cur ^= 1;
        HIPCHK(c, hipMemcpyAsync(&n_front, &w.ctr[PR_C_NEXT], 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }

    // accounting: one pass over the entries
    launch_prune_account(c->stream, P<bw_unpack_entry>(s->d_entries), n_e, w.bits, d_stat + live_at, (uint64_t*)d_stat);
    HIPCHK(c, hipGetLastError());
    uint64_t ctr[PR_C_COUNT];
    HIPCHK(c, hipMemcpyAsync(ctr, w.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
    if (n_e) HIPCHK(c, hipMemcpyAsync(live, d_stat + live_at, n_e, hipMemcpyDeviceToHost, c->stream));
    if (n_pf) HIPCHK(c, hipMemcpyAsync(stats, d_stat, stat_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t n_dev = ctr[PR_C_ERRORS], dev_take = std::min(n_dev, dev_cap);
    *n_dev_out = n_dev;
    if (dev_take) HIPCHK(c, hipMemcpy(errs, s->pr_err.p, dev_take * sizeof(bw_prune_error), hipMemcpyDeviceToHost));
    for (uint64_t k = 0; k < herr.size() && dev_take + k < err_cap; k++) errs[dev_take + k] = herr[k];
    for (uint64_t p = 0; p < n_pf; p++) {
        counts->live_blobs += stats[p].live_blobs;
        counts->live_bytes += stats[p].live_bytes;
        counts->total_blobs += stats[p].total_blobs;
        counts->total_bytes += stats[p].total_bytes;
    }
    counts->n_trees_expanded = ctr[PR_C_EXPANDED];
    counts->n_levels = n_levels;
    counts->n_errors = n_dev + herr.size();
    if (counts->n_errors > err_cap) {
        c->err = "prune: " + std::to_string(counts->n_errors) + " errors do not fit err_cap";
        return BW_ENOSPC;
    }
    return BW_OK;
}

extern "C" int bw_prune_mark(bw_restore* s, const uint8_t* roots, uint64_t n_roots, uint32_t flags, uint8_t* live,
                             bw_prune_packfile_stat* stats, bw_prune_counts* counts, bw_prune_error* errs,
                             uint64_t err_cap) {
    if (!s || !counts || (flags & ~BW_UNPACK_VERIFY) || (n_roots && !roots) || (err_cap && !errs)) return BW_EINVAL;
    if ((!s->entries.empty() && !live) || (!s->pf.empty() && !stats)) return BW_EINVAL;
    hipSetDevice(s->c->device);
    // The device's error list does not follow a generous err_cap: it holds PR_ERR_DEVICE records, and
    // only a walk that met more of them (and whose caller has room for more) is run a second time
    // with a list of the size it needs.  The walk is deterministic, so the second count is the first.
    uint64_t dev_cap = std::min<uint64_t>(err_cap, PR_ERR_DEVICE);
    for (;;) {
        uint64_t n_dev = 0;
        const int rc = pr_mark_once(s, roots, n_roots, flags, live, stats, counts, errs, err_cap, dev_cap, &n_dev);
        if ((rc != BW_OK && rc != BW_ENOSPC) || n_dev <= dev_cap || dev_cap >= err_cap) return rc;
        dev_cap = std::min(err_cap, n_dev);
    }
}

// ------------------------------------------------------------------ the plan (host only)
// write_packfiles' grouping over the sealed lengths: bw_pack_plan's own rule (flags 0: the payload is
// the frame, sealed = payload + 16), so that the two cannot drift apart
static int pr_group(const std::vector<uint64_t>& sealed, std::vector<bw_packfile>& out) {
    std::vector<uint64_t> payload(sealed.size());
    for (size_t i = 0; i < sealed.size(); i++) payload[i] = sealed[i] - BW_SEAL_TAG_BYTES;  // the range check gave length >= 16
    uint64_t n = 0, total = 0;
    int rc = bw_pack_plan(payload.data(), payload.size(), 0, nullptr, 0, &n, &total);
    if (rc != BW_OK && rc != BW_ENOSPC) return rc;
    out.resize(n);
    return n ? bw_pack_plan(payload.data(), payload.size(), 0, out.data(), n, &n, &total) : BW_OK;
}

extern "C" int bw_prune_plan(const bw_unpack_entry* entries, uint64_t n_entries, const bw_packfile* packfiles, uint64_t n_pf,
                             const uint8_t* live, const uint8_t* rewrite, uint64_t* order, uint64_t order_cap,
                             uint64_t* n_moved, bw_packfile* plan, uint64_t plan_cap, uint64_t* n_new,
                             uint64_t* total_bytes, uint64_t* bad_entry) {
    if (!n_moved || !n_new || !total_bytes || !bad_entry) return BW_EINVAL;
    *n_moved = *n_new = *total_bytes = 0;
    *bad_entry = ~0ull;
    if ((n_entries && (!entries || !live)) || (n_pf && (!packfiles || !rewrite)) || (order_cap && !order) ||
        (plan_cap && !plan))
        return BW_EINVAL;
    // ascending by packfile position, then by entry index (the entries of a packfile need not be together)
    std::vector<uint64_t> ord;
    for (uint64_t i = 0; i < n_entries; i++) {
        const bw_unpack_entry& e = entries[i];
        if (e.packfile >= n_pf) {
            *bad_entry = i;
            return BW_EINVAL;
        }
        if (!live[i] || !rewrite[e.packfile]) continue;
        if (!rs_range_ok(packfiles[e.packfile].size, packfiles[e.packfile].header_len, e.offset, e.length)) {
            *bad_entry = i;
            return BW_EINVAL;
        }
        ord.push_back(i);
    }
    std::stable_sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) { return entries[a].packfile < entries[b].packfile; });
    std::vector<uint64_t> sealed(ord.size());
    for (uint64_t k = 0; k < ord.size(); k++) sealed[k] = entries[ord[k]].length;
    std::vector<bw_packfile> pl;
    if (int rc = pr_group(sealed, pl)) return rc;
    *n_moved = ord.size();
    *n_new = pl.size();
    *total_bytes = pl.empty() ? 0 : pl.back().offset + pl.back().size;
    for (const bw_packfile& p : pl)
        if (p.size > BW_PACKFILE_MAX_SIZE) return BW_EINVAL;
    if (ord.size() > order_cap || pl.size() > plan_cap) return BW_ENOSPC;
    std::copy(ord.begin(), ord.end(), order);
    std::copy(pl.begin(), pl.end(), plan);
    return BW_OK;
}

// ------------------------------------------------------------------ the repack
// Every moved blob's nonce || sealed bytes from its old place to its new one.  A wave takes one piece
// (at most RS_PIECE bytes of one blob, found by a binary search of the piece prefix) and copies it
// as k_rs_gather does, in the strict form: a blob's neighbours in the old packfile are not read.
__global__ void __launch_bounds__(256) k_prune_move(const uint8_t* pf, const uint64_t* src, const uint64_t* dst,
                                                    const uint64_t* len, const uint64_t* piece0, uint64_t n, uint8_t* out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
    const uint64_t waves = (uint64_t)gridDim.x * blockDim.x / 64;
    const uint64_t total = piece0[n];
    for (uint64_t pc = wave; pc < total; pc += waves) {
        uint64_t lo = 0, hi = n;  // piece0[lo] <= pc < piece0[hi]; every blob has a piece (12 bytes at least)
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) / 2;
            if (piece0[mid] <= pc) lo = mid; else hi = mid;
        }
        const uint64_t p0 = (pc - piece0[lo]) * RS_PIECE, l = len[lo];
        if (p0 >= l) continue;
        const uint64_t nb = l - p0 < RS_PIECE ? l - p0 : RS_PIECE;
        rs_copy_piece<true>(pf + src[lo] + p0, out + dst[lo] + p0, nb, lane);
    }
}

void bw::launch_prune_move(hipStream_t st, const uint8_t* pf, const uint64_t* src, const uint64_t* dst, const uint64_t* len,
                           const uint64_t* piece0, uint64_t n, uint64_t total_pieces, uint8_t* out) {
    if (!n || !total_pieces) return;
    const uint64_t blocks = std::min<uint64_t>(8192, (total_pieces + 3) / 4);
    hipLaunchKernelGGL(k_prune_move, dim3((uint32_t)blocks), dim3(256), 0, st, pf, src, dst, len, piece0, n, out);
}

extern "C" int bw_prune_repack_device(bw_restore* s, const uint64_t* order, uint64_t n, const bw_packfile* plan, uint64_t npf,
                                      const uint8_t* new_ids, uint8_t* d_out) {
    if (!s || (n && !order) || (npf && (!plan || !new_ids || !d_out))) return BW_EINVAL;
    bw_ctx* c = s->c;
    hipSetDevice(c->device);
    const uint64_t n_e = s->entries.size();
    auto refuse = [&](const std::string& why) {
        c->err = "prune: the order or the plan does not match the session's entries: " + why;
        return BW_EINVAL;
    };
    // the order: live entries as bw_prune_plan lists them (ascending by packfile, then by index), each inside its packfile
    for (uint64_t i = 0; i < n; i++) {
        if (order[i] >= n_e) return refuse("entry " + std::to_string(i) + " of the order is outside the table");
        const bw_unpack_entry& e = s->entries[order[i]];
        if (!rs_range_ok(s->pf[e.packfile].size, s->pf[e.packfile].header_len, e.offset, e.length))
            return refuse("entry " + std::to_string(order[i]) + " leaves its packfile");
        if (i) {
            const bw_unpack_entry& q = s->entries[order[i - 1]];
            if (q.packfile > e.packfile || (q.packfile == e.packfile && order[i - 1] >= order[i]))
                return refuse("the order is not ascending at " + std::to_string(i));
        }
    }
    // the plan: what the grouping gives for exactly these blobs
    std::vector<uint64_t> sealed(n);
    for (uint64_t i = 0; i < n; i++) sealed[i] = s->entries[order[i]].length;
    std::vector<bw_packfile> pl;
    if (int rc = pr_group(sealed, pl)) return rc;
    if (pl.size() != npf) return refuse("the grouping gives " + std::to_string(pl.size()) + " packfiles");
    for (uint64_t p = 0; p < npf; p++) {
        if (memcmp(&pl[p], &plan[p], sizeof(bw_packfile))) return refuse("packfile " + std::to_string(p) + " differs from the grouping");
        if (plan[p].size > BW_PACKFILE_MAX_SIZE) return refuse("packfile " + std::to_string(p) + " exceeds the size limit");
    }
    if (!n) return BW_OK;

    // the tables (repack_tables' columns), then one PackFileDesc per packfile
    const RepackTables r = repack_tables(order, n, plan, npf, s->pf.data(), s->entries.data());
    std::vector<PackFileDesc> files(npf);
    for (uint64_t p = 0; p < npf; p++) files[p] = PackFileDesc{r.h_off[p], plan[p].n_blobs, plan[p].offset, plan[p].header_len};
    const uint64_t tab_bytes = 8 * r.tab.size();
    if (int rc = ensure(c, s->pr_tab, tab_bytes + npf * sizeof(PackFileDesc) + 16)) return rc;
    if (int rc = ensure(c, s->pr_hdr, r.hdr_total + 16)) return rc;
    uint64_t* d_tab = P<uint64_t>(s->pr_tab);
    auto d_col = [&](int col) { return d_tab + (uint64_t)col * n; };
    PackFileDesc* d_files = (PackFileDesc*)(P<uint8_t>(s->pr_tab) + tab_bytes);
    HIPCHK(c, hipMemcpyAsync(d_tab, r.tab.data(), tab_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_files, files.data(), npf * sizeof(PackFileDesc), hipMemcpyHostToDevice, c->stream));
    // the header plaintexts, built in place: the entries, then each Vec length and u64 LE prefix (k_pack_files)
    launch_pack_meta_sealed(c->stream, P<bw_unpack_entry>(s->d_entries), d_col(RP_ORDER), d_col(RP_SECT), d_col(RP_HOFF), n,
                            P<uint8_t>(s->pr_hdr));
    launch_pack_meta(c->stream, nullptr, 0, d_files, npf, P<uint8_t>(s->pr_hdr), d_out);
    launch_prune_move(c->stream, s->d_pf, d_col(RP_SRC), d_col(RP_DST), d_col(RP_LEN), d_col(RP_PIECE0), n, r.pieces, d_out);
    HIPCHK(c, hipGetLastError());
    // every header: derive_backup_key(b"header") + AES-GCM(new packfile id) behind the length prefix
    std::vector<uint8_t> info(npf * 6);
    for (uint64_t p = 0; p < npf; p++) memcpy(&info[6 * p], "header", 6);
    if (int rc = bw_seal_device(c, s->prk, P<uint8_t>(s->pr_hdr), r.h_off.data(), r.h_len.data(), npf, info.data(), 6, new_ids,
                                d_out, r.h_dst.data()))
        return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BW_OK;
}

extern "C" int bw_prune_repack(bw_restore* s, const uint64_t* order, uint64_t n, const bw_packfile* plan, uint64_t npf,
                               const uint8_t* new_ids, uint8_t* out) {
    if (!s || (npf && (!plan || !out))) return BW_EINVAL;
    bw_ctx* c = s->c;
    hipSetDevice(c->device);
    const uint64_t total = store_extent(plan, npf);
    if (total > (uint64_t)BW_PACKFILE_MAX_SIZE * std::max<uint64_t>(npf, 1)) return BW_EINVAL;  // checked again below
    if (int rc = ensure(c, s->win, total + 16)) return rc;
    if (int rc = bw_prune_repack_device(s, order, n, plan, npf, new_ids, P<uint8_t>(s->win))) return rc;
    if (total && n) HIPCHK(c, hipMemcpy(out, s->win.p, total, hipMemcpyDeviceToHost));
    return BW_OK;
}
