// bw_impact.hip -- impact (include/backuwup_gpu_pack.h, "impact"): which files of which snapshots a set
// of lost blobs takes down.  The reference cannot ask it.  Two walks over a restore session:
//   the mark    prune's level-synchronous walk (each distinct tree blob through the unpack chain once)
//               with a taint beside the reached bit: im_walk<Pol> (k_im_roots, k_im_expand: locate, SELF, the
//               rows that settle at once, the edge list; shared with retain, bw_retain.hip, which runs it under
//               the RtReach policy), then impact's own half: k_im_propagate (BELOW to its least fixed point, one sweep
//               per launch series, repeated by the host until a sweep changes nothing), k_im_taint,
//               k_im_root_affected
//   the report  a third policy over the tree-chain fetch (bw_walk.h) beside the diff walk's and the
//               parent match's: k_wk_resolve<ImFetch> with the ancestor check and the refusal of SELF
//               entries, k_wk_take<ImFetch> into the ImItem, k_im_rows (which rows are affected, the next
//               level's items), k_im_records
// Opening and decoding tree blobs goes through the unpack chain unchanged (rs_tree_decode, bw_restore.hip).
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/backuwup_gpu.h"
#include "bw_device.h"
#include "bw_internal.h"
#include "bw_ctx.h"
#include "bw_restore.h"
#include "bw_impact.h"

using namespace bw;

// ------------------------------------------------------------------ the mark
__device__ static void im_error(const ImMark& w, const uint8_t* hash, const uint8_t* parent, uint64_t child_pos,
                                uint32_t reason) {
    const uint64_t at = atomicAdd((unsigned long long*)&w.ctr[IM_C_ERRORS], 1ull);
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

__device__ static inline uint32_t im_shift(uint64_t e) { return 8 * (uint32_t)(e & 3); }

// One reference per lane; every lane of the wave calls this (active = the lane has a reference).  self
// = the expanded entry that holds the references, RS_EMPTY for the roots (which append no edge and have
// nobody to give BELOW to).  The places in the next frontier and in the edge lists come per wave from one
// atomic each (wk_wave_place).  Pol: which references become edges and what settles at once (bw_impact.h).
template <class Pol>
__device__ static void im_visit(const ImMark& w, bool active, const uint8_t* key, bool tree_ref, const uint8_t* parent,
                                uint64_t child_pos, uint32_t self) {
    bool push = false, edge = false, leaf = false, affected = false;
    uint64_t e = ~0ull;
    if (active) {
        const uint8_t st = rs_locate_one(w.loc, key, e);
        if (st) {
            im_error(w, key, parent, child_pos, st);
            affected = true;
        } else {
            const bw_unpack_entry& en = w.loc.entries[e];
            const bool tree = en.kind == BW_BLOB_TREE;
            const uint32_t sh = im_shift(e);
            const bool lost = w.bad && w.bad[e];
            // a chunk is never opened here: its range is its whole check, and every lane that reaches it makes it
            const bool range_bad = !tree && !rs_range_ok(w.pf[en.packfile].size, w.pf[en.packfile].header_len, en.offset, en.length);
            const bool queue = tree_ref && tree && !lost;  // a lost tree blob is never opened
            const uint32_t want = (IM_REACHED | (queue ? IM_QUEUED : 0u) | (lost || range_bad ? IM_SELF : 0u)) << sh;
            const uint32_t old = atomicOr(&w.bits[e >> 2], want);
            if (tree_ref && !tree) {
                im_error(w, key, parent, child_pos, BW_RESTORE_ENOTTREE);
                affected = true;
            }
            if (range_bad && !(old & (IM_REACHED << sh))) im_error(w, en.hash, nullptr, ~0ull, BW_UNPACK_ERANGE);
            if (Pol::ALL_EDGES) {
                edge = tree_ref && tree;  // only these pass something on
                leaf = !edge;
            } else {
                if (!tree) affected = affected || lost || range_bad;  // settled at once: a chunk's SELF never changes
                edge = tree;
            }
            push = queue && !(old & (IM_QUEUED << sh));
        }
    }
    const uint64_t at = wk_wave_place(push, &w.ctr[IM_C_NEXT]);
    if (push) w.next[at] = e;  // at most one place per entry: the list holds n_entries
    if (self == RS_EMPTY) return;
    const uint64_t eat = wk_wave_place(edge, &w.ctr[IM_C_EDGES]);
    if (edge) {
        if (eat < w.edge_cap) w.edges[eat] = ImEdge{self, (uint32_t)e | (tree_ref ? 0u : IM_EDGE_SELF_ONLY)};
        else atomicAdd((unsigned long long*)&w.ctr[IM_C_DROPPED], 1ull);  // the host sized the list: it refuses the walk
    }
    if (Pol::ALL_EDGES) {
        const uint64_t lat = wk_wave_place(leaf, &w.ctr[IM_C_LEAF]);
        if (leaf) {
            if (lat < w.edge_cap) w.leaf[lat] = ImEdge{self, (uint32_t)e | (tree_ref ? 0u : IM_EDGE_SELF_ONLY)};
            else atomicAdd((unsigned long long*)&w.ctr[IM_C_DROPPED], 1ull);
        }
    }
    const uint64_t bal = __ballot(affected);
    if (bal && (threadIdx.x & 63) == (uint32_t)__ffsll((unsigned long long)bal) - 1)
        atomicOr(&w.bits[self >> 2], IM_BELOW << im_shift(self));
}

template <class Pol>
__global__ void __launch_bounds__(256) k_im_roots(ImMark w, const uint8_t* roots, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    im_visit<Pol>(w, i < n, roots + 32 * (i < n ? i : 0), true, nullptr, i, RS_EMPTY);
}

// Workgroup (b, y): tree blob b of the sub-batch, its references y * 256 + t, stepping by IM_EXPAND_Y *
// 256 (k_prune_expand's shape).  The rows are read where the parser found them in the decode slot.
template <class Pol>
__global__ void __launch_bounds__(256) k_im_expand(ImMark w, const uint64_t* front, const uint8_t* slots,
                                                   const uint64_t* off, const RsTreeHdr* hdr, const uint32_t* cst, uint64_t m) {
    const uint64_t b = blockIdx.x;
    if (b >= m) return;
    const uint64_t se = front[b];
    const RsTreeHdr& h = hdr[b];
    const uint8_t* self = w.loc.entries[se].hash;
    const bool first = blockIdx.y == 0 && threadIdx.x == 0;
    if (cst[b] || h.status) {  // refused: SELF; the chain's refusal is the host's to report, the parser's is ours
        if (first) {
            if (!cst[b]) im_error(w, self, nullptr, ~0ull, h.status);
            atomicOr(&w.bits[se >> 2], IM_SELF << im_shift(se));
        }
        return;
    }
    if (first) atomicAdd((unsigned long long*)&w.ctr[IM_C_EXPANDED], 1ull);
    const uint64_t nch = h.n_children, nrefs = nch + (h.has_next ? 1 : 0);
    const uint8_t* rows = slots + off[b] + h.ch_pos;
    const bool dir = h.kind == BW_TREE_DIR;
    for (uint64_t r0 = (uint64_t)blockIdx.y * 256; r0 < nrefs; r0 += (uint64_t)IM_EXPAND_Y * 256) {
        const uint64_t r = r0 + threadIdx.x;
        const bool child = r < nch;
        im_visit<Pol>(w, r < nrefs, child ? rows + 32 * r : h.next, dir || !child, self, child ? r : ~0ull, (uint32_t)se);
    }
}

// One lane per edge of [lo, hi): a child with a bit its reference looks at gives its parent BELOW.  The
// bits only ever grow, so a stale read costs a sweep, never an answer.
__global__ void __launch_bounds__(256) k_im_propagate(uint32_t* bits, const ImEdge* edges, uint64_t lo, uint64_t hi,
                                                      uint64_t* changed) {
    const uint64_t i = lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hi) return;
    const ImEdge ed = edges[i];
    const uint32_t child = ed.child & ~IM_EDGE_SELF_ONLY;
    const uint32_t mask = (ed.child & IM_EDGE_SELF_ONLY) ? IM_SELF : (IM_SELF | IM_BELOW);
    const uint32_t cw = __atomic_load_n(&bits[child >> 2], __ATOMIC_RELAXED);
    if (!((cw >> im_shift(child)) & mask)) return;
    const uint32_t pbit = IM_BELOW << im_shift(ed.parent);
    if (__atomic_load_n(&bits[ed.parent >> 2], __ATOMIC_RELAXED) & pbit) return;
    if (!(atomicOr(&bits[ed.parent >> 2], pbit) & pbit)) *changed = 1;
}

// One lane per entry: the two public bits.
__global__ void __launch_bounds__(256) k_im_taint(const uint32_t* bits, uint64_t n, uint8_t* taint) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) taint[e] = (uint8_t)((bits[e >> 2] >> im_shift(e)) & (IM_SELF | IM_BELOW));
}

// a tree reference, against a taint byte per entry: unlocatable, not a tree, or any bit
__device__ static inline bool im_tree_ref_affected(const RsLocator& loc, const uint8_t* taint, const uint8_t* key) {
    uint64_t e;
    if (rs_locate_one(loc, key, e)) return true;
    return loc.entries[e].kind != BW_BLOB_TREE || (taint[e] & (IM_SELF | IM_BELOW));
}

// One lane per root.
__global__ void __launch_bounds__(256) k_im_root_affected(RsLocator loc, const uint8_t* taint, const uint8_t* roots, uint64_t n,
                                                          uint8_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = im_tree_ref_affected(loc, taint, roots + 32 * i) ? 1 : 0;
}

static void im_host_error(std::vector<bw_prune_error>& v, const uint8_t* hash, uint32_t reason) {
    bw_prune_error e;
    memset(&e, 0, sizeof(e));
    memcpy(e.hash, hash, 32);
    e.child_pos = ~0ull;
    e.reason = reason;
    v.push_back(e);
}

static int im_refuse(bw_ctx* c, const char* why) { return wk_refuse(c, "impact", why); }

// The walk the two marks share (impact's below, retain's in bw_retain.hip): the roots, the frontier loop
// and the expansions, with a device error list of dev_cap records.  It leaves the bits, the edge lists by
// level and the counters on the device and synchronises.  The frontier loop and the second-walk rule are
// pr_mark_once's and bw_prune_mark's (bw_prune.hip), written beside them so that prune returns what it
// returned: a fix to either loop belongs in both.
template <class Pol>
int bw::im_walk(bw_restore* s, const uint8_t* roots, uint64_t n_roots, const uint8_t* bad, uint32_t flags, uint64_t dev_cap,
                uint64_t out_bytes, DevBuf* leaf, ImWalked& wd) {
    const uint64_t n_e = s->entries.size(), n_pf = s->pf.size();
    bw_ctx* c = s->c;

    const uint64_t words = (n_e + 3) / 4;
    if (int rc = ensure(c, s->im[IM_B_BITS], 4 * words + 16)) return rc;
    for (int k = 0; k < 2; k++)
        if (int rc = ensure(c, s->im[IM_B_FRONT0 + k], 8 * n_e + 16)) return rc;
    if (int rc = ensure(c, s->im[IM_B_CTR], 8 * IM_C_COUNT)) return rc;
    if (int rc = ensure(c, s->im[IM_B_ERR], dev_cap * sizeof(bw_prune_error) + 16)) return rc;
    if (int rc = ensure(c, s->im[IM_B_PF], n_pf * sizeof(PrPackfile) + 16)) return rc;
    if (int rc = ensure(c, s->im[IM_B_BAD], n_e + 16)) return rc;
    // the caller's results and, behind them, the roots (s->q is the parser's)
    if (int rc = ensure(c, s->im[IM_B_OUT], out_bytes + 32 * n_roots + 16)) return rc;
    if (int rc = ensure(c, s->q, sizeof(RsTreeHdr) * (uint64_t)s->slots + 16)) return rc;
    wd.d_out = P<uint8_t>(s->im[IM_B_OUT]);
    wd.d_roots = wd.d_out + out_bytes;
    uint8_t* d_roots = wd.d_roots;
    const std::vector<PrPackfile> hpf = rs_packfile_table(s);
    HIPCHK(c, hipMemsetAsync(s->im[IM_B_BITS].p, 0, 4 * words + 16, c->stream));
    HIPCHK(c, hipMemsetAsync(s->im[IM_B_CTR].p, 0, 8 * IM_C_COUNT, c->stream));
    if (n_pf) HIPCHK(c, hipMemcpyAsync(s->im[IM_B_PF].p, hpf.data(), n_pf * sizeof(PrPackfile), hipMemcpyHostToDevice, c->stream));
    if (bad && n_e) HIPCHK(c, hipMemcpyAsync(s->im[IM_B_BAD].p, bad, n_e, hipMemcpyHostToDevice, c->stream));
    if (n_roots) HIPCHK(c, hipMemcpyAsync(d_roots, roots, 32 * n_roots, hipMemcpyHostToDevice, c->stream));

    ImMark& w = wd.w;
    w.loc = rs_locator(s);
    w.pf = P<PrPackfile>(s->im[IM_B_PF]);
    w.bad = bad ? P<uint8_t>(s->im[IM_B_BAD]) : nullptr;
    w.bits = P<uint32_t>(s->im[IM_B_BITS]);
    w.ctr = P<uint64_t>(s->im[IM_B_CTR]);
    w.errs = P<bw_prune_error>(s->im[IM_B_ERR]);
    w.err_cap = dev_cap;
    w.edges = P<ImEdge>(s->im[IM_B_EDGES]);
    w.leaf = leaf ? P<ImEdge>(*leaf) : nullptr;
    w.edge_cap = 0;
    int cur = 0;
    w.next = P<uint64_t>(s->im[IM_B_FRONT0 + cur]);
    if (n_roots) hipLaunchKernelGGL(k_im_roots<Pol>, wk_grid(n_roots), dim3(256), 0, c->stream, w, d_roots, n_roots);
    HIPCHK(c, hipGetLastError());

    std::vector<bw_prune_error>& herr = wd.herr;
    herr.clear();
    std::vector<uint64_t> fr, eidx;
    std::vector<uint8_t> bst;
    std::vector<uint32_t> cst;
    std::vector<uint64_t> slot_at, blen;
    ImLevels& levels = wd.levels;
    levels = ImLevels();
    uint64_t* ctr = wd.ctr;
    uint64_t edge_ub = 0;  // no more edges than this can have been appended
    HIPCHK(c, hipMemcpyAsync(ctr, w.ctr, sizeof(wd.ctr), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t n_front = ctr[IM_C_NEXT];
    while (n_front) {
        if (n_front > n_e) return im_refuse(c, "a frontier longer than the entry table");
        // the chain takes host entry tables: the frontier's entry indices come back, 8 bytes per tree blob
        fr.resize(n_front);
        const uint64_t* d_front = P<uint64_t>(s->im[IM_B_FRONT0 + cur]);
        HIPCHK(c, hipMemcpyAsync(fr.data(), d_front, 8 * n_front, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemsetAsync(&w.ctr[IM_C_NEXT], 0, 8, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        w.next = P<uint64_t>(s->im[IM_B_FRONT0 + (cur ^ 1)]);
        for (uint64_t lo = 0; lo < n_front; lo += s->slots) {
            const uint64_t m = std::min<uint64_t>(s->slots, n_front - lo);
            eidx.assign(fr.begin() + lo, fr.begin() + lo + m);
            for (uint64_t k = 0; k < m; k++)
                if (eidx[k] >= n_e) return im_refuse(c, "a frontier names an entry outside the table");
            // rs_tree_decode's two steps, taken apart for the decoded sizes: they bound the edges the sub-batch
            // can append without a look at the parsed headers, so that a sub-batch costs one sync, as prune's does
            RsTables t;
            if (int rc = rs_tables(s, m, m, t)) return rc;  // the first instance words hold the chain statuses
            slot_at.resize(m);
            for (uint64_t k = 0; k < m; k++) slot_at[k] = k * RS_SLOT_STRIDE;
            if (int rc = rs_decode(s, eidx, slot_at, flags, t, blen, bst)) return rc;
            cst.assign(m, 0);
            for (uint64_t k = 0; k < m; k++)
                if (bst[k]) {
                    cst[k] = bst[k];
                    im_host_error(herr, s->entries[eidx[k]].hash, bst[k]);
                }
            uint32_t* d_cst = (uint32_t*)t.dst_off;
            HIPCHK(c, hipMemcpyAsync(d_cst, cst.data(), 4 * m, hipMemcpyHostToDevice, c->stream));
            if (int rc = rs_tree_parse(s, t, m, nullptr)) return rc;  // the headers stay in s->q, sized above
            // the edge lists grow by what this sub-batch can append at most, and keep what they hold
            const uint64_t more = im_edge_bound(bst.data(), blen.data(), m);
            if (int rc = wk_grow(c, "impact", s->im[IM_B_EDGES], sizeof(ImEdge) * (edge_ub + more) + 16, sizeof(ImEdge) * edge_ub))
                return rc;
            if (leaf)
                if (int rc = wk_grow(c, "impact", *leaf, sizeof(ImEdge) * (edge_ub + more) + 16, sizeof(ImEdge) * edge_ub)) return rc;
            edge_ub += more;
            w.edges = P<ImEdge>(s->im[IM_B_EDGES]);
            w.leaf = leaf ? P<ImEdge>(*leaf) : nullptr;
            w.edge_cap = edge_ub;
            hipLaunchKernelGGL(k_im_expand<Pol>, dim3((uint32_t)m, IM_EXPAND_Y), dim3(256), 0, c->stream, w, d_front + lo,
                               P<uint8_t>(s->slot_buf), t.slot_off, P<RsTreeHdr>(s->q), d_cst, m);
            HIPCHK(c, hipGetLastError());
            // the slots and the tables are reused by the next sub-batch
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        cur ^= 1;
        HIPCHK(c, hipMemcpyAsync(ctr, w.ctr, sizeof(wd.ctr), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        n_front = ctr[IM_C_NEXT];
        if (ctr[IM_C_DROPPED] || ctr[IM_C_EDGES] + ctr[IM_C_LEAF] > edge_ub || !levels.close(ctr[IM_C_EDGES]))
            return im_refuse(c, "an edge count that cannot be");
    }
    return BW_OK;
}
template int bw::im_walk<ImTaint>(bw_restore*, const uint8_t*, uint64_t, const uint8_t*, uint32_t, uint64_t, uint64_t, DevBuf*, ImWalked&);
template int bw::im_walk<RtReach>(bw_restore*, const uint8_t*, uint64_t, const uint8_t*, uint32_t, uint64_t, uint64_t, DevBuf*, ImWalked&);

int bw::im_errors_out(bw_restore* s, const ImWalked& wd, const char* walk, bw_prune_error* errs, uint64_t err_cap, uint64_t dev_cap,
                      uint64_t* n_dev_out, uint64_t* n_errors) {
    bw_ctx* c = s->c;
    const uint64_t n_dev = wd.ctr[IM_C_ERRORS], dev_take = std::min(n_dev, dev_cap);
    *n_dev_out = n_dev;
    if (dev_take) HIPCHK(c, hipMemcpy(errs, s->im[IM_B_ERR].p, dev_take * sizeof(bw_prune_error), hipMemcpyDeviceToHost));
    for (uint64_t k = 0; k < wd.herr.size() && dev_take + k < err_cap; k++) errs[dev_take + k] = wd.herr[k];
    *n_errors = n_dev + wd.herr.size();
    if (*n_errors > err_cap) {
        c->err = std::string(walk) + ": " + std::to_string(*n_errors) + " errors do not fit err_cap";
        return BW_ENOSPC;
    }
    return BW_OK;
}

// Impact's half of the mark: the walk, BELOW to its fixed point over the edges, the results.  *n_dev_out =
// the errors the kernels met.
static int im_mark_once(bw_restore* s, const uint8_t* roots, uint64_t n_roots, const uint8_t* bad, uint32_t flags,
                        uint8_t* taint, uint8_t* root_affected, bw_impact_counts* counts, bw_prune_error* errs,
                        uint64_t err_cap, uint64_t dev_cap, uint64_t* n_dev_out) {
    const uint64_t n_e = s->entries.size();
    bw_ctx* c = s->c;
    memset(counts, 0, sizeof(*counts));
    // the results: [taint | root_affected]
    const uint64_t ra_at = (n_e + 15) & ~15ull, out_bytes = ra_at + ((n_roots + 15) & ~15ull);
    ImWalked wd;
    if (int rc = im_walk<ImTaint>(s, roots, n_roots, bad, flags, dev_cap, out_bytes, nullptr, wd)) return rc;
    const ImMark& w = wd.w;
    const ImLevels& levels = wd.levels;
    uint8_t *d_taint = wd.d_out, *d_ra = d_taint + ra_at, *d_roots = wd.d_roots;

    // BELOW to its least fixed point: sweeps, latest level first, until one changes nothing
    uint64_t n_sweeps = 0, changed = 1;
    const auto ranges = levels.sweep();
    while (changed) {
        if (n_sweeps > n_e + 1) return im_refuse(c, "more sweeps than the store has entries");  // a sweep that changes something sets a bit
        HIPCHK(c, hipMemsetAsync(&w.ctr[IM_C_CHANGED], 0, 8, c->stream));
        for (const auto& r : ranges)
            hipLaunchKernelGGL(k_im_propagate, wk_grid(r.second - r.first), dim3(256), 0, c->stream, w.bits, w.edges, r.first,
                               r.second, &w.ctr[IM_C_CHANGED]);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&changed, &w.ctr[IM_C_CHANGED], 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        n_sweeps++;
    }

    // results: the taint bytes, then the roots against them
    if (n_e) hipLaunchKernelGGL(k_im_taint, wk_grid(n_e), dim3(256), 0, c->stream, w.bits, n_e, d_taint);
    if (n_roots)
        hipLaunchKernelGGL(k_im_root_affected, wk_grid(n_roots), dim3(256), 0, c->stream, w.loc, d_taint, d_roots, n_roots, d_ra);
    HIPCHK(c, hipGetLastError());
    if (n_e) HIPCHK(c, hipMemcpyAsync(taint, d_taint, n_e, hipMemcpyDeviceToHost, c->stream));
    if (n_roots) HIPCHK(c, hipMemcpyAsync(root_affected, d_ra, n_roots, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    counts->n_trees_expanded = wd.ctr[IM_C_EXPANDED];
    counts->n_levels = levels.n_levels();
    counts->n_edges = levels.n_edges();
    counts->n_sweeps = n_sweeps;
    for (uint64_t e = 0; e < n_e; e++) counts->n_tainted += taint[e] != 0;
    for (uint64_t r = 0; r < n_roots; r++) counts->n_roots_affected += root_affected[r];
    return im_errors_out(s, wd, "impact", errs, err_cap, dev_cap, n_dev_out, &counts->n_errors);
}

extern "C" int bw_impact_mark(bw_restore* s, const uint8_t* roots, uint64_t n_roots, const uint8_t* bad, uint32_t flags,
                              uint8_t* taint, uint8_t* root_affected, bw_impact_counts* counts, bw_prune_error* errs,
                              uint64_t err_cap) {
    if (!s || !counts || (flags & ~BW_UNPACK_VERIFY) || (n_roots && (!roots || !root_affected)) || (err_cap && !errs))
        return BW_EINVAL;
    if (!s->entries.empty() && !taint) return BW_EINVAL;
    hipSetDevice(s->c->device);
    if (s->entries.size() >= IM_MAX_ENTRIES) return wk_too_large(s->c, "impact", "2^31 entries or more");
    // the device's error list and the second walk when it was too short: bw_prune_mark's rule
    uint64_t dev_cap = std::min<uint64_t>(err_cap, IM_ERR_DEVICE);
    for (;;) {
        uint64_t n_dev = 0;
        const int rc = im_mark_once(s, roots, n_roots, bad, flags, taint, root_affected, counts, errs, err_cap, dev_cap, &n_dev);
        if ((rc != BW_OK && rc != BW_ENOSPC) || n_dev <= dev_cap || dev_cap >= err_cap) return rc;
        dev_cap = std::min(err_cap, n_dev);
    }
}

// ------------------------------------------------------------------ the report walk: the fetch's policy
// What the shared fetch (bw_walk.h) leaves to the walk.  An owner is an item of the level.
struct ImFetch {
    typedef ImWalk Walk;
    static constexpr const char* NAME = "impact";
    static constexpr const char* ROWS_TOO_MANY = "a level of more than 2^30 children rows";
    static constexpr uint64_t MAX_ROWS = IM_MAX_ROWS;
    static constexpr uint64_t ERRS_PER_REF = 2;  // the ancestor check's, and the locate's

    // an item's first piece: is its hash one of its ancestors' on this path?  Then it is read for its name only.
    __device__ static bool first(const ImWalk& w, const WkRef& r) {
        uint64_t rec = w.items[r.owner].parent;
        for (uint64_t step = 0; rec != IM_NONE && step <= w.level; step++) {  // each step is one level up
            const bw_impact_record& p = w.recs[rec];
            if (rs_eq(p.hash, r.hash, 32)) {
                wk_error(w.f, r.hash, r.by, r.by_pos, BW_RESTORE_EFORMAT);
                atomicOr(&w.items[r.owner].state, IM_CYCLIC);
                return true;
            }
            rec = p.parent;
        }
        return false;
    }

    // a lost entry is never opened, and is no error of this walk
    __device__ static bool refuse(const ImWalk& w, uint64_t e) { return w.taint[e] & IM_SELF; }

    __device__ static void lost(const ImWalk& w, uint32_t item) { atomicOr(&w.items[item].state, IM_TRUNC); }

    __device__ static void header(const ImWalk& w, uint32_t item, const RsTreeHdr& h, uint64_t name_off) {
        ImItem& it = w.items[item];
        atomicOr(&it.state, IM_OK);
        it.kind = h.kind;
        it.tflags = h.flags;
        it.size = h.size;
        it.mtime = h.mtime;
        it.ctime = h.ctime;
        it.name_off = name_off;
        it.name_len = h.name_len;
    }
};

// One lane per row of the level's lists: is it affected, and for a Dir item the next level's item.
// next_items / next_refs hold a place per row of a Dir item.
__global__ void __launch_bounds__(256) k_im_rows(ImWalk w, ImItem* next_items, WkRef* next_refs) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool push = false;
    uint64_t seg = 0, k = 0;
    uint32_t item = 0;
    const uint8_t* row = nullptr;
    if (r < w.n_rows) {
        seg = wk_range_of(w.f.seg_row0, w.f.n_seg, r);  // no segment is empty
        item = w.f.seg_node[seg];
        row = wk_stage_row(w.f, seg, r);
        k = r - w.item_row0[item];
        ImItem& it = w.items[item];
        const bool dir = it.kind == BW_TREE_DIR;
        bool affected;
        if (dir) {
            affected = im_tree_ref_affected(w.f.loc, w.taint, row);
        } else {
            uint64_t e;
            affected = rs_locate_one(w.f.loc, row, e) || (w.taint[e] & IM_SELF);
        }
        if (affected) {
            atomicAdd((unsigned long long*)&it.n_affected, 1ull);
            atomicMin((unsigned long long*)&it.first_affected, (unsigned long long)k);
        }
        push = affected && dir;
    }
    const uint64_t j = wk_wave_place(push, &w.ctr[IM_C_ITEMS]);
    if (!push) return;  // at most one place per row of a Dir item: the lists hold that many
    ImItem& x = next_items[j];
    memset(&x, 0, sizeof(x));
    wk_copy32(x.hash, row);
    x.parent = w.rec0 + item;
    x.root = w.items[item].root;
    x.first_affected = IM_NONE;
    WkRef& f = next_refs[j];
    wk_copy32(f.hash, row);
    wk_copy32(f.by, w.f.seg_hash + 32ull * w.f.seg_sid[seg]);
    f.by_pos = r - w.f.seg_row0[seg];
    f.owner = (uint32_t)j;
    f.pad = 0;
}

// One lane per item, after k_im_rows: its record.
__global__ void __launch_bounds__(256) k_im_records(ImWalk w) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w.n_items) return;
    const ImItem& it = w.items[i];
    bw_impact_record& r = w.recs[w.rec0 + i];
    memset(&r, 0, sizeof(r));
    wk_copy32(r.hash, it.hash);
    r.root = it.root;
    r.parent = it.parent;
    r.first_affected = IM_NONE;
    r.flags = ((it.state & IM_OK) ? 0 : BW_IMPACT_UNREADABLE) | ((it.state & IM_TRUNC) ? BW_IMPACT_TRUNCATED : 0) |
              ((it.state & IM_CYCLIC) ? BW_IMPACT_CYCLIC : 0);
    if (!(it.state & IM_OK)) return;
    r.name_off = it.name_off;
    r.name_len = it.name_len;
    r.kind = it.kind;
    r.meta_flags = it.tflags;
    r.size = it.size;
    r.mtime = it.mtime;
    r.ctime = it.ctime;
    r.n_children = w.item_rows[i];
    r.n_affected = it.n_affected;
    r.first_affected = it.first_affected;
}

extern "C" int bw_impact_paths(bw_restore* s, const uint8_t* roots, uint64_t n_roots, const uint8_t* taint, uint32_t flags,
                               bw_impact_record* records, uint64_t record_cap, uint8_t* names, uint64_t names_cap,
                               bw_impact_root* per_root, bw_impact_paths_counts* counts, bw_prune_error* errs,
                               uint64_t err_cap) {
    if (!s || !counts || (flags & ~BW_UNPACK_VERIFY) || (record_cap && !records) || (names_cap && !names) ||
        (err_cap && !errs) || (n_roots && (!roots || !per_root)) || (!s->entries.empty() && !taint))
        return BW_EINVAL;
    bw_ctx* c = s->c;
    hipSetDevice(c->device);
    const uint64_t n_e = s->entries.size();
    memset(counts, 0, sizeof(*counts));
    if (n_roots) memset(per_root, 0, n_roots * sizeof(bw_impact_root));
    if (im_taint_check(taint, n_e) != ~0ull) {
        c->err = "impact: taint holds a bit that is neither SELF nor BELOW";
        return BW_EINVAL;
    }
    if (!n_roots) return BW_OK;
    if (n_roots > IM_MAX_ROWS) return wk_too_large(c, ImFetch::NAME, "more than 2^30 roots");

    WkHost<ImFetch> H;
    if (int rc = wk_open(H, s, flags)) return rc;
    ImWalk& w = H.w;
    w.ctr = P<uint64_t>(s->wk[WK_B_CTR]);
    if (int rc = ensure(c, s->im[IM_B_TAINT], n_e + 16)) return rc;
    if (n_e) HIPCHK(c, hipMemcpyAsync(s->im[IM_B_TAINT].p, taint, n_e, hipMemcpyHostToDevice, c->stream));
    w.taint = P<uint8_t>(s->im[IM_B_TAINT]);

    // level 0: the affected roots in root order; the device says which they are
    int lv = 0;
    uint64_t n_items = 0;
    {
        if (int rc = ensure(c, s->q, 33 * n_roots + 16)) return rc;
        uint8_t* d_roots = P<uint8_t>(s->q);
        std::vector<uint8_t> ra(n_roots);
        HIPCHK(c, hipMemcpyAsync(d_roots, roots, 32 * n_roots, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_im_root_affected, wk_grid(n_roots), dim3(256), 0, c->stream, w.f.loc, w.taint, d_roots, n_roots,
                           d_roots + 32 * n_roots);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(ra.data(), d_roots + 32 * n_roots, n_roots, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::vector<ImItem> hi;
        std::vector<WkRef> hr;
        for (uint64_t r = 0; r < n_roots; r++) {
            if (!ra[r]) continue;
            ImItem it;
            memset(&it, 0, sizeof(it));
            memcpy(it.hash, roots + 32 * r, 32);
            it.parent = IM_NONE;
            it.root = (uint32_t)r;
            it.first_affected = IM_NONE;
            WkRef f;
            memset(&f, 0, sizeof(f));
            memcpy(f.hash, roots + 32 * r, 32);
            f.by_pos = r;
            f.owner = (uint32_t)hi.size();
            hi.push_back(it);
            hr.push_back(f);
        }
        n_items = hi.size();
        if (int rc = ensure(c, s->im[IM_B_ITEMS0 + lv], n_items * sizeof(ImItem) + 16)) return rc;
        if (int rc = ensure(c, s->im[IM_B_REFS0 + lv], n_items * sizeof(WkRef) + 16)) return rc;
        if (n_items) {
            HIPCHK(c, hipMemcpyAsync(s->im[IM_B_ITEMS0 + lv].p, hi.data(), n_items * sizeof(ImItem), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(s->im[IM_B_REFS0 + lv].p, hr.data(), n_items * sizeof(WkRef), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));  // hi and hr leave scope
        }
    }

    uint64_t n_rec = 0, n_levels = 0;
    uint64_t rec_fit = 0, names_fit = 0;  // the totals of the levels that fit the caller's arrays
    uint64_t& name_total = H.lv.name_total;  // the names of every level so far
    bool full = false;
    std::vector<uint64_t> lvl;

    while (n_items) {
        // an item that is expanded has a located hash no ancestor has: a path is no longer than the table
        if (n_levels > n_e + 1) return im_refuse(c, "more levels than the store has entries");
        if (n_items > IM_MAX_ROWS) return wk_too_large(c, ImFetch::NAME, "a level of more than 2^30 items");
        w.level = n_levels++;
        w.items = P<ImItem>(s->im[IM_B_ITEMS0 + lv]);
        w.n_items = n_items;
        w.rec0 = n_rec;
        H.owners.assign(n_items, WkOwner());
        H.lv.segs.clear();
        H.lv.stage_rows = 0;
        // the records so far are the ancestors the fetch's check walks; this level's follow them
        DevBuf& rec_buf = s->im[IM_B_REC];
        if (int rc = wk_grow(c, ImFetch::NAME, rec_buf, (n_rec + n_items) * sizeof(bw_impact_record) + 16, n_rec * sizeof(bw_impact_record)))
            return rc;
        w.recs = P<bw_impact_record>(rec_buf);

        // ---- read: every item's header and name, and every row of every piece of its chain (bw_walk.h)
        if (int rc = wk_fetch(H, P<WkRef>(s->im[IM_B_REFS0 + lv]), n_items, true, true, H.owners.data())) return rc;

        // ---- the level's lists: item after item; the walk's own tables between the segments': [item_row0 | item_rows]
        const uint64_t n_rows = H.lv.stage_rows;
        wk_level_tables(w.f, H.lv.segs, lvl, 2 * n_items);
        const uint64_t n_seg = w.f.n_seg;
        uint64_t* item_row0 = lvl.data() + 2 * n_seg + 1;
        uint64_t* item_rows = item_row0 + n_items;
        uint64_t run = 0, dir_rows = 0;  // only a row of a Dir item can become an item of the next level
        for (uint64_t i = 0; i < n_items; i++) {
            item_row0[i] = run;
            item_rows[i] = H.owners[i].n_rows;
            run += H.owners[i].n_rows;
            if (H.owners[i].dir) dir_rows += H.owners[i].n_rows;
        }
        if (run != n_rows) return im_refuse(c, "the level's rows do not add up");
        if (int rc = ensure(c, s->im[IM_B_LVL], 8 * lvl.size() + 16)) return rc;
        HIPCHK(c, hipMemcpyAsync(s->im[IM_B_LVL].p, lvl.data(), 8 * lvl.size(), hipMemcpyHostToDevice, c->stream));
        wk_level_pointers(w.f, P<uint64_t>(s->im[IM_B_LVL]), 2 * n_items);
        w.item_row0 = w.f.seg_stage + n_seg;
        w.item_rows = w.item_row0 + n_items;
        w.n_rows = n_rows;
        w.f.stage = P<uint8_t>(s->wk[WK_B_STAGE]);
        w.f.seg_hash = P<uint8_t>(s->wk[WK_B_SEGHASH]);
        w.f.names = P<uint8_t>(s->wk[WK_B_NAMES]);

        // ---- which rows are affected, and the next level's items: a row gives one item at most
        HIPCHK(c, hipMemsetAsync(&w.ctr[IM_C_ITEMS], 0, 8, c->stream));
        if (n_rows) {
            DevBuf &next_items = s->im[IM_B_ITEMS0 + (lv ^ 1)], &next_refs = s->im[IM_B_REFS0 + (lv ^ 1)];
            if (int rc = ensure(c, next_items, dir_rows * sizeof(ImItem) + 16)) return rc;
            if (int rc = ensure(c, next_refs, dir_rows * sizeof(WkRef) + 16)) return rc;
            hipLaunchKernelGGL(k_im_rows, wk_grid(n_rows), dim3(256), 0, c->stream, w, P<ImItem>(next_items), P<WkRef>(next_refs));
        }
        hipLaunchKernelGGL(k_im_records, wk_grid(n_items), dim3(256), 0, c->stream, w);
        HIPCHK(c, hipGetLastError());
        uint64_t ctr[WK_C_COUNT];
        HIPCHK(c, hipMemcpyAsync(ctr, w.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const uint64_t n_next = ctr[IM_C_ITEMS];
        if (n_next > dir_rows) return im_refuse(c, "a level's item count that cannot be");
        n_rec += n_items;
        if (n_rec > record_cap || name_total > names_cap) {
            full = true;
            break;
        }
        rec_fit = n_rec;
        names_fit = name_total;
        n_items = n_next;
        lv ^= 1;
    }

    // ---- results
    uint64_t n_err = 0;
    HIPCHK(c, hipMemcpyAsync(&n_err, w.f.n_err, 8, hipMemcpyDeviceToHost, c->stream));
    if (rec_fit) HIPCHK(c, hipMemcpyAsync(records, s->im[IM_B_REC].p, rec_fit * sizeof(bw_impact_record), hipMemcpyDeviceToHost, c->stream));
    if (names_fit) HIPCHK(c, hipMemcpyAsync(names, s->wk[WK_B_NAMES].p, names_fit, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int rc = wk_errors_out(H, n_err, errs, err_cap);
    if (rc != BW_OK && rc != BW_ENOSPC) return rc;
    for (uint64_t i = 0; i < rec_fit; i++) {  // the per-root summary of the records returned
        const bw_impact_record& r = records[i];
        if (r.root >= n_roots) return im_refuse(c, "a record under a root that was not given");
        bw_impact_root& pr = per_root[r.root];
        pr.n_records++;
        if (r.flags & BW_IMPACT_UNREADABLE) {
            pr.n_unreadable++;
        } else if (r.kind == BW_TREE_FILE) {
            pr.n_files++;
            pr.lost_chunk_refs += r.n_affected;
        }
    }
    counts->n_records = n_rec;
    counts->name_bytes = name_total;
    counts->n_levels = n_levels;
    counts->n_errors = n_err;
    if (full) {
        c->err = "impact: level " + std::to_string(n_levels - 1) + " does not fit record_cap or names_cap";
        return BW_ENOSPC;
    }
    return rc;
}
