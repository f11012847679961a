// bw_diff.hip -- the diff walk (include/backuwup_gpu_pack.h, "diff"): what changed between two roots,
// opening only the tree blobs on a changed path.  The reference has no diff.  The walk is
// level-synchronous and host-driven like prune's mark: the host counts, lays a level's arenas out by
// prefix sums over the parsed headers and feeds the unpack chain `slots` blobs at a time; every
// comparison of hash bytes and name bytes is a kernel's.  Per level:
//   wk_fetch      the nodes' headers, names and chains (bw_walk.h, shared with the parent match):
//                 k_wk_resolve<DfFetch> with the ancestor check, k_wk_take<DfFetch> into the DfNode
//   k_df_rows     the chains' rows gathered into one list per node
//   k_df_join / k_df_pair   the name join of the level's nodes and their records
//   k_df_insert / k_df_compare / k_df_finish   set membership, prefix, suffix, n_new, the next frontier
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/backuwup_gpu.h"
#include "bw_device.h"
#include "bw_internal.h"
#include "bw_ctx.h"
#include "bw_restore.h"
#include "bw_diff.h"

using namespace bw;

// ------------------------------------------------------------------ the fetch's policy
// What the shared fetch (bw_walk.h) leaves to the walk.  An owner is a node of the level.
struct DfFetch {
    typedef DfWalk Walk;
    static constexpr const char* NAME = "diff";
    static constexpr const char* ROWS_TOO_MANY = "a level of more than 2^30 children rows";
    static constexpr uint64_t MAX_ROWS = DF_MAX_ROWS;
    static constexpr uint64_t ERRS_PER_REF = 2;  // the ancestor check's, and the locate's

    // a node's first piece: is its hash one of its ancestors' on its side?  Then it is read for its name only.
    __device__ static bool first(const DfWalk& w, const WkRef& r) {
        const DfNode& nd = w.nodes[r.owner];
        // the parent records upwards on the node's side; each step is one level, so `level` bounds the walk
        uint64_t rec = nd.parent;
        for (uint64_t step = 0; rec != DF_NONE && step <= w.level; step++) {
            const bw_diff_record& p = w.recs[rec];
            const bool present = nd.side ? p.change != BW_DIFF_REMOVED : p.change != BW_DIFF_ADDED;
            if (present && rs_eq(nd.side ? p.b.hash : p.a.hash, r.hash, 32)) {
                wk_error(w.f, r.hash, r.by, r.by_pos, BW_RESTORE_EFORMAT);
                atomicOr(&w.nodes[r.owner].state, DF_CYCLIC);
                return true;
            }
            rec = p.parent;
        }
        return false;
    }

    __device__ static bool refuse(const DfWalk&, uint64_t) { return false; }  // every located piece is opened

    __device__ static void lost(const DfWalk& w, uint32_t node) { atomicOr(&w.nodes[node].state, DF_TRUNC); }

    __device__ static void header(const DfWalk& w, uint32_t node, const RsTreeHdr& h, uint64_t name_off) {
        DfNode& nd = w.nodes[node];
        atomicOr(&nd.state, DF_OK);
        nd.kind = h.kind;
        nd.tflags = h.flags;
        nd.size = h.size;
        nd.mtime = h.mtime;
        nd.ctime = h.ctime;
        nd.name_off = name_off;
        nd.name_len = h.name_len;
    }
};

// ------------------------------------------------------------------ the level's lists
// One lane per row of the final arena: its segment by a binary search of the segments' first rows.
__global__ void __launch_bounds__(256) k_df_rows(DfWalk w) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= w.n_rows) return;
    const uint64_t seg = wk_range_of(w.f.seg_row0, w.f.n_seg, r);  // no segment is empty
    const uint64_t* s = (const uint64_t*)wk_stage_row(w.f, seg, r);
    uint64_t* d = (uint64_t*)(w.rows + 32 * r);
    for (int i = 0; i < 4; i++) d[i] = s[i];
    w.row_seg[r] = (uint32_t)seg;
}

// ------------------------------------------------------------------ the name join
// The key of a readable node: (parent item, side, name).  The roots pair whatever their names.
__device__ static inline uint64_t df_key_len(const DfNode& n) { return n.parent == DF_NONE ? 0 : n.name_len; }

__device__ static uint32_t df_key_hash(const DfWalk& w, const DfNode& n, uint32_t side) {
    return wk_key_hash((n.parent * 0x9e3779b97f4a7c15ull) ^ side, w.f.names + n.name_off, df_key_len(n));
}

__device__ static bool df_key_eq(const DfWalk& w, const DfNode& a, uint32_t a_side, const DfNode& b, uint32_t b_side) {
    if (a.parent != b.parent || a_side != b_side) return false;
    return wk_name_eq(w.f.names + a.name_off, df_key_len(a), w.f.names + b.name_off, df_key_len(b));
}

// One lane per node.  tab[slot] = some node of the key, best[slot] = the lowest (position, node) of
// it: the representative of its name.  The table holds twice the nodes, and a probe ends at cap.
__global__ void __launch_bounds__(256) k_df_join(DfWalk w, uint32_t* tab, uint64_t* best, uint32_t cap) {
    const uint64_t n = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= w.n_nodes) return;
    DfNode& nd = w.nodes[n];
    if (!(nd.state & DF_OK)) return;
    const uint32_t h = df_key_hash(w, nd, nd.side);
    for (uint32_t probe = 0; probe < cap; probe++) {
        const uint32_t slot = (h + probe) & (cap - 1);
        const uint32_t cur = atomicCAS(&tab[slot], RS_EMPTY, (uint32_t)n);
        if (cur == RS_EMPTY || df_key_eq(w, w.nodes[cur], w.nodes[cur].side, nd, nd.side)) {
            atomicMin((unsigned long long*)&best[slot], (unsigned long long)((nd.pos << 32) | n));
            nd.slot = slot;
            return;
        }
    }
}

__device__ static void df_side(bw_diff_side& s, const DfNode* n, uint64_t n_rows) {
    memset(&s, 0, sizeof(s));
    if (!n) return;
    wk_copy32(s.hash, n->hash);
    if (!(n->state & DF_OK)) return;
    s.kind = n->kind;
    s.flags = n->tflags;
    s.size = n->size;
    s.mtime = n->mtime;
    s.ctime = n->ctime;
    s.n_children = n_rows;
}

// One lane per node, after k_df_join.  A node owns a record unless it is the B side of a pair (the
// A side owns that one).  Owners take consecutive records per wave and write them whole.
__global__ void __launch_bounds__(256) k_df_pair(DfWalk w, const uint32_t* tab, const uint64_t* best, uint32_t cap) {
    const uint64_t n = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = n < w.n_nodes;
    bool owner = false;
    uint32_t partner = RS_EMPTY;
    if (active) {
        const DfNode& nd = w.nodes[n];
        owner = true;
        if ((nd.state & DF_OK) && (uint32_t)best[nd.slot] == (uint32_t)n) {
            const uint32_t other = nd.side ^ 1;
            const uint32_t h = df_key_hash(w, nd, other);
            for (uint32_t probe = 0; probe < cap; probe++) {
                const uint32_t slot = (h + probe) & (cap - 1);
                const uint32_t cur = tab[slot];
                if (cur == RS_EMPTY) break;
                if (df_key_eq(w, w.nodes[cur], w.nodes[cur].side, nd, other)) {
                    partner = (uint32_t)best[slot];
                    owner = nd.side == 0;
                    break;
                }
            }
        }
    }
    const uint64_t rec = wk_wave_place(owner, &w.ctr[DF_C_RECORDS]);
    if (!owner) return;
    DfNode& nd = w.nodes[n];
    DfNode* pn = partner == RS_EMPTY ? nullptr : &w.nodes[partner];
    nd.rec = rec;
    nd.partner = partner;
    if (pn) {
        pn->rec = rec;
        pn->partner = (uint32_t)n;
    }
    const DfNode* na = nd.side == 0 ? &nd : pn;
    const DfNode* nb = nd.side == 0 ? pn : &nd;
    const uint64_t ra = na ? w.node_rows[na - w.nodes] : 0, rb = nb ? w.node_rows[nb - w.nodes] : 0;
    bw_diff_record& r = w.recs[rec];
    r.change = na && nb ? (na->kind == nb->kind ? BW_DIFF_MODIFIED : BW_DIFF_TYPE_CHANGED) : (na ? BW_DIFF_REMOVED : BW_DIFF_ADDED);
    r.flags = 0;
    if (na) r.flags |= ((na->state & DF_OK) ? 0 : BW_DIFF_UNREADABLE) | ((na->state & DF_TRUNC) ? BW_DIFF_TRUNCATED : 0);
    if (nb) r.flags |= ((nb->state & DF_OK) ? 0 : BW_DIFF_UNREADABLE) | ((nb->state & DF_TRUNC) ? BW_DIFF_TRUNCATED : 0);
    r.parent = nd.parent;
    const DfNode* name_of = nb ? nb : na;
    const bool named = name_of->state & DF_OK;
    r.name_off = named ? name_of->name_off : 0;
    r.name_len = named ? name_of->name_len : 0;
    df_side(r.a, na, ra);
    df_side(r.b, nb, rb);
    // the first mismatch from either end is found by atomicMin from "none", which is min(n_a, n_b)
    const uint64_t lim = r.change == BW_DIFF_MODIFIED ? (ra < rb ? ra : rb) : 0;
    r.common_prefix = lim;
    r.common_suffix = lim;
    r.n_new = 0;
}

// ------------------------------------------------------------------ compare
// rows of the level's arena are 32-byte aligned
__device__ static inline bool df_row_eq(const uint8_t* a, const uint8_t* b) {
    const uint64_t *x = (const uint64_t*)a, *y = (const uint64_t*)b;
    return ((x[0] ^ y[0]) | (x[1] ^ y[1]) | (x[2] ^ y[2]) | (x[3] ^ y[3])) == 0;
}

__device__ static inline uint32_t df_row_node(const DfWalk& w, uint64_t r) { return w.f.seg_node[w.row_seg[r]]; }

__device__ static inline uint32_t df_row_hash(const uint8_t* row, uint32_t node) {
    return rs_mix(*(const uint64_t*)row ^ ((uint64_t)node << 32) ^ node);
}

// One lane per row.  The rows of the two sides of a MODIFIED item go into one table salted by their
// node (the rs_insert pattern); an equal key already there is enough, sets have no multiplicity.
__global__ void __launch_bounds__(256) k_df_insert(DfWalk w, uint32_t* tab, uint32_t cap) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= w.n_rows) return;
    const uint32_t node = df_row_node(w, r);
    const DfNode& nd = w.nodes[node];
    if (nd.partner == RS_EMPTY || w.recs[nd.rec].change != BW_DIFF_MODIFIED) return;
    const uint8_t* key = w.rows + 32 * r;
    const uint32_t h = df_row_hash(key, node);
    for (uint32_t probe = 0; probe < cap; probe++) {
        const uint32_t slot = (h + probe) & (cap - 1);
        const uint32_t cur = atomicCAS(&tab[slot], RS_EMPTY, (uint32_t)r);
        if (cur == RS_EMPTY) return;
        if (df_row_node(w, cur) == node && df_row_eq(w.rows + 32ull * cur, key)) return;
    }
}

__device__ static bool df_find(const DfWalk& w, const uint32_t* tab, uint32_t cap, const uint8_t* key, uint32_t node) {
    const uint32_t h = df_row_hash(key, node);
    for (uint32_t probe = 0; probe < cap; probe++) {
        const uint32_t cur = tab[(h + probe) & (cap - 1)];
        if (cur == RS_EMPTY) return false;
        if (df_row_node(w, cur) == node && df_row_eq(w.rows + 32ull * cur, key)) return true;
    }
    return false;
}

// One lane per row, after k_df_insert: membership in the other side's set, the mismatches from both
// ends (taken from the A side's rows), n_new, and the next frontier: the unmatched rows of a Dir item,
// every row of a one-sided or type-changed Dir.  next_nodes / next_refs hold a place per row of a Dir node.
__global__ void __launch_bounds__(256) k_df_compare(DfWalk w, const uint32_t* tab, uint32_t cap, DfNode* next_nodes,
                                                    WkRef* next_refs) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = r < w.n_rows;
    bool push = false;
    uint32_t seg = 0, node = 0;
    uint64_t k = 0;
    if (active) {
        seg = w.row_seg[r];
        node = w.f.seg_node[seg];
        const DfNode& nd = w.nodes[node];
        const uint8_t* row = w.rows + 32 * r;
        k = r - w.node_row0[node];
        bw_diff_record& rec = w.recs[nd.rec];
        if (rec.change == BW_DIFF_MODIFIED) {
            const uint32_t pn = nd.partner;
            const uint64_t n_own = w.node_rows[node], n_oth = w.node_rows[pn];
            const uint8_t* oth = w.rows + 32 * w.node_row0[pn];
            const bool found = df_find(w, tab, cap, row, pn);
            if (nd.side == 1 && !found) atomicAdd((unsigned long long*)&rec.n_new, 1ull);
            if (nd.side == 0) {
                if (k < n_oth && !df_row_eq(row, oth + 32 * k)) atomicMin((unsigned long long*)&rec.common_prefix, (unsigned long long)k);
                const uint64_t s = n_own - 1 - k;
                if (s < n_oth && !df_row_eq(row, oth + 32 * (n_oth - 1 - s)))
                    atomicMin((unsigned long long*)&rec.common_suffix, (unsigned long long)s);
            }
            push = !found && nd.kind == BW_TREE_DIR;
        } else {
            push = nd.kind == BW_TREE_DIR;
        }
    }
    const uint64_t j = wk_wave_place(push, &w.ctr[DF_C_NEXT]);
    if (!push) return;  // at most one place per row of a Dir node: the lists hold that many
    const DfNode& nd = w.nodes[node];
    const uint8_t* row = w.rows + 32 * r;
    DfNode& x = next_nodes[j];
    memset(&x, 0, sizeof(x));
    wk_copy32(x.hash, row);
    x.parent = nd.rec;
    x.pos = k;
    x.side = nd.side;
    x.partner = RS_EMPTY;
    WkRef& f = next_refs[j];
    wk_copy32(f.hash, row);
    wk_copy32(f.by, w.f.seg_hash + 32ull * w.f.seg_sid[seg]);
    f.by_pos = r - w.f.seg_row0[seg];
    f.owner = (uint32_t)j;
    f.pad = 0;
}

// One lane per node: the owner of a MODIFIED record caps its suffix at min(n_a, n_b) - common_prefix.
__global__ void __launch_bounds__(256) k_df_finish(DfWalk w) {
    const uint64_t n = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= w.n_nodes) return;
    const DfNode& nd = w.nodes[n];
    if (nd.side != 0 || nd.partner == RS_EMPTY) return;
    bw_diff_record& r = w.recs[nd.rec];
    if (r.change != BW_DIFF_MODIFIED) return;
    const uint64_t lim = r.a.n_children < r.b.n_children ? r.a.n_children : r.b.n_children;
    if (r.common_suffix > lim - r.common_prefix) r.common_suffix = lim - r.common_prefix;
}

// ------------------------------------------------------------------ the host's side
static int df_refuse(bw_ctx* c, const char* why) { return wk_refuse(c, DfFetch::NAME, why); }

extern "C" int bw_diff_trees(bw_restore* s, const uint8_t* root_a, const uint8_t* root_b, uint32_t flags,
                             bw_diff_record* records, uint64_t record_cap, uint8_t* names, uint64_t names_cap,
                             uint8_t* read, bw_diff_counts* counts, bw_prune_error* errs, uint64_t err_cap) {
    if (!s || !counts || (flags & ~BW_UNPACK_VERIFY) || (record_cap && !records) || (names_cap && !names) ||
        (err_cap && !errs) || (!s->entries.empty() && !read))
        return BW_EINVAL;
    bw_ctx* c = s->c;
    hipSetDevice(c->device);
    const uint64_t n_e = s->entries.size();
    memset(counts, 0, sizeof(*counts));
    if (n_e) memset(read, 0, n_e);
    if ((!root_a && !root_b) || (root_a && root_b && !memcmp(root_a, root_b, 32))) return BW_OK;

    WkHost<DfFetch> H;
    if (int rc = wk_open(H, s, flags)) return rc;
    DfWalk& w = H.w;
    w.ctr = P<uint64_t>(s->wk[WK_B_CTR]);

    // level 0: the roots
    int lv = 0;
    uint64_t n_nodes = 0;
    {
        DfNode hn[2];
        WkRef hr[2];
        memset(hn, 0, sizeof(hn));
        memset(hr, 0, sizeof(hr));
        const uint8_t* roots[2] = {root_a, root_b};
        for (uint32_t side = 0; side < 2; side++) {
            if (!roots[side]) continue;
            DfNode& n = hn[n_nodes];
            memcpy(n.hash, roots[side], 32);
            n.parent = DF_NONE;
            n.side = side;
            n.partner = RS_EMPTY;
            WkRef& r = hr[n_nodes];
            memcpy(r.hash, roots[side], 32);
            r.by_pos = side;
            r.owner = (uint32_t)n_nodes++;
        }
        if (int rc = ensure(c, s->df[DF_B_NODES0 + lv], sizeof(hn))) return rc;
        if (int rc = ensure(c, s->df[DF_B_REFS0 + lv], sizeof(hr))) return rc;
        HIPCHK(c, hipMemcpyAsync(s->df[DF_B_NODES0 + lv].p, hn, sizeof(hn), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(s->df[DF_B_REFS0 + lv].p, hr, sizeof(hr), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // hn and hr leave scope
    }

    uint64_t n_rec = 0, n_levels = 0;
    uint64_t rec_fit = 0, names_fit = 0;  // the totals of the levels that fit the caller's arrays
    uint64_t& name_total = H.lv.name_total;  // the names of every level so far
    bool full = false;
    std::vector<uint64_t> lvl;

    while (n_nodes) {
        // a node that is expanded has a located hash no ancestor of its side has: a path is no longer than the table
        if (n_levels > n_e + 1) return df_refuse(c, "more levels than the store has entries");
        if (n_nodes > DF_MAX_ROWS) return wk_too_large(c, DfFetch::NAME, "a level of more than 2^30 nodes");
        w.level = n_levels++;
        w.nodes = P<DfNode>(s->df[DF_B_NODES0 + lv]);
        w.n_nodes = n_nodes;
        H.owners.assign(n_nodes, WkOwner());
        H.lv.segs.clear();
        H.lv.stage_rows = 0;

        // ---- read: every node's header and name, and every row of every piece of its chain (bw_walk.h)
        if (int rc = wk_fetch(H, P<WkRef>(s->df[DF_B_REFS0 + lv]), n_nodes, true, true, H.owners.data())) return rc;

        // ---- the level's lists: node after node, a chain's segments in chain order
        // the walk's own tables between the segments': [node_row0 | node_rows]
        const uint64_t n_rows = H.lv.stage_rows;
        wk_level_tables(w.f, H.lv.segs, lvl, 2 * n_nodes);
        const uint64_t n_seg = w.f.n_seg;
        uint64_t* node_row0 = lvl.data() + 2 * n_seg + 1;
        uint64_t* node_rows = node_row0 + n_nodes;
        uint64_t run = 0, dir_rows = 0;  // only a row of a Dir node can become a node of the next level
        for (uint64_t i = 0; i < n_nodes; i++) {
            node_row0[i] = run;
            node_rows[i] = H.owners[i].n_rows;
            run += H.owners[i].n_rows;
            if (H.owners[i].dir) dir_rows += H.owners[i].n_rows;
        }
        if (run != n_rows) return df_refuse(c, "the level's rows do not add up");
        if (int rc = ensure(c, s->df[DF_B_LVL], 8 * lvl.size() + 16)) return rc;
        if (int rc = ensure(c, s->df[DF_B_ROWS], 32 * n_rows + 32)) return rc;
        if (int rc = ensure(c, s->df[DF_B_ROWSEG], 4 * n_rows + 16)) return rc;
        HIPCHK(c, hipMemcpyAsync(s->df[DF_B_LVL].p, lvl.data(), 8 * lvl.size(), hipMemcpyHostToDevice, c->stream));
        wk_level_pointers(w.f, P<uint64_t>(s->df[DF_B_LVL]), 2 * n_nodes);
        w.node_row0 = w.f.seg_stage + n_seg;
        w.node_rows = w.node_row0 + n_nodes;
        w.rows = P<uint8_t>(s->df[DF_B_ROWS]);
        w.row_seg = P<uint32_t>(s->df[DF_B_ROWSEG]);
        w.n_rows = n_rows;
        w.f.stage = P<uint8_t>(s->wk[WK_B_STAGE]);
        w.f.seg_hash = P<uint8_t>(s->wk[WK_B_SEGHASH]);
        w.f.names = P<uint8_t>(s->wk[WK_B_NAMES]);
        if (n_rows) hipLaunchKernelGGL(k_df_rows, wk_grid(n_rows), dim3(256), 0, c->stream, w);

        // ---- the name join and the records: a node gives one record at most
        const uint32_t ncap = df_table_cap(n_nodes);
        DevBuf& rec_buf = s->df[DF_B_REC];
        if (int rc = ensure(c, s->df[DF_B_TAB], 12ull * ncap + 16)) return rc;
        if (int rc = wk_grow(c, DfFetch::NAME, rec_buf, (n_rec + n_nodes) * sizeof(bw_diff_record) + 16, n_rec * sizeof(bw_diff_record)))
            return rc;
        uint64_t* d_best = P<uint64_t>(s->df[DF_B_TAB]);
        uint32_t* d_ntab = (uint32_t*)(d_best + ncap);
        w.recs = P<bw_diff_record>(rec_buf);
        HIPCHK(c, hipMemsetAsync(s->df[DF_B_TAB].p, 0xff, 12ull * ncap, c->stream));
        hipLaunchKernelGGL(k_df_join, wk_grid(n_nodes), dim3(256), 0, c->stream, w, d_ntab, d_best, ncap);
        hipLaunchKernelGGL(k_df_pair, wk_grid(n_nodes), dim3(256), 0, c->stream, w, d_ntab, d_best, ncap);

        // ---- compare, and the next frontier: a row gives one node at most
        if (n_rows) {
            const uint32_t rcap = df_table_cap(n_rows);
            DevBuf &rtab = s->df[DF_B_RTAB], &next_nodes = s->df[DF_B_NODES0 + (lv ^ 1)], &next_refs = s->df[DF_B_REFS0 + (lv ^ 1)];
            if (int rc = ensure(c, rtab, 4ull * rcap + 16)) return rc;
            if (int rc = ensure(c, next_nodes, dir_rows * sizeof(DfNode) + 16)) return rc;
            if (int rc = ensure(c, next_refs, dir_rows * sizeof(WkRef) + 16)) return rc;
            HIPCHK(c, hipMemsetAsync(rtab.p, 0xff, 4ull * rcap, c->stream));
            HIPCHK(c, hipMemsetAsync(&w.ctr[DF_C_NEXT], 0, 8, c->stream));
            hipLaunchKernelGGL(k_df_insert, wk_grid(n_rows), dim3(256), 0, c->stream, w, P<uint32_t>(rtab), rcap);
            hipLaunchKernelGGL(k_df_compare, wk_grid(n_rows), dim3(256), 0, c->stream, w, P<uint32_t>(rtab), rcap,
                               P<DfNode>(next_nodes), P<WkRef>(next_refs));
            hipLaunchKernelGGL(k_df_finish, wk_grid(n_nodes), dim3(256), 0, c->stream, w);
        }
        HIPCHK(c, hipGetLastError());
        uint64_t ctr[WK_C_COUNT];
        HIPCHK(c, hipMemcpyAsync(ctr, w.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const uint64_t n_next = n_rows ? ctr[DF_C_NEXT] : 0;
        if (ctr[DF_C_RECORDS] < n_rec || ctr[DF_C_RECORDS] > n_rec + n_nodes || n_next > dir_rows)
            return df_refuse(c, "a level's record or frontier count that cannot be");
        n_rec = ctr[DF_C_RECORDS];
        if (n_rec > record_cap || name_total > names_cap) {
            full = true;
            break;
        }
        rec_fit = n_rec;
        names_fit = name_total;
        n_nodes = n_next;
        lv ^= 1;
    }

    // ---- results
    uint64_t n_err = 0;
    HIPCHK(c, hipMemcpyAsync(&n_err, w.f.n_err, 8, hipMemcpyDeviceToHost, c->stream));
    if (n_e) HIPCHK(c, hipMemcpyAsync(read, w.f.read, n_e, hipMemcpyDeviceToHost, c->stream));
    if (rec_fit) HIPCHK(c, hipMemcpyAsync(records, s->df[DF_B_REC].p, rec_fit * sizeof(bw_diff_record), hipMemcpyDeviceToHost, c->stream));
    if (names_fit) HIPCHK(c, hipMemcpyAsync(names, s->wk[WK_B_NAMES].p, names_fit, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int rc = wk_errors_out(H, n_err, errs, err_cap);
    if (rc != BW_OK && rc != BW_ENOSPC) return rc;
    counts->n_records = n_rec;
    counts->name_bytes = name_total;
    counts->n_levels = n_levels;
    counts->n_errors = n_err;
    for (uint64_t e = 0; e < n_e; e++) counts->n_read += read[e];
    if (full) {
        c->err = "diff: level " + std::to_string(n_levels - 1) + " does not fit record_cap or names_cap";
        return BW_ENOSPC;
    }
    return rc;
}
