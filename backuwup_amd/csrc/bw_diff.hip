// bw_diff.hip -- the diff walk (include/backuwup_gpu_pack.h, "diff"): what changed between two roots,
// opening only the tree blobs on a changed path.  The reference has no diff.  The walk is
// level-synchronous and host-driven like prune's mark: the host counts, lays a level's arenas out by
// prefix sums over the parsed headers and feeds the unpack chain `slots` blobs at a time; every
// comparison of hash bytes and name bytes is a kernel's.  Per level:
//   k_df_resolve  one lane per reference: locate, kind, the ancestor check, read[]
//   k_df_take     one workgroup per decoded blob: header, name and children rows out of the slot
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

// ------------------------------------------------------------------ device helpers
__device__ static void df_error(const DfWalk& w, const uint8_t* hash, const uint8_t* by, uint64_t pos, uint32_t reason) {
    const uint64_t at = atomicAdd((unsigned long long*)&w.ctr[DF_C_ERRORS], 1ull);
    if (at >= w.err_cap) return;  // the host sized the list for every error a launch can give
    bw_prune_error& e = w.errs[at];
    for (int i = 0; i < 32; i++) {
        e.hash[i] = hash[i];
        e.parent[i] = by[i];
    }
    e.child_pos = pos;
    e.reason = reason;
    e.pad = 0;
}

__device__ static inline void df_copy32(uint8_t* d, const uint8_t* s) {
    for (int i = 0; i < 32; i++) d[i] = s[i];
}

// rows of the level's arena are 32-byte aligned
__device__ static inline bool df_row_eq(const uint8_t* a, const uint8_t* b) {
    const uint64_t *x = (const uint64_t*)a, *y = (const uint64_t*)b;
    return ((x[0] ^ y[0]) | (x[1] ^ y[1]) | (x[2] ^ y[2]) | (x[3] ^ y[3])) == 0;
}

// Every lane of the wave calls this: the lanes with push = true get consecutive places from *ctr
// (one atomic by the first of them, each lane's place from the ballot, as prune's pr_visit does).
__device__ static inline uint64_t df_wave_place(bool push, uint64_t* ctr) {
    const uint64_t bal = __ballot(push);
    if (!bal) return 0;
    const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__ffsll((unsigned long long)bal) - 1;
    uint64_t base = 0;
    if (lane == leader) base = atomicAdd((unsigned long long*)ctr, (unsigned long long)__popcll(bal));
    const uint32_t lo = __shfl((uint32_t)base, leader), hi = __shfl((uint32_t)(base >> 32), leader);
    return (((uint64_t)hi << 32) | lo) + __popcll(bal & ((1ull << lane) - 1));
}

// ------------------------------------------------------------------ resolve
// out[i] = the entry the reference names (low 32 bits, RS_EMPTY when there is none to open) and,
// in bit 32, whether the node is cyclic.  overlong: the chain has more pieces than the store has
// entries, so every reference of the round is refused unread.
__global__ void __launch_bounds__(256) k_df_resolve(DfWalk w, const DfRef* refs, uint64_t n, int round0, int overlong,
                                                    uint64_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DfRef& r = refs[i];
    DfNode& nd = w.nodes[r.node];
    uint64_t res = RS_EMPTY;
    if (overlong) {
        df_error(w, r.hash, r.by, r.by_pos, BW_RESTORE_EFORMAT);
        atomicOr(&nd.state, DF_TRUNC);
        out[i] = res;
        return;
    }
    bool cyc = false;
    if (round0) {
        // the parent records upwards on the node's side; each step is one level, so `level` bounds the walk
        uint64_t rec = nd.parent;
        for (uint64_t step = 0; rec != DF_NONE && step <= w.level; step++) {
            const bw_diff_record& p = w.recs[rec];
            const bool present = nd.side ? p.change != BW_DIFF_REMOVED : p.change != BW_DIFF_ADDED;
            if (present && rs_eq(nd.side ? p.b.hash : p.a.hash, r.hash, 32)) {
                cyc = true;
                break;
            }
            rec = p.parent;
        }
        if (cyc) {
            df_error(w, r.hash, r.by, r.by_pos, BW_RESTORE_EFORMAT);
            atomicOr(&nd.state, DF_CYCLIC);
        }
    }
    uint64_t e;
    const uint8_t st = rs_locate_one(w.loc, r.hash, e);
    if (st) {
        df_error(w, r.hash, r.by, r.by_pos, st);
    } else if (w.loc.entries[e].kind != BW_BLOB_TREE) {
        df_error(w, r.hash, r.by, r.by_pos, BW_RESTORE_ENOTTREE);
    } else {
        w.read[e] = 1;
        res = e;
    }
    if (res == RS_EMPTY && !round0) atomicOr(&nd.state, DF_TRUNC);
    out[i] = res | (cyc ? 1ull << 32 : 0);
}

// ------------------------------------------------------------------ take
// Workgroup b: blob b of the sub-batch, decoded at slots + off[b] and parsed into hdr[b].  A blob the
// chain or the parser refused is an error of its reference.  A good one gives the node its header and
// name (round 0), its rows to the staging arena, and its next_sibling to the next round.
__global__ void __launch_bounds__(256) k_df_take(DfWalk w, const DfRef* refs, const DfTake* tab, const uint8_t* slots,
                                                 const uint64_t* off, const RsTreeHdr* hdr, uint64_t m, int round0,
                                                 DfRef* next) {
    const uint64_t b = blockIdx.x;
    if (b >= m) return;
    const DfTake t = tab[b];
    const DfRef& r = refs[t.ref];
    DfNode& nd = w.nodes[r.node];
    const RsTreeHdr& h = hdr[b];
    const uint32_t bad = t.cst ? t.cst : h.status;
    if (bad) {
        if (threadIdx.x == 0) {
            df_error(w, r.hash, r.by, r.by_pos, bad);
            if (!round0) atomicOr(&nd.state, DF_TRUNC);
        }
        return;
    }
    const uint8_t* blob = slots + off[b];
    if (threadIdx.x == 0) {
        if (round0) {
            atomicOr(&nd.state, DF_OK);
            nd.kind = h.kind;
            nd.tflags = h.flags;
            nd.size = h.size;
            nd.mtime = h.mtime;
            nd.ctime = h.ctime;
            nd.name_off = t.name_off;
            nd.name_len = h.name_len;
        }
        if (t.seg != DF_NONE) df_copy32(w.seg_hash + 32 * t.seg, r.hash);
        if (t.next != DF_NONE) {
            DfRef& x = next[t.next];
            df_copy32(x.hash, h.next);
            df_copy32(x.by, r.hash);
            x.by_pos = DF_NONE;
            x.node = r.node;
            x.pad = 0;
        }
    }
    // the parser bounded the name and the rows by the blob; a name is short and goes byte by byte
    if (round0)
        for (uint64_t i = threadIdx.x; i < h.name_len; i += 256) w.names[t.name_off + i] = blob[h.name_pos + i];
    // the rows: each wave takes pieces of RS_PIECE bytes and copies them in 16-byte vectors (the
    // strict form of the gather's copy: ch_pos lies at any byte, and nothing outside the rows is loaded)
    const uint8_t* src = blob + h.ch_pos;
    uint8_t* dst = w.stage + 32 * t.stage;
    const uint64_t nb = 32 * t.n_rows;  // t.n_rows <= h.n_children
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t p0 = (uint64_t)(threadIdx.x >> 6) * RS_PIECE; p0 < nb; p0 += 4ull * RS_PIECE)
        rs_copy_piece<true>(src + p0, dst + p0, nb - p0 < RS_PIECE ? nb - p0 : RS_PIECE, lane);
}

// ------------------------------------------------------------------ the level's lists
// One lane per row of the final arena: its segment by a binary search of the segments' first rows.
__global__ void __launch_bounds__(256) k_df_rows(DfWalk w) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= w.n_rows) return;
    uint64_t lo = 0, hi = w.n_seg;  // seg_row0[lo] <= r < seg_row0[hi]; no segment is empty
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (w.seg_row0[mid] <= r) lo = mid; else hi = mid;
    }
    const uint64_t* s = (const uint64_t*)(w.stage + 32 * (w.seg_stage[lo] + (r - w.seg_row0[lo])));
    uint64_t* d = (uint64_t*)(w.rows + 32 * r);
    for (int i = 0; i < 4; i++) d[i] = s[i];
    w.row_seg[r] = (uint32_t)lo;
}

// ------------------------------------------------------------------ the name join
// The key of a readable node: (parent item, side, name).  The roots pair whatever their names.
__device__ static inline uint64_t df_key_len(const DfNode& n) { return n.parent == DF_NONE ? 0 : n.name_len; }

__device__ static uint32_t df_key_hash(const DfWalk& w, const DfNode& n, uint32_t side) {
    uint64_t h = 0xcbf29ce484222325ull ^ (n.parent * 0x9e3779b97f4a7c15ull) ^ side;
    const uint8_t* p = w.names + n.name_off;
    const uint64_t len = df_key_len(n);
    for (uint64_t i = 0; i < len; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return rs_mix(h);
}

__device__ static bool df_key_eq(const DfWalk& w, const DfNode& a, uint32_t a_side, const DfNode& b, uint32_t b_side) {
    if (a.parent != b.parent || a_side != b_side) return false;
    const uint64_t len = df_key_len(a);
    if (len != df_key_len(b)) return false;
    const uint8_t *x = w.names + a.name_off, *y = w.names + b.name_off;
    uint32_t d = 0;
    for (uint64_t i = 0; i < len; i++) d |= x[i] ^ y[i];
    return d == 0;
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
    df_copy32(s.hash, n->hash);
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
    const uint64_t rec = df_wave_place(owner, &w.ctr[DF_C_RECORDS]);
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
__device__ static inline uint32_t df_row_node(const DfWalk& w, uint64_t r) { return w.seg_node[w.row_seg[r]]; }

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
                                                    DfRef* next_refs) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = r < w.n_rows;
    bool push = false;
    uint32_t seg = 0, node = 0;
    uint64_t k = 0;
    if (active) {
        seg = w.row_seg[r];
        node = w.seg_node[seg];
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
    const uint64_t j = df_wave_place(push, &w.ctr[DF_C_NEXT]);
    if (!push) return;  // at most one place per row of a Dir node: the lists hold that many
    const DfNode& nd = w.nodes[node];
    const uint8_t* row = w.rows + 32 * r;
    DfNode& x = next_nodes[j];
    memset(&x, 0, sizeof(x));
    df_copy32(x.hash, row);
    x.parent = nd.rec;
    x.pos = k;
    x.side = nd.side;
    x.partner = RS_EMPTY;
    DfRef& f = next_refs[j];
    df_copy32(f.hash, row);
    df_copy32(f.by, w.seg_hash + 32ull * w.seg_sid[seg]);
    f.by_pos = r - w.seg_row0[seg];
    f.node = (uint32_t)j;
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
static inline dim3 df_grid(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

// a buffer of at least `need` bytes that keeps its first `keep` bytes
static int df_grow(bw_ctx* c, DevBuf& b, uint64_t need, uint64_t keep) {
    if (b.cap >= need) return BW_OK;
    DevBuf nb;
    if (int rc = ensure(c, nb, need + need / 2)) return rc;
    if (keep && b.p) {
        hipError_t e = hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            free_dev(nb);
            c->err = std::string("diff: growing a buffer: ") + hipGetErrorString(e);
            return BW_EHIP;
        }
    } else {
        hipStreamSynchronize(c->stream);
    }
    free_dev(b);
    b = nb;
    return BW_OK;
}

namespace {
struct HostNode {
    bool ok = false, cyclic = false, dir = false;
    uint64_t n_rows = 0;
};
struct HostSeg {
    uint32_t node, sid;
    uint64_t stage, count;
};
}  // namespace

static int df_refuse(bw_ctx* c, const char* why) {
    c->err = std::string("diff: ") + why;
    return BW_EHIP;
}

// the walk's hard limit: a level of more than DF_MAX_ROWS nodes or children rows
static int df_too_large(bw_ctx* c, const char* what) {
    c->err = std::string("diff: a level of more than 2^30 ") + what + ": the walk's tables index a level in 32 bits";
    return BW_ENOMEM;
}

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

    DfWalk w;
    memset(&w, 0, sizeof(w));
    w.loc = rs_locator(s);
    if (int rc = ensure(c, s->df_ctr, 8 * DF_C_COUNT)) return rc;
    if (int rc = ensure(c, s->df_read, n_e + 16)) return rc;
    HIPCHK(c, hipMemsetAsync(s->df_ctr.p, 0, 8 * DF_C_COUNT, c->stream));
    HIPCHK(c, hipMemsetAsync(s->df_read.p, 0, n_e + 16, c->stream));
    w.ctr = P<uint64_t>(s->df_ctr);
    w.read = P<uint8_t>(s->df_read);

    // level 0: the roots
    int lv = 0;
    uint64_t n_nodes = 0;
    {
        DfNode hn[2];
        DfRef hr[2];
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
            DfRef& r = hr[n_nodes];
            memcpy(r.hash, roots[side], 32);
            r.by_pos = side;
            r.node = (uint32_t)n_nodes++;
        }
        if (int rc = ensure(c, s->df_nodes[lv], sizeof(hn))) return rc;
        if (int rc = ensure(c, s->df_refs[lv], sizeof(hr))) return rc;
        HIPCHK(c, hipMemcpyAsync(s->df_nodes[lv].p, hn, sizeof(hn), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(s->df_refs[lv].p, hr, sizeof(hr), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // hn and hr leave scope
    }

    uint64_t err_ub = 0;      // no more errors than this can have been written
    uint64_t n_rec = 0, name_total = 0, n_levels = 0;
    uint64_t rec_fit = 0, names_fit = 0;  // the totals of the levels that fit the caller's arrays
    bool full = false;
    std::vector<uint64_t> out, eidx, lvl;
    std::vector<uint32_t> ref_node, next_ref_node, located;
    std::vector<uint8_t> bst;
    std::vector<RsTreeHdr> hd;
    std::vector<DfTake> take;
    std::vector<HostNode> hn;
    std::vector<HostSeg> segs;
    auto errs_for = [&](uint64_t more) {  // room for `more` further errors
        err_ub += more;
        if (int rc = df_grow(c, s->df_err, err_ub * sizeof(bw_prune_error) + 16, (err_ub - more) * sizeof(bw_prune_error))) return rc;
        w.errs = P<bw_prune_error>(s->df_err);
        w.err_cap = err_ub;
        return (int)BW_OK;
    };

    while (n_nodes) {
        // a node that is expanded has a located hash no ancestor of its side has: a path is no longer than the table
        if (n_levels > n_e + 1) return df_refuse(c, "more levels than the store has entries");
        if (n_nodes > DF_MAX_ROWS) return df_too_large(c, "nodes");
        w.level = n_levels++;
        w.nodes = P<DfNode>(s->df_nodes[lv]);
        w.n_nodes = n_nodes;
        hn.assign(n_nodes, HostNode());
        segs.clear();
        uint64_t stage_rows = 0;

        // ---- read: round r fetches piece r of every chain that has one, `slots` blobs at a time
        const DfRef* d_refs = P<DfRef>(s->df_refs[lv]);
        uint64_t n_refs = n_nodes;
        ref_node.resize(n_nodes);
        for (uint64_t i = 0; i < n_nodes; i++) ref_node[i] = (uint32_t)i;
        int ch = 0;
        for (uint64_t round = 0; n_refs; round++) {
            const bool round0 = round == 0, overlong = round > n_e;
            if (round > n_e + 1) return df_refuse(c, "a chain round past the refused one");
            if (int rc = errs_for(2 * n_refs)) return rc;
            if (int rc = ensure(c, s->df_out, 8 * n_refs + 16)) return rc;
            hipLaunchKernelGGL(k_df_resolve, df_grid(n_refs), dim3(256), 0, c->stream, w, d_refs, n_refs, (int)round0,
                               (int)overlong, P<uint64_t>(s->df_out));
            HIPCHK(c, hipGetLastError());
            out.resize(n_refs);
            HIPCHK(c, hipMemcpyAsync(out.data(), s->df_out.p, 8 * n_refs, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            located.clear();
            for (uint64_t i = 0; i < n_refs; i++) {
                const uint32_t e = (uint32_t)out[i];
                if (round0) hn[ref_node[i]].cyclic = (out[i] >> 32) & 1;
                if (e == RS_EMPTY) continue;
                if (e >= n_e) return df_refuse(c, "a reference resolved to an entry outside the table");
                located.push_back((uint32_t)i);
            }
            const int nx = ch;  // the next round's references: the chain buffer this round does not read
            if (int rc = ensure(c, s->df_chain[nx], located.size() * sizeof(DfRef) + 16)) return rc;
            DfRef* d_next = P<DfRef>(s->df_chain[nx]);
            next_ref_node.clear();
            for (uint64_t lo = 0; lo < located.size(); lo += s->slots) {
                const uint64_t m = std::min<uint64_t>(s->slots, located.size() - lo);
                eidx.resize(m);
                for (uint64_t k = 0; k < m; k++) eidx[k] = (uint32_t)out[located[lo + k]];
                RsTables t;
                if (int rc = rs_tree_decode(s, eidx, flags, m, t, bst)) return rc;
                if (int rc = rs_tree_parse(s, t, m, &hd)) return rc;
                HIPCHK(c, hipStreamSynchronize(c->stream));
                take.assign(m, DfTake());
                uint64_t add_rows = 0, add_names = 0, add_segs = 0;
                for (uint64_t k = 0; k < m; k++) {
                    DfTake& tk = take[k];
                    const RsTreeHdr& h = hd[k];
                    const uint32_t node = ref_node[located[lo + k]];
                    tk.ref = located[lo + k];
                    tk.cst = bst[k];
                    tk.stage = stage_rows + add_rows;
                    tk.name_off = name_total + add_names;
                    tk.next = tk.seg = DF_NONE;
                    if (tk.cst || h.status) continue;
                    HostNode& x = hn[node];
                    if (round0) {
                        x.ok = true;
                        x.dir = h.kind == BW_TREE_DIR;
                        add_names += h.name_len;
                    }
                    if (x.cyclic) continue;  // read for its name: no rows, no chain
                    tk.n_rows = h.n_children;
                    if (h.n_children) {
                        tk.seg = segs.size();
                        segs.push_back(HostSeg{node, (uint32_t)segs.size(), tk.stage, h.n_children});
                        add_segs++;
                        add_rows += h.n_children;
                        x.n_rows += h.n_children;
                    }
                    if (h.has_next) {
                        tk.next = next_ref_node.size();
                        next_ref_node.push_back(node);
                    }
                }
                if (stage_rows + add_rows > DF_MAX_ROWS) return df_too_large(c, "children rows");
                if (int rc = df_grow(c, s->df_stage, 32 * (stage_rows + add_rows) + 32, 32 * stage_rows)) return rc;
                if (int rc = df_grow(c, s->df_seghash, 32 * segs.size() + 32, 32 * (segs.size() - add_segs))) return rc;
                if (int rc = df_grow(c, s->df_names, name_total + add_names + 16, name_total)) return rc;
                if (int rc = errs_for(m)) return rc;
                if (int rc = ensure(c, s->df_take, m * sizeof(DfTake) + 16)) return rc;
                w.stage = P<uint8_t>(s->df_stage);
                w.seg_hash = P<uint8_t>(s->df_seghash);
                w.names = P<uint8_t>(s->df_names);
                HIPCHK(c, hipMemcpyAsync(s->df_take.p, take.data(), m * sizeof(DfTake), hipMemcpyHostToDevice, c->stream));
                hipLaunchKernelGGL(k_df_take, dim3((uint32_t)m), dim3(256), 0, c->stream, w, d_refs, P<DfTake>(s->df_take),
                                   P<uint8_t>(s->slot_buf), t.slot_off, P<RsTreeHdr>(s->q), m, (int)round0, d_next);
                HIPCHK(c, hipGetLastError());
                stage_rows += add_rows;
                name_total += add_names;
                // the slots, the tables and the take table are reused by the next sub-batch
                HIPCHK(c, hipStreamSynchronize(c->stream));
            }
            d_refs = d_next;
            n_refs = next_ref_node.size();
            ref_node.swap(next_ref_node);
            ch ^= 1;
        }

        // ---- the level's lists: node after node, a chain's segments in chain order
        std::stable_sort(segs.begin(), segs.end(), [](const HostSeg& a, const HostSeg& b) { return a.node < b.node; });
        const uint64_t n_seg = segs.size(), n_rows = stage_rows;
        // [seg_row0 (n_seg + 1) | seg_stage | node_row0 | node_rows | seg_node, seg_sid (u32 each)]
        lvl.assign(2 * n_seg + 1 + 2 * n_nodes + n_seg + 1, 0);
        uint64_t* seg_row0 = lvl.data();
        uint64_t* seg_stage = seg_row0 + n_seg + 1;
        uint64_t* node_row0 = seg_stage + n_seg;
        uint64_t* node_rows = node_row0 + n_nodes;
        uint32_t* seg_node = (uint32_t*)(node_rows + n_nodes);
        uint32_t* seg_sid = seg_node + n_seg;
        uint64_t run = 0;
        for (uint64_t k = 0; k < n_seg; k++) {
            seg_row0[k] = run;
            seg_stage[k] = segs[k].stage;
            seg_node[k] = segs[k].node;
            seg_sid[k] = segs[k].sid;
            run += segs[k].count;
        }
        seg_row0[n_seg] = run;
        run = 0;
        uint64_t dir_rows = 0;  // only a row of a Dir node can become a node of the next level
        for (uint64_t i = 0; i < n_nodes; i++) {
            node_row0[i] = run;
            node_rows[i] = hn[i].n_rows;
            run += hn[i].n_rows;
            if (hn[i].dir) dir_rows += hn[i].n_rows;
        }
        if (run != n_rows) return df_refuse(c, "the level's rows do not add up");
        if (int rc = ensure(c, s->df_lvl, 8 * lvl.size() + 16)) return rc;
        if (int rc = ensure(c, s->df_rows, 32 * n_rows + 32)) return rc;
        if (int rc = ensure(c, s->df_rowseg, 4 * n_rows + 16)) return rc;
        HIPCHK(c, hipMemcpyAsync(s->df_lvl.p, lvl.data(), 8 * lvl.size(), hipMemcpyHostToDevice, c->stream));
        const uint64_t* d_lvl = P<uint64_t>(s->df_lvl);
        w.seg_row0 = d_lvl;
        w.seg_stage = d_lvl + n_seg + 1;
        w.node_row0 = w.seg_stage + n_seg;
        w.node_rows = w.node_row0 + n_nodes;
        w.seg_node = (const uint32_t*)(w.node_rows + n_nodes);
        w.seg_sid = w.seg_node + n_seg;
        w.rows = P<uint8_t>(s->df_rows);
        w.row_seg = P<uint32_t>(s->df_rowseg);
        w.n_seg = n_seg;
        w.n_rows = n_rows;
        w.stage = P<uint8_t>(s->df_stage);
        w.seg_hash = P<uint8_t>(s->df_seghash);
        w.names = P<uint8_t>(s->df_names);
        if (n_rows) hipLaunchKernelGGL(k_df_rows, df_grid(n_rows), dim3(256), 0, c->stream, w);

        // ---- the name join and the records: a node gives one record at most
        const uint32_t ncap = df_table_cap(n_nodes);
        if (int rc = ensure(c, s->df_tab, 12ull * ncap + 16)) return rc;
        if (int rc = df_grow(c, s->df_rec, (n_rec + n_nodes) * sizeof(bw_diff_record) + 16, n_rec * sizeof(bw_diff_record))) return rc;
        uint64_t* d_best = P<uint64_t>(s->df_tab);
        uint32_t* d_ntab = (uint32_t*)(d_best + ncap);
        w.recs = P<bw_diff_record>(s->df_rec);
        HIPCHK(c, hipMemsetAsync(s->df_tab.p, 0xff, 12ull * ncap, c->stream));
        hipLaunchKernelGGL(k_df_join, df_grid(n_nodes), dim3(256), 0, c->stream, w, d_ntab, d_best, ncap);
        hipLaunchKernelGGL(k_df_pair, df_grid(n_nodes), dim3(256), 0, c->stream, w, d_ntab, d_best, ncap);

        // ---- compare, and the next frontier: a row gives one node at most
        if (n_rows) {
            const uint32_t rcap = df_table_cap(n_rows);
            if (int rc = ensure(c, s->df_rtab, 4ull * rcap + 16)) return rc;
            if (int rc = ensure(c, s->df_nodes[lv ^ 1], dir_rows * sizeof(DfNode) + 16)) return rc;
            if (int rc = ensure(c, s->df_refs[lv ^ 1], dir_rows * sizeof(DfRef) + 16)) return rc;
            HIPCHK(c, hipMemsetAsync(s->df_rtab.p, 0xff, 4ull * rcap, c->stream));
            HIPCHK(c, hipMemsetAsync(&w.ctr[DF_C_NEXT], 0, 8, c->stream));
            hipLaunchKernelGGL(k_df_insert, df_grid(n_rows), dim3(256), 0, c->stream, w, P<uint32_t>(s->df_rtab), rcap);
            hipLaunchKernelGGL(k_df_compare, df_grid(n_rows), dim3(256), 0, c->stream, w, P<uint32_t>(s->df_rtab), rcap,
                               P<DfNode>(s->df_nodes[lv ^ 1]), P<DfRef>(s->df_refs[lv ^ 1]));
            hipLaunchKernelGGL(k_df_finish, df_grid(n_nodes), dim3(256), 0, c->stream, w);
        }
        HIPCHK(c, hipGetLastError());
        uint64_t ctr[DF_C_COUNT];
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
    HIPCHK(c, hipMemcpyAsync(&n_err, &w.ctr[DF_C_ERRORS], 8, hipMemcpyDeviceToHost, c->stream));
    if (n_e) HIPCHK(c, hipMemcpyAsync(read, s->df_read.p, n_e, hipMemcpyDeviceToHost, c->stream));
    if (rec_fit) HIPCHK(c, hipMemcpyAsync(records, s->df_rec.p, rec_fit * sizeof(bw_diff_record), hipMemcpyDeviceToHost, c->stream));
    if (names_fit) HIPCHK(c, hipMemcpyAsync(names, s->df_names.p, names_fit, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_err > err_ub) return df_refuse(c, "more errors than the kernels can have met");
    const uint64_t take_err = std::min(n_err, err_cap);
    if (take_err) HIPCHK(c, hipMemcpy(errs, s->df_err.p, take_err * sizeof(bw_prune_error), hipMemcpyDeviceToHost));
    counts->n_records = n_rec;
    counts->name_bytes = name_total;
    counts->n_levels = n_levels;
    counts->n_errors = n_err;
    for (uint64_t e = 0; e < n_e; e++) counts->n_read += read[e];
    if (full) {
        c->err = "diff: level " + std::to_string(n_levels - 1) + " does not fit record_cap or names_cap";
        return BW_ENOSPC;
    }
    if (n_err > err_cap) {
        c->err = "diff: " + std::to_string(n_err) + " errors do not fit err_cap";
        return BW_ENOSPC;
    }
    return BW_OK;
}
