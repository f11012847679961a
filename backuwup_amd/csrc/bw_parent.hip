// bw_parent.hip -- the parent match (include/backuwup_gpu_pack.h, "parent match"): which files of a new
// backup are the parent snapshot's as they stand, by name, size and mtime, so that they need not be
// read.  The reference has no such step: it maps and chunks every file on every run
// (dir_packer.rs:231-282) and lets dedup discard the result; this goes past it, like prune, check,
// rekey, parity and diff.  The walk is level-synchronous and host-driven like the diff walk: the host
// counts, lays a level's arenas out by prefix sums over the parsed headers and feeds the unpack chain
// `slots` blobs at a time; every comparison of hash bytes and name bytes, the verdict and the sums are
// a kernel's.  Per level:
//   wk_fetch      twice (bw_walk.h, shared with the diff walk): the items' chains, rows only, then the
//                 parent children's first pieces, header and name only (k_wk_resolve / k_wk_take<PmFetch>)
//   k_pm_rows    the chains' rows gathered into one list per item: the level's parent children
//   k_pm_build    the (item, name) table over the readable children, the lowest position winning
//   k_pm_probe    every scan child of an item's Dir against the table
//   k_pm_verdict  the status and hash of each, n_unchanged and unchanged_bytes, the next level's items
// An item's first piece is read once as its parent's child (for the name) and once more as the head of
// its chain (for the rows): Dirs are few beside files, and the level then needs no second staging.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/backuwup_gpu.h"
#include "bw_device.h"
#include "bw_internal.h"
#include "bw_ctx.h"
#include "bw_restore.h"
#include "bw_parent.h"

using namespace bw;

// ------------------------------------------------------------------ the fetch's policy
// What the shared fetch (bw_walk.h) leaves to the walk.  A chain's owner is an item of the level; the
// owner of a header is a parent child.  A chain that loses a later piece just ends there.
struct PmFetch {
    typedef PmWalk Walk;
    static constexpr const char* NAME = "parent match";
    static constexpr const char* ROWS_TOO_MANY = "more than 2^30 children rows in a level";
    static constexpr uint64_t MAX_ROWS = PM_MAX_ROWS;
    static constexpr uint64_t ERRS_PER_REF = 1;

    __device__ static bool first(const PmWalk&, const WkRef&) { return false; }
    __device__ static bool refuse(const PmWalk&, uint64_t) { return false; }  // every located piece is opened

    __device__ static void lost(const PmWalk&, uint32_t) {}

    __device__ static void header(const PmWalk& w, uint32_t child, const RsTreeHdr& h, uint64_t name_off) {
        PmChild& c = w.child[child];
        c.ok = 1;
        c.kind = h.kind;
        c.tflags = h.flags;
        c.size = h.size;
        c.mtime = h.mtime;
        c.ctime = h.ctime;
        c.name_off = name_off;
        c.name_len = h.name_len;
    }
};

// ------------------------------------------------------------------ the level's parent children
// One lane per row of the level's lists: the child it is, and the reference to its first piece.
__global__ void __launch_bounds__(256) k_pm_rows(PmWalk w, WkRef* crefs) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= w.n_child) return;
    const uint64_t seg = wk_range_of(w.f.seg_row0, w.f.n_seg, r);  // no segment is empty
    const uint8_t* row = wk_stage_row(w.f, seg, r);
    const uint32_t item = w.f.seg_node[seg];
    PmChild& c = w.child[r];
    memset(&c, 0, sizeof(c));
    wk_copy32(c.hash, row);
    c.item = item;
    c.pos = r - w.node_row0[item];
    WkRef& f = crefs[r];
    wk_copy32(f.hash, row);
    wk_copy32(f.by, w.f.seg_hash + 32ull * w.f.seg_sid[seg]);
    f.by_pos = r - w.f.seg_row0[seg];
    f.owner = (uint32_t)r;
    f.pad = 0;
}

// ------------------------------------------------------------------ the (item, name) join
// The key: (item, name bytes), compared whole.  On level 0 the roots pair whatever their names.
__device__ static inline uint32_t pm_key_hash(uint32_t item, const uint8_t* p, uint64_t len) {
    return wk_key_hash(item * 0x9e3779b97f4a7c15ull, p, len);
}

// One lane per parent child.  tab[slot] = some readable child of the key, best[slot] = the lowest
// (position, child) of it: the one that answers for its name.  The table holds twice the children, and
// a probe ends at cap.
__global__ void __launch_bounds__(256) k_pm_build(PmWalk w, uint32_t* tab, uint64_t* best, uint32_t cap) {
    const uint64_t n = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= w.n_child) return;
    const PmChild& c = w.child[n];
    if (!c.ok) return;
    const uint64_t len = w.root ? 0 : c.name_len;
    const uint8_t* name = w.f.names + c.name_off;
    const uint32_t h = pm_key_hash(c.item, name, len);
    for (uint32_t probe = 0; probe < cap; probe++) {
        const uint32_t slot = (h + probe) & (cap - 1);
        const uint32_t cur = atomicCAS(&tab[slot], RS_EMPTY, (uint32_t)n);
        bool same = cur == RS_EMPTY;
        if (!same) {
            const PmChild& o = w.child[cur];  // cur was ok when it was put there, and its name is in place
            same = o.item == c.item && wk_name_eq(w.f.names + o.name_off, w.root ? 0 : o.name_len, name, len);
        }
        if (same) {
            atomicMin((unsigned long long*)&best[slot], (unsigned long long)((c.pos << 32) | n));
            return;
        }
    }
}

// One lane per probe: scan child k of item i's Dir.  match[2 p] = the parent child that answers for
// its name (or RS_EMPTY), match[2 p + 1] = the scan node.
__global__ void __launch_bounds__(256) k_pm_probe(PmWalk w, const uint32_t* tab, const uint64_t* best, uint32_t cap,
                                                  uint32_t* match) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= w.n_probes) return;
    const uint64_t item = wk_range_of(w.probe_row0, w.n_items, p);
    const uint64_t node = w.item_first[item] + (p - w.probe_row0[item]);
    const bw_restore_node& sn = w.scan[node];
    const uint64_t len = w.root ? 0 : sn.name_len;
    const uint8_t* name = w.scan_names + sn.name_off;
    const uint32_t h = pm_key_hash((uint32_t)item, name, len);
    uint32_t found = RS_EMPTY;
    for (uint32_t probe = 0; probe < cap; probe++) {
        const uint32_t slot = (h + probe) & (cap - 1);
        const uint32_t cur = tab[slot];
        if (cur == RS_EMPTY) break;
        const PmChild& o = w.child[cur];
        if (o.item == (uint32_t)item && wk_name_eq(w.f.names + o.name_off, w.root ? 0 : o.name_len, name, len)) {
            found = (uint32_t)best[slot];
            break;
        }
    }
    match[2 * p] = found;
    match[2 * p + 1] = (uint32_t)node;
}

// One lane per probe, after k_pm_probe: the status and the hash of its scan node, the wave's share of
// n_unchanged and unchanged_bytes, and the next level's items (one place per Dir against Dir pair).
__global__ void __launch_bounds__(256) k_pm_verdict(PmWalk w, const uint32_t* match, PmItem* next) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = p < w.n_probes;
    uint32_t status = BW_PARENT_NEW, child = RS_EMPTY, node = 0;
    uint64_t bytes = 0;
    if (active) {
        child = match[2 * p];
        node = match[2 * p + 1];
    }
    if (child != RS_EMPTY) {
        const bw_restore_node& sn = w.scan[node];
        const PmChild& c = w.child[child];
        if (sn.kind != c.kind) {
            status = BW_PARENT_TYPE_CHANGED;
        } else if (sn.kind == BW_TREE_DIR) {
            status = BW_PARENT_DIR;
        } else {
            const uint32_t need = BW_TREE_HAS_SIZE | BW_TREE_HAS_MTIME;
            bool same = sn.flags == c.tflags && (sn.flags & need) == need && sn.size == c.size && sn.mtime == c.mtime;
            if (same && (sn.flags & BW_TREE_HAS_CTIME)) same = sn.ctime == c.ctime;
            status = !same ? BW_PARENT_CHANGED : (sn.mtime < w.trust_before ? BW_PARENT_UNCHANGED : BW_PARENT_RACY);
            if (status == BW_PARENT_UNCHANGED) bytes = sn.size;
        }
        bw_parent_result& out = w.res[node];  // scan nodes of one probe list are distinct: one writer each
        wk_copy32(out.hash, c.hash);
        out.status = status;
        out.pad = 0;
    }
    // the sums: the wave's files by the ballot, its bytes by a butterfly over the two halves
    const uint64_t unch = __ballot(status == BW_PARENT_UNCHANGED);
    if (unch) {
        uint32_t lo = (uint32_t)bytes, hi = (uint32_t)(bytes >> 32);
        uint64_t sum = bytes;
        for (int d = 32; d; d >>= 1) {
            const uint64_t o = ((uint64_t)__shfl_xor(hi, d) << 32) | __shfl_xor(lo, d);
            sum += o;
            lo = (uint32_t)sum;
            hi = (uint32_t)(sum >> 32);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd((unsigned long long*)&w.ctr[PM_C_UNCHANGED], (unsigned long long)__popcll(unch));
            atomicAdd((unsigned long long*)&w.ctr[PM_C_BYTES], (unsigned long long)sum);
        }
    }
    const bool push = status == BW_PARENT_DIR;
    const uint64_t j = wk_wave_place(push, &w.ctr[PM_C_NEXT]);
    if (!push) return;  // at most one place per probe: the list holds that many
    PmItem& x = next[j];
    wk_copy32(x.hash, w.child[child].hash);
    x.scan = node;
    x.pad = 0;
}

// ------------------------------------------------------------------ the host's side
static int pm_refuse(bw_ctx* c, const char* why) { return wk_refuse(c, PmFetch::NAME, why); }

extern "C" int bw_parent_match(bw_restore* s, const uint8_t* parent_root, uint64_t trust_before, uint32_t flags,
                               const bw_restore_node* nodes, uint64_t n_nodes, const uint8_t* names, uint64_t names_len,
                               bw_parent_result* results, uint8_t* read, bw_parent_counts* counts, bw_prune_error* errs,
                               uint64_t err_cap) {
    if (!s || !counts || (flags & ~BW_UNPACK_VERIFY) || !nodes || !n_nodes || !results || (names_len && !names) ||
        (err_cap && !errs) || (!s->entries.empty() && !read))
        return BW_EINVAL;
    bw_ctx* c = s->c;
    const uint64_t n_e = s->entries.size();
    memset(counts, 0, sizeof(*counts));
    if (n_e) memset(read, 0, n_e);
    if (n_nodes > PM_MAX_ROWS) return wk_too_large(c, PmFetch::NAME, "more than 2^30 scan nodes");
    if (const uint64_t bad = pm_scan_invalid(nodes, n_nodes, names_len)) {
        c->err = "parent match: scan node " + std::to_string(bad - 1) + " breaks the scan's rules";
        return BW_EINVAL;
    }
    memset(results, 0, n_nodes * sizeof(*results));  // BW_PARENT_NEW, no hash
    if (!parent_root) return BW_OK;
    hipSetDevice(c->device);

    WkHost<PmFetch> H;
    if (int rc = wk_open(H, s, flags)) return rc;
    PmWalk& w = H.w;
    w.trust_before = trust_before;
    if (int rc = ensure(c, s->pm[PM_B_SCAN], n_nodes * sizeof(bw_restore_node) + 16)) return rc;
    if (int rc = ensure(c, s->pm[PM_B_SNAMES], names_len + 16)) return rc;
    if (int rc = ensure(c, s->pm[PM_B_RES], n_nodes * sizeof(bw_parent_result) + 16)) return rc;
    HIPCHK(c, hipMemsetAsync(s->pm[PM_B_RES].p, 0, n_nodes * sizeof(bw_parent_result), c->stream));
    HIPCHK(c, hipMemcpyAsync(s->pm[PM_B_SCAN].p, nodes, n_nodes * sizeof(bw_restore_node), hipMemcpyHostToDevice, c->stream));
    if (names_len) HIPCHK(c, hipMemcpyAsync(s->pm[PM_B_SNAMES].p, names, names_len, hipMemcpyHostToDevice, c->stream));
    w.ctr = P<uint64_t>(s->wk[WK_B_CTR]);
    w.scan = P<bw_restore_node>(s->pm[PM_B_SCAN]);
    w.scan_names = P<uint8_t>(s->pm[PM_B_SNAMES]);
    w.res = P<bw_parent_result>(s->pm[PM_B_RES]);

    // Level 0 has one item that is no Dir pair yet: its one "scan child" is node 0 and its one "parent
    // child" is parent_root, and their names are not compared.  From level 1 on the items are the
    // Dir against Dir pairs of the level before.
    // n_levels counts the levels that hold an item, and level 0 holds the root item whatever becomes of it.
    uint64_t n_items = 1, n_levels = 0;
    std::vector<uint32_t> item_scan;  // per item: its scan Dir
    std::vector<uint64_t> lvl;
    std::vector<PmItem> h_items;
    bool root = true;
    while (n_items) {
        if (n_levels > n_nodes) return pm_refuse(c, "more levels than the scan has nodes");
        if (!root) n_levels++;
        H.lv = WkLevel();
        H.owners.assign(n_items, WkOwner());
        w.root = root;
        w.n_items = n_items;
        uint64_t n_child = 1;

        // ---- the items' chains: every row of every piece (bw_walk.h)
        if (!root) {
            if (int rc = ensure(c, s->pm[PM_B_REFS], n_items * sizeof(WkRef) + 16)) return rc;
            // the items' first pieces as references: read a second time, as the heads of their chains
            std::vector<WkRef> hr(n_items);
            memset(hr.data(), 0, n_items * sizeof(WkRef));
            for (uint64_t i = 0; i < n_items; i++) {
                memcpy(hr[i].hash, h_items[i].hash, 32);
                memcpy(hr[i].by, h_items[i].hash, 32);  // an error of this read names the piece itself
                hr[i].by_pos = WK_NONE;
                hr[i].owner = (uint32_t)i;
            }
            HIPCHK(c, hipMemcpyAsync(s->pm[PM_B_REFS].p, hr.data(), n_items * sizeof(WkRef), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));  // hr leaves scope
            if (int rc = wk_fetch(H, P<WkRef>(s->pm[PM_B_REFS]), n_items, false, true, H.owners.data())) return rc;
            n_child = H.lv.stage_rows;
        }

        // ---- the level's layout; the walk's own tables between the segments':
        //      [node_row0 | probe_row0 (n_items + 1) | item_first]
        const uint64_t n_own = 3 * n_items + 1;
        if (wk_level_tables(w.f, H.lv.segs, lvl, n_own) != n_child && !root) return pm_refuse(c, "the level's rows do not add up");
        const uint64_t n_seg = w.f.n_seg;
        uint64_t* node_row0 = lvl.data() + 2 * n_seg + 1;
        uint64_t* probe_row0 = node_row0 + n_items;
        uint64_t* item_first = probe_row0 + n_items + 1;
        uint64_t run = 0, n_probes = 0;
        for (uint64_t i = 0; i < n_items; i++) {
            node_row0[i] = run;
            run += H.owners[i].n_rows;
            probe_row0[i] = n_probes;
            if (root) {
                item_first[i] = 0;
                n_probes += 1;
            } else {
                const bw_restore_node& sn = nodes[item_scan[i]];
                item_first[i] = sn.child_first;
                n_probes += sn.n_children;
            }
        }
        probe_row0[n_items] = n_probes;
        if (int rc = ensure(c, s->pm[PM_B_LVL], 8 * lvl.size() + 16)) return rc;
        if (int rc = ensure(c, s->pm[PM_B_CHILD], n_child * sizeof(PmChild) + 16)) return rc;
        if (int rc = ensure(c, s->pm[PM_B_CREFS], n_child * sizeof(WkRef) + 16)) return rc;
        HIPCHK(c, hipMemcpyAsync(s->pm[PM_B_LVL].p, lvl.data(), 8 * lvl.size(), hipMemcpyHostToDevice, c->stream));
        wk_level_pointers(w.f, P<uint64_t>(s->pm[PM_B_LVL]), n_own);
        w.node_row0 = w.f.seg_stage + n_seg;
        w.probe_row0 = w.node_row0 + n_items;
        w.item_first = w.probe_row0 + n_items + 1;
        w.child = P<PmChild>(s->pm[PM_B_CHILD]);
        w.n_child = n_child;
        w.n_probes = n_probes;
        w.f.stage = P<uint8_t>(s->wk[WK_B_STAGE]);
        w.f.seg_hash = P<uint8_t>(s->wk[WK_B_SEGHASH]);

        // ---- the parent children and their first pieces
        if (root) {
            PmChild hc;
            WkRef hr;
            memset(&hc, 0, sizeof(hc));
            memset(&hr, 0, sizeof(hr));
            memcpy(hc.hash, parent_root, 32);
            memcpy(hr.hash, parent_root, 32);
            HIPCHK(c, hipMemcpyAsync(s->pm[PM_B_CHILD].p, &hc, sizeof(hc), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(s->pm[PM_B_CREFS].p, &hr, sizeof(hr), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));  // hc and hr leave scope
        } else if (n_child) {
            hipLaunchKernelGGL(k_pm_rows, wk_grid(n_child), dim3(256), 0, c->stream, w, P<WkRef>(s->pm[PM_B_CREFS]));
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));  // lvl is rewritten by the next level
        if (n_child)
            if (int rc = wk_fetch(H, P<WkRef>(s->pm[PM_B_CREFS]), n_child, true, false, nullptr)) return rc;
        w.f.names = P<uint8_t>(s->wk[WK_B_NAMES]);

        // ---- the join, the verdict and the next level's items: a probe gives one item at most
        uint64_t n_next = 0;
        if (n_probes) {
            const uint32_t cap = pm_table_cap(n_child);
            if (int rc = ensure(c, s->pm[PM_B_TAB], 12ull * cap + 16)) return rc;
            if (int rc = ensure(c, s->pm[PM_B_MATCH], 8 * n_probes + 16)) return rc;
            DevBuf& next_buf = s->pm[PM_B_ITEMS];
            if (int rc = ensure(c, next_buf, n_probes * sizeof(PmItem) + 16)) return rc;
            uint64_t* d_best = P<uint64_t>(s->pm[PM_B_TAB]);
            uint32_t* d_tab = (uint32_t*)(d_best + cap);
            HIPCHK(c, hipMemsetAsync(s->pm[PM_B_TAB].p, 0xff, 12ull * cap, c->stream));
            HIPCHK(c, hipMemsetAsync(&w.ctr[PM_C_NEXT], 0, 8, c->stream));
            if (n_child) hipLaunchKernelGGL(k_pm_build, wk_grid(n_child), dim3(256), 0, c->stream, w, d_tab, d_best, cap);
            hipLaunchKernelGGL(k_pm_probe, wk_grid(n_probes), dim3(256), 0, c->stream, w, d_tab, d_best, cap,
                               P<uint32_t>(s->pm[PM_B_MATCH]));
            hipLaunchKernelGGL(k_pm_verdict, wk_grid(n_probes), dim3(256), 0, c->stream, w, P<uint32_t>(s->pm[PM_B_MATCH]),
                               P<PmItem>(next_buf));
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&n_next, &w.ctr[PM_C_NEXT], 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (n_next > n_probes) return pm_refuse(c, "a level's item count that cannot be");
            h_items.resize(n_next);
            if (n_next) HIPCHK(c, hipMemcpy(h_items.data(), next_buf.p, n_next * sizeof(PmItem), hipMemcpyDeviceToHost));
            item_scan.resize(n_next);
            for (uint64_t i = 0; i < n_next; i++) {
                const uint32_t sn = h_items[i].scan;
                if (sn >= n_nodes || nodes[sn].kind != BW_TREE_DIR) return pm_refuse(c, "an item that is no scan Dir");
                item_scan[i] = sn;
            }
        }
        n_items = n_next;
        root = false;
    }

    // ---- results
    uint64_t ctr[WK_C_COUNT];
    HIPCHK(c, hipMemcpyAsync(ctr, w.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
    if (n_e) HIPCHK(c, hipMemcpyAsync(read, w.f.read, n_e, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(results, s->pm[PM_B_RES].p, n_nodes * sizeof(bw_parent_result), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t n_err = ctr[WK_C_ERRORS];
    const int rc = wk_errors_out(H, n_err, errs, err_cap);
    if (rc != BW_OK && rc != BW_ENOSPC) return rc;
    counts->n_levels = n_levels ? n_levels : 1;
    counts->n_errors = n_err;
    counts->n_unchanged = ctr[PM_C_UNCHANGED];
    counts->unchanged_bytes = ctr[PM_C_BYTES];
    for (uint64_t e = 0; e < n_e; e++) counts->n_read += read[e];
    return rc;
}
