// bw_find.hip -- find (include/backuwup_gpu_pack.h, "find"): which paths of which snapshots match a set
// of patterns.  The reference cannot ask it.  A fourth policy over the tree-chain fetch (bw_walk.h) beside
// the diff walk's, the parent match's and impact's report walk's, and one kernel of its own kind:
//   k_wk_resolve<FdFetch>, k_wk_take<FdFetch>  the first piece of every item of a level, for its header
//               and name only (the parent match's second fetch); then the whole chains of the Dir items
//               that are descended, and with BW_FIND_CHUNKS those of the File items that are hits
//   k_fd_match   a lane per (item, pattern): the item's name through the pattern's automaton from the
//               parent's carried state; the byte masks in LDS, the per-byte rule bw_find_host.h's fd_step
//   k_fd_decide  a lane per item: the pattern bits into HIT with the filters, PRUNED, what is fetched next
//   k_fd_rows    a lane per row of the level's lists: the next level's items
//   k_fd_chunks  a lane per chunk row of the hit files: into the caller's order
//   k_fd_records a lane per item: its record
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
#include "bw_find.h"

using namespace bw;

// ------------------------------------------------------------------ the fetch's policy
struct FdFetch {
    typedef FdWalk Walk;
    static constexpr const char* NAME = "find";
    static constexpr const char* ROWS_TOO_MANY = "a level of more than 2^30 children rows";
    static constexpr uint64_t MAX_ROWS = FD_MAX_ROWS;
    static constexpr uint64_t ERRS_PER_REF = 2;  // the ancestor check's, and the locate's

    // an item's first piece: is its hash one of its ancestors' on this path?  Then it is not descended.
    __device__ static bool first(const FdWalk& w, const WkRef& r) {
        uint64_t rec = w.items[r.owner].parent;
        for (uint64_t step = 0; rec != FD_NONE && step <= w.level; step++) {  // each step is one level up
            const bw_find_record& p = w.recs[rec];
            if (rs_eq(p.hash, r.hash, 32)) {
                wk_error(w.f, r.hash, r.by, r.by_pos, BW_RESTORE_EFORMAT);
                atomicOr(&w.items[r.owner].state, FD_CYCLIC);
                return true;
            }
            rec = p.parent;
        }
        return false;
    }

    __device__ static bool refuse(const FdWalk&, uint64_t) { return false; }

    __device__ static void lost(const FdWalk& w, uint32_t item) { atomicOr(&w.items[item].state, FD_TRUNC); }

    __device__ static void header(const FdWalk& w, uint32_t item, const RsTreeHdr& h, uint64_t name_off) {
        FdItem& it = w.items[item];
        atomicOr(&it.state, FD_OK);
        it.kind = h.kind;
        it.tflags = h.flags;
        it.size = h.size;
        it.mtime = h.mtime;
        it.ctime = h.ctime;
        it.name_off = name_off;
        it.name_len = h.name_len;
    }
};

// ------------------------------------------------------------------ the match
// Lane g of the grid-stride loop: item g / n_patterns, pattern g % n_patterns, so a wave reads few
// distinct names and the lanes of one item read neighbouring LDS words.  LDS: the byte masks,
// [byte][pattern], 2 KiB a pattern.  The state is one register pair; one pass over the name.
__global__ void __launch_bounds__(256) k_fd_match(FdWalk w) {
    extern __shared__ uint64_t lds_mask[];
    const uint32_t np = w.q.n_patterns;
    for (uint32_t i = threadIdx.x; i < 256 * np; i += 256) lds_mask[i] = w.masks[i];
    __syncthreads();
    const uint64_t n = w.n_items * np;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (uint64_t)gridDim.x * 256) {
        const uint64_t i = g / np;
        const uint32_t p = (uint32_t)(g % np);
        FdItem& it = w.items[i];
        uint64_t carried = 0;
        if (it.state & FD_OK) {
            const FdPat pat = w.pats[p];
            const uint64_t* mask = lds_mask + p;
            // other lanes OR into this item: what the loop needs of it is read once
            const uint64_t parent = it.parent, name_len = it.name_len;
            const uint8_t* name = w.f.names + it.name_off;
            const bool dir = it.kind == BW_TREE_DIR;
            uint64_t s;
            if (parent == FD_NONE) {
                s = pat.init;  // a root: its children start from the initial states, and it matches nothing
                carried = dir ? s : 0;
            } else {
                s = w.st_prev[(parent - w.rec0_prev) * np + p];
                for (uint64_t k = 0; k < name_len && s; k++) s = fd_step(mask, np, pat, s, name[k]);
                if (fd_accepts(pat, s) && (dir || !pat.dir_only)) atomicOr(&it.patterns, 1u << p);
                carried = dir ? fd_after_slash(mask, np, pat, s) : 0;
            }
            if (carried) atomicOr(&it.state, FD_ALIVE);
        }
        w.st_cur[g] = carried;
    }
}

// One lane per item, after k_fd_match.
__global__ void __launch_bounds__(256) k_fd_decide(FdWalk w, uint8_t* code) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w.n_items) return;
    FdItem& it = w.items[i];
    uint8_t x = FD_X_NONE;
    uint32_t fl = 0;
    if (it.state & FD_OK) {
        const FdQuery& q = w.q;
        const uint32_t pats = it.parent == FD_NONE ? 0 : (it.patterns | it.inherit);
        it.patterns = pats;
        const bool dir = it.kind == BW_TREE_DIR;
        bool hit = pats != 0 && (!q.kinds || (it.kind < 2 && ((q.kinds >> it.kind) & 1)));
        if (q.size_min != 0 || q.size_max != ~0ull)
            hit = hit && (it.tflags & BW_TREE_HAS_SIZE) && it.size >= q.size_min && it.size <= q.size_max;
        if (q.mtime_min != 0 || q.mtime_max != ~0ull)
            hit = hit && (it.tflags & BW_TREE_HAS_MTIME) && it.mtime >= q.mtime_min && it.mtime <= q.mtime_max;
        if (hit) fl |= BW_FIND_HIT;
        const bool hands_down = (q.flags & BW_FIND_SUBTREE) && pats != 0;
        if (dir && !(it.state & FD_CYCLIC)) {
            if (!(it.state & FD_ALIVE) && !hands_down) {
                fl |= BW_FIND_PRUNED;
                x = FD_X_PRUNED;
            } else {
                x = FD_X_DIR;
            }
        } else if (!dir && hit && (q.flags & BW_FIND_CHUNKS) && !(it.state & FD_CYCLIC)) {
            x = FD_X_CHUNKS;
        }
    } else {
        it.patterns = 0;
    }
    it.flags = fl;
    code[i] = x;
}

// One lane per chain that is fetched: its reference is the item's own, xmap[e] says which item.
__global__ void __launch_bounds__(256) k_fd_xrefs(const WkRef* refs, const uint32_t* xmap, uint64_t n, WkRef* out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) out[e] = refs[xmap[e]];
}

// One lane per row of the level's lists (the rows of the Dir items that are descended, item after item,
// each chain in chain order): row r is item r of the next level.
__global__ void __launch_bounds__(256) k_fd_rows(FdWalk w, const uint32_t* xmap, uint64_t n_rows, FdItem* next_items, WkRef* next_refs) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint64_t seg = wk_range_of(w.f.seg_row0, w.f.n_seg, r);  // no segment is empty
    const uint32_t item = xmap[w.f.seg_node[seg]];
    const uint8_t* row = wk_stage_row(w.f, seg, r);
    const FdItem& par = w.items[item];
    FdItem& x = next_items[r];
    memset(&x, 0, sizeof(x));
    wk_copy32(x.hash, row);
    x.parent = w.rec0 + item;
    x.root = par.root;
    x.inherit = (w.q.flags & BW_FIND_SUBTREE) ? par.patterns : 0;
    WkRef& f = next_refs[r];
    wk_copy32(f.hash, row);
    wk_copy32(f.by, w.f.seg_hash + 32ull * w.f.seg_sid[seg]);
    f.by_pos = r - w.f.seg_row0[seg];
    f.owner = (uint32_t)r;
    f.pad = 0;
}

// One lane per chunk row of the level's hit files, in the lists' order (file after file): 32 bytes.
__global__ void __launch_bounds__(256) k_fd_chunks(WkFetch f, uint64_t n_rows, uint8_t* out) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint64_t seg = wk_range_of(f.seg_row0, f.n_seg, r);
    wk_copy32(out + 32 * r, wk_stage_row(f, seg, r));
}

// One lane per item, last of its level: its record.  tab[2 * i], tab[2 * i + 1] = child_first, n_children.
__global__ void __launch_bounds__(256) k_fd_records(FdWalk w, const uint64_t* tab) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w.n_items) return;
    const FdItem& it = w.items[i];
    bw_find_record& r = w.recs[w.rec0 + i];
    memset(&r, 0, sizeof(r));
    wk_copy32(r.hash, it.hash);
    r.root = it.root;
    r.parent = it.parent;
    r.flags = ((it.state & FD_OK) ? it.flags : BW_FIND_UNREADABLE) | ((it.state & FD_TRUNC) ? BW_FIND_TRUNCATED : 0) |
              ((it.state & FD_CYCLIC) ? BW_FIND_CYCLIC : 0);
    if (!(it.state & FD_OK)) return;
    r.name_off = it.name_off;
    r.name_len = it.name_len;
    r.kind = it.kind;
    r.meta_flags = it.tflags;
    r.size = it.size;
    r.mtime = it.mtime;
    r.ctime = it.ctime;
    r.child_first = tab[2 * i];
    r.n_children = tab[2 * i + 1];
    r.patterns = it.patterns;
}

static int fd_refuse(bw_ctx* c, const char* why) { return wk_refuse(c, "find", why); }

// The level's lists after a rows fetch over n_x chains: the segment tables to `buf`, named in w.f.
static int fd_lists(WkHost<FdFetch>& H, std::vector<uint64_t>& lvl, DevBuf& buf) {
    bw_restore* s = H.s;
    bw_ctx* c = H.c;
    WkFetch& f = H.w.f;
    wk_level_tables(f, H.lv.segs, lvl, 0);
    if (int rc = ensure(c, buf, 8 * lvl.size() + 16)) return rc;
    HIPCHK(c, hipMemcpyAsync(buf.p, lvl.data(), 8 * lvl.size(), hipMemcpyHostToDevice, c->stream));
    wk_level_pointers(f, P<uint64_t>(buf), 0);
    f.stage = P<uint8_t>(s->wk[WK_B_STAGE]);
    f.seg_hash = P<uint8_t>(s->wk[WK_B_SEGHASH]);
    f.names = P<uint8_t>(s->wk[WK_B_NAMES]);
    return BW_OK;
}

extern "C" int bw_find_paths(bw_restore* s, const uint8_t* roots, uint64_t n_roots, const bw_find_query* query, uint32_t flags,
                             bw_find_record* records, uint64_t record_cap, uint8_t* names, uint64_t names_cap,
                             uint8_t* chunks, uint64_t chunks_cap, bw_find_root* per_root, bw_find_counts* counts,
                             bw_prune_error* errs, uint64_t err_cap) {
    const uint32_t known = BW_UNPACK_VERIFY | BW_FIND_ICASE | BW_FIND_SUBTREE | BW_FIND_CHUNKS;
    if (!s || !counts || !query || (flags & ~known) || (record_cap && !records) || (names_cap && !names) ||
        (chunks_cap && !chunks) || (err_cap && !errs) || (n_roots && (!roots || !per_root)))
        return BW_EINVAL;
    bw_ctx* c = s->c;
    hipSetDevice(c->device);
    const uint64_t n_e = s->entries.size();
    memset(counts, 0, sizeof(*counts));
    if (n_roots) memset(per_root, 0, n_roots * sizeof(bw_find_root));
    const uint32_t np = query->n_patterns;
    if (!np || np > BW_FIND_MAX_PATTERNS || !query->patterns || !query->pattern_off) {
        c->err = "find: between 1 and 32 patterns are taken";
        return BW_EINVAL;
    }
    if (query->kinds & ~((1u << BW_TREE_FILE) | (1u << BW_TREE_DIR))) {
        c->err = "find: kinds holds a bit that is neither File's nor Dir's";
        return BW_EINVAL;
    }
    // the patterns: compiled here, the byte masks side by side per byte for the kernel's LDS
    std::vector<uint64_t> hmask(256ull * np);
    std::vector<FdPat> hpat(np);
    {
        FdCompiled fc;
        std::string why;
        for (uint32_t p = 0; p < np; p++) {
            const uint64_t lo = query->pattern_off[p], hi = query->pattern_off[p + 1];
            if (hi < lo) {
                c->err = "find: pattern_off does not ascend";
                return BW_EINVAL;
            }
            if (fd_compile(query->patterns + lo, hi - lo, (flags & BW_FIND_ICASE) != 0, fc, why)) {
                c->err = "find: pattern " + std::to_string(p) + ": " + why;
                return BW_EINVAL;
            }
            hpat[p] = fc.p;
            for (uint32_t b = 0; b < 256; b++) hmask[(uint64_t)b * np + p] = fc.mask[b];
        }
    }
    if (!n_roots) return BW_OK;
    if (n_roots > FD_MAX_ROWS) return wk_too_large(c, FdFetch::NAME, "more than 2^30 roots");

    WkHost<FdFetch> H;
    if (int rc = wk_open(H, s, flags & BW_UNPACK_VERIFY)) return rc;
    FdWalk& w = H.w;
    const uint64_t pat_at = (8 * hmask.size() + 15) & ~15ull;
    if (int rc = ensure(c, s->fd[FD_B_PAT], pat_at + np * sizeof(FdPat) + 16)) return rc;
    HIPCHK(c, hipMemcpyAsync(s->fd[FD_B_PAT].p, hmask.data(), 8 * hmask.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(P<uint8_t>(s->fd[FD_B_PAT]) + pat_at, hpat.data(), np * sizeof(FdPat), hipMemcpyHostToDevice, c->stream));
    w.masks = P<uint64_t>(s->fd[FD_B_PAT]);
    w.pats = (const FdPat*)(P<uint8_t>(s->fd[FD_B_PAT]) + pat_at);
    w.q.n_patterns = np;
    w.q.kinds = query->kinds;
    w.q.flags = flags;
    w.q.size_min = query->size_min;
    w.q.size_max = query->size_max;
    w.q.mtime_min = query->mtime_min;
    w.q.mtime_max = query->mtime_max;

    // level 0: every root in root order
    int lv = 0;
    uint64_t n_items = n_roots;
    {
        std::vector<FdItem> hi(n_roots);
        std::vector<WkRef> hr(n_roots);
        memset(hi.data(), 0, n_roots * sizeof(FdItem));
        memset(hr.data(), 0, n_roots * sizeof(WkRef));
        for (uint64_t r = 0; r < n_roots; r++) {
            memcpy(hi[r].hash, roots + 32 * r, 32);
            hi[r].parent = FD_NONE;
            hi[r].root = (uint32_t)r;
            memcpy(hr[r].hash, roots + 32 * r, 32);
            hr[r].by_pos = r;
            hr[r].owner = (uint32_t)r;
        }
        if (int rc = ensure(c, s->fd[FD_B_ITEMS0], n_items * sizeof(FdItem) + 16)) return rc;
        if (int rc = ensure(c, s->fd[FD_B_REFS0], n_items * sizeof(WkRef) + 16)) return rc;
        HIPCHK(c, hipMemcpyAsync(s->fd[FD_B_ITEMS0].p, hi.data(), n_items * sizeof(FdItem), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(s->fd[FD_B_REFS0].p, hr.data(), n_items * sizeof(WkRef), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // hi, hr, hmask and hpat may leave scope
    }

    uint64_t n_rec = 0, n_levels = 0, n_chunks = 0, n_pruned = 0, rec0_prev = 0;
    uint64_t rec_fit = 0, names_fit = 0, chunks_fit = 0;  // the totals of the levels that fit the caller's arrays
    uint64_t& name_total = H.lv.name_total;  // the names of every level so far
    bool full = false;
    std::vector<uint64_t> lvl, tab;
    std::vector<uint8_t> code;
    std::vector<uint32_t> xdir, xfile;

    while (n_items) {
        // an item that is descended has a located hash no ancestor has: a path is no longer than the table
        if (n_levels > n_e + 1) return fd_refuse(c, "more levels than the store has entries");
        if (n_items > FD_MAX_ROWS) return wk_too_large(c, FdFetch::NAME, "a level of more than 2^30 items");
        w.level = n_levels++;
        w.items = P<FdItem>(s->fd[FD_B_ITEMS0 + lv]);
        w.n_items = n_items;
        w.rec0 = n_rec;
        w.rec0_prev = rec0_prev;
        const WkRef* d_refs = P<WkRef>(s->fd[FD_B_REFS0 + lv]);
        // the records so far are the ancestors the fetch's check walks; this level's follow them
        DevBuf& rec_buf = s->fd[FD_B_REC];
        if (int rc = wk_grow(c, FdFetch::NAME, rec_buf, (n_rec + n_items) * sizeof(bw_find_record) + 16, n_rec * sizeof(bw_find_record)))
            return rc;
        w.recs = P<bw_find_record>(rec_buf);

        // ---- read: every item's first piece, for its header and name
        if (int rc = wk_fetch(H, d_refs, n_items, true, false, (WkOwner*)nullptr)) return rc;
        w.f.names = P<uint8_t>(s->wk[WK_B_NAMES]);

        // ---- match, then decide: the host learns which chains to fetch
        if (int rc = ensure(c, s->fd[FD_B_ST0 + lv], 8 * n_items * np + 16)) return rc;
        if (int rc = ensure(c, s->fd[FD_B_CODE], n_items + 16)) return rc;
        w.st_prev = P<uint64_t>(s->fd[FD_B_ST0 + (lv ^ 1)]);
        w.st_cur = P<uint64_t>(s->fd[FD_B_ST0 + lv]);
        {
            const uint64_t pairs = n_items * np;
            const uint32_t blocks = (uint32_t)std::min<uint64_t>((pairs + 255) / 256, FD_MATCH_BLOCKS);
            hipLaunchKernelGGL(k_fd_match, dim3(blocks), dim3(256), 2048 * np, c->stream, w);
            hipLaunchKernelGGL(k_fd_decide, wk_grid(n_items), dim3(256), 0, c->stream, w, P<uint8_t>(s->fd[FD_B_CODE]));
            HIPCHK(c, hipGetLastError());
        }
        code.resize(n_items);
        HIPCHK(c, hipMemcpyAsync(code.data(), s->fd[FD_B_CODE].p, n_items, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        xdir.clear();
        xfile.clear();
        for (uint64_t i = 0; i < n_items; i++) {
            if (code[i] == FD_X_DIR) xdir.push_back((uint32_t)i);
            else if (code[i] == FD_X_CHUNKS) xfile.push_back((uint32_t)i);
            else if (code[i] == FD_X_PRUNED) n_pruned++;
            else if (code[i] != FD_X_NONE) return fd_refuse(c, "an item's code that cannot be");
        }
        tab.assign(2 * n_items, 0);
        if (int rc = ensure(c, s->fd[FD_B_XMAP], 4 * (xdir.size() + xfile.size()) + 16)) return rc;
        if (int rc = ensure(c, s->fd[FD_B_XREFS], std::max(xdir.size(), xfile.size()) * sizeof(WkRef) + 16)) return rc;
        uint32_t* d_xdir = P<uint32_t>(s->fd[FD_B_XMAP]);
        uint32_t* d_xfile = d_xdir + xdir.size();
        if (!xdir.empty()) HIPCHK(c, hipMemcpyAsync(d_xdir, xdir.data(), 4 * xdir.size(), hipMemcpyHostToDevice, c->stream));
        if (!xfile.empty()) HIPCHK(c, hipMemcpyAsync(d_xfile, xfile.data(), 4 * xfile.size(), hipMemcpyHostToDevice, c->stream));

        // ---- the rows of the Dir items that are descended: the next level's items, row after row
        uint64_t n_next = 0;
        if (!xdir.empty()) {
            const uint64_t n_x = xdir.size();
            hipLaunchKernelGGL(k_fd_xrefs, wk_grid(n_x), dim3(256), 0, c->stream, d_refs, d_xdir, n_x, P<WkRef>(s->fd[FD_B_XREFS]));
            HIPCHK(c, hipGetLastError());
            H.owners.assign(n_x, WkOwner());
            H.lv.segs.clear();
            H.lv.stage_rows = 0;
            if (int rc = wk_fetch(H, P<WkRef>(s->fd[FD_B_XREFS]), n_x, false, true, H.owners.data())) return rc;
            const uint64_t n_rows = H.lv.stage_rows;
            if (int rc = fd_lists(H, lvl, s->fd[FD_B_LVL])) return rc;
            uint64_t run = 0;
            for (uint64_t e = 0; e < n_x; e++) {
                tab[2 * xdir[e]] = H.owners[e].n_rows ? n_rec + n_items + run : 0;
                tab[2 * xdir[e] + 1] = H.owners[e].n_rows;
                run += H.owners[e].n_rows;
            }
            if (run != n_rows) return fd_refuse(c, "the level's rows do not add up");
            if (n_rows) {
                DevBuf &next_items = s->fd[FD_B_ITEMS0 + (lv ^ 1)], &next_refs = s->fd[FD_B_REFS0 + (lv ^ 1)];
                if (int rc = ensure(c, next_items, n_rows * sizeof(FdItem) + 16)) return rc;
                if (int rc = ensure(c, next_refs, n_rows * sizeof(WkRef) + 16)) return rc;
                hipLaunchKernelGGL(k_fd_rows, wk_grid(n_rows), dim3(256), 0, c->stream, w, d_xdir, n_rows, P<FdItem>(next_items),
                                   P<WkRef>(next_refs));
                HIPCHK(c, hipGetLastError());
            }
            n_next = n_rows;
            HIPCHK(c, hipStreamSynchronize(c->stream));  // lvl and the staging arena are reused below
        }

        // ---- the chunk rows of the File items that are hits, behind those of the levels before
        if (!xfile.empty()) {
            const uint64_t n_x = xfile.size();
            hipLaunchKernelGGL(k_fd_xrefs, wk_grid(n_x), dim3(256), 0, c->stream, d_refs, d_xfile, n_x, P<WkRef>(s->fd[FD_B_XREFS]));
            HIPCHK(c, hipGetLastError());
            H.owners.assign(n_x, WkOwner());
            H.lv.segs.clear();
            H.lv.stage_rows = 0;
            if (int rc = wk_fetch(H, P<WkRef>(s->fd[FD_B_XREFS]), n_x, false, true, H.owners.data())) return rc;
            const uint64_t n_rows = H.lv.stage_rows;
            if (int rc = fd_lists(H, lvl, s->fd[FD_B_LVL2])) return rc;
            uint64_t run = 0;
            for (uint64_t e = 0; e < n_x; e++) {
                tab[2 * xfile[e]] = n_chunks + run;
                tab[2 * xfile[e] + 1] = H.owners[e].n_rows;
                run += H.owners[e].n_rows;
            }
            if (run != n_rows) return fd_refuse(c, "the level's chunk rows do not add up");
            if (int rc = wk_grow(c, FdFetch::NAME, s->fd[FD_B_CHUNKS], 32 * (n_chunks + n_rows) + 32, 32 * n_chunks)) return rc;
            if (n_rows) {
                hipLaunchKernelGGL(k_fd_chunks, wk_grid(n_rows), dim3(256), 0, c->stream, w.f, n_rows,
                                   P<uint8_t>(s->fd[FD_B_CHUNKS]) + 32 * n_chunks);
                HIPCHK(c, hipGetLastError());
            }
            n_chunks += n_rows;
        }

        // ---- the records
        if (int rc = ensure(c, s->fd[FD_B_TAB], 8 * tab.size() + 16)) return rc;
        HIPCHK(c, hipMemcpyAsync(s->fd[FD_B_TAB].p, tab.data(), 8 * tab.size(), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_fd_records, wk_grid(n_items), dim3(256), 0, c->stream, w, P<uint64_t>(s->fd[FD_B_TAB]));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        rec0_prev = n_rec;
        n_rec += n_items;
        if (n_rec > record_cap || name_total > names_cap || ((flags & BW_FIND_CHUNKS) && n_chunks > chunks_cap)) {
            full = true;
            break;
        }
        rec_fit = n_rec;
        names_fit = name_total;
        chunks_fit = n_chunks;
        n_items = n_next;
        lv ^= 1;
    }

    // ---- results
    uint64_t n_err = 0;
    HIPCHK(c, hipMemcpyAsync(&n_err, w.f.n_err, 8, hipMemcpyDeviceToHost, c->stream));
    if (rec_fit) HIPCHK(c, hipMemcpyAsync(records, s->fd[FD_B_REC].p, rec_fit * sizeof(bw_find_record), hipMemcpyDeviceToHost, c->stream));
    if (names_fit) HIPCHK(c, hipMemcpyAsync(names, s->wk[WK_B_NAMES].p, names_fit, hipMemcpyDeviceToHost, c->stream));
    if (chunks_fit) HIPCHK(c, hipMemcpyAsync(chunks, s->fd[FD_B_CHUNKS].p, 32 * chunks_fit, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int rc = wk_errors_out(H, n_err, errs, err_cap);
    if (rc != BW_OK && rc != BW_ENOSPC) return rc;
    for (uint64_t i = 0; i < rec_fit; i++) {  // the per-root summary of the records returned
        const bw_find_record& r = records[i];
        if (r.root >= n_roots) return fd_refuse(c, "a record under a root that was not given");
        bw_find_root& pr = per_root[r.root];
        pr.n_records++;
        if (r.flags & BW_FIND_UNREADABLE) pr.n_unreadable++;
        if (r.flags & BW_FIND_HIT) {
            pr.n_hits++;
            if (r.kind == BW_TREE_FILE) {
                pr.n_hit_files++;
                pr.hit_bytes += r.size;
            }
        }
    }
    counts->n_records = n_rec;
    counts->name_bytes = name_total;
    counts->n_chunks = n_chunks;
    counts->n_levels = n_levels;
    counts->n_opened = H.n_opened;
    counts->n_pruned = n_pruned;
    counts->n_errors = n_err;
    if (full) {
        c->err = "find: level " + std::to_string(n_levels - 1) + " does not fit record_cap, names_cap or chunks_cap";
        return BW_ENOSPC;
    }
    return rc;
}
