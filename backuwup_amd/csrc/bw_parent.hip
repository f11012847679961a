// bw_parent.hip -- the parent match (include/backuwup_gpu_pack.h, "parent match"): which files of a new
// backup are the parent snapshot's as they stand, by name, size and mtime, so that they need not be
// read.  The reference has no such step: it maps and chunks every file on every run
// (dir_packer.rs:231-282) and lets dedup discard the result; this goes past it, like prune, check,
// rekey, parity and diff.  The walk is level-synchronous and host-driven like the diff walk: the host
// counts, lays a level's arenas out by prefix sums over the parsed headers and feeds the unpack chain
// `slots` blobs at a time; every comparison of hash bytes and name bytes, the verdict and the sums are
// a kernel's.  Per level:
//   k_pm_resolve  one lane per reference: locate, kind, read[]
//   k_pm_take     one workgroup per decoded blob: a chain piece's rows, or a child's header and name
//   k_pm_rows     the chains' rows gathered into one list per item: the level's parent children
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

// ------------------------------------------------------------------ device helpers
__device__ static void pm_error(const PmWalk& w, const uint8_t* hash, const uint8_t* by, uint64_t pos, uint32_t reason) {
    const uint64_t at = atomicAdd((unsigned long long*)&w.ctr[PM_C_ERRORS], 1ull);
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

__device__ static inline void pm_copy32(uint8_t* d, const uint8_t* s) {
    for (int i = 0; i < 32; i++) d[i] = s[i];
}

// Every lane of the wave calls this: the lanes with push = true get consecutive places from *ctr (one
// atomic by the first of them, each lane's place from the ballot).
__device__ static inline uint64_t pm_wave_place(bool push, uint64_t* ctr) {
    const uint64_t bal = __ballot(push);
    if (!bal) return 0;
    const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__ffsll((unsigned long long)bal) - 1;
    uint64_t base = 0;
    if (lane == leader) base = atomicAdd((unsigned long long*)ctr, (unsigned long long)__popcll(bal));
    const uint32_t lo = __shfl((uint32_t)base, leader), hi = __shfl((uint32_t)(base >> 32), leader);
    return (((uint64_t)hi << 32) | lo) + __popcll(bal & ((1ull << lane) - 1));
}

// the largest i < n with row0[i] <= r (row0 ascends; equal entries are empty ranges and are passed over)
__device__ static inline uint64_t pm_range_of(const uint64_t* row0, uint64_t n, uint64_t r) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (row0[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------ resolve
// out[i] = the entry the reference names, or RS_EMPTY when there is none to open.  overlong: the chain
// has more pieces than the store has entries, so every reference of the round is refused unread.
__global__ void __launch_bounds__(256) k_pm_resolve(PmWalk w, const PmRef* refs, uint64_t n, int overlong, uint32_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PmRef& r = refs[i];
    uint32_t res = RS_EMPTY;
    if (overlong) {
        pm_error(w, r.hash, r.by, r.by_pos, BW_RESTORE_EFORMAT);
        out[i] = res;
        return;
    }
    uint64_t e;
    const uint8_t st = rs_locate_one(w.loc, r.hash, e);
    if (st) {
        pm_error(w, r.hash, r.by, r.by_pos, st);
    } else if (w.loc.entries[e].kind != BW_BLOB_TREE) {
        pm_error(w, r.hash, r.by, r.by_pos, BW_RESTORE_ENOTTREE);
    } else {
        w.read[e] = 1;
        res = (uint32_t)e;
    }
    out[i] = res;
}

// ------------------------------------------------------------------ take
// Workgroup b: blob b of the sub-batch, decoded at slots + off[b] and parsed into hdr[b].  A blob the
// chain or the parser refused is an error of its reference.  A good chain piece gives its rows to the
// staging arena and its next_sibling to the next round; a good first piece of a child (children = 1)
// gives the child its header and its name, and nothing of its rows or its chain is looked at.
__global__ void __launch_bounds__(256) k_pm_take(PmWalk w, const PmRef* refs, const PmTake* tab, const uint8_t* slots,
                                                 const uint64_t* off, const RsTreeHdr* hdr, uint64_t m, int children,
                                                 PmRef* next) {
    const uint64_t b = blockIdx.x;
    if (b >= m) return;
    const PmTake t = tab[b];
    const PmRef& r = refs[t.ref];
    const RsTreeHdr& h = hdr[b];
    const uint32_t bad = t.cst ? t.cst : h.status;
    if (bad) {
        if (threadIdx.x == 0) pm_error(w, r.hash, r.by, r.by_pos, bad);
        return;
    }
    const uint8_t* blob = slots + off[b];
    if (children) {
        if (threadIdx.x == 0) {
            PmChild& c = w.child[r.owner];
            c.ok = 1;
            c.kind = h.kind;
            c.tflags = h.flags;
            c.size = h.size;
            c.mtime = h.mtime;
            c.ctime = h.ctime;
            c.name_off = t.name_off;
            c.name_len = h.name_len;
        }
        // the parser bounded the name by the blob; the host gave it h.name_len bytes of the arena
        for (uint64_t i = threadIdx.x; i < h.name_len; i += 256) w.names[t.name_off + i] = blob[h.name_pos + i];
        return;
    }
    if (threadIdx.x == 0) {
        if (t.seg != PM_NONE) pm_copy32(w.seg_hash + 32 * t.seg, r.hash);
        if (t.next != PM_NONE) {
            PmRef& x = next[t.next];
            pm_copy32(x.hash, h.next);
            pm_copy32(x.by, r.hash);
            x.by_pos = PM_NONE;
            x.owner = r.owner;
            x.pad = 0;
        }
    }
    // the rows: each wave takes pieces of RS_PIECE bytes and copies them in 16-byte vectors (the strict
    // form: ch_pos lies at any byte, and nothing outside the rows is loaded); t.n_rows == h.n_children,
    // which the parser bounded by the blob
    const uint8_t* src = blob + h.ch_pos;
    uint8_t* dst = w.stage + 32 * t.stage;
    const uint64_t nb = 32 * t.n_rows;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t p0 = (uint64_t)(threadIdx.x >> 6) * RS_PIECE; p0 < nb; p0 += 4ull * RS_PIECE)
        rs_copy_piece<true>(src + p0, dst + p0, nb - p0 < RS_PIECE ? nb - p0 : RS_PIECE, lane);
}

// ------------------------------------------------------------------ the level's parent children
// One lane per row of the level's lists: the child it is, and the reference to its first piece.
__global__ void __launch_bounds__(256) k_pm_rows(PmWalk w, PmRef* crefs) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= w.n_child) return;
    const uint64_t seg = pm_range_of(w.seg_row0, w.n_seg, r);  // no segment is empty
    const uint8_t* row = w.stage + 32 * (w.seg_stage[seg] + (r - w.seg_row0[seg]));
    const uint32_t item = w.seg_node[seg];
    PmChild& c = w.child[r];
    memset(&c, 0, sizeof(c));
    pm_copy32(c.hash, row);
    c.item = item;
    c.pos = r - w.node_row0[item];
    PmRef& f = crefs[r];
    pm_copy32(f.hash, row);
    pm_copy32(f.by, w.seg_hash + 32ull * w.seg_sid[seg]);
    f.by_pos = r - w.seg_row0[seg];
    f.owner = (uint32_t)r;
    f.pad = 0;
}

// ------------------------------------------------------------------ the (item, name) join
// The key: (item, name bytes), compared whole.  On level 0 the roots pair whatever their names.
__device__ static inline uint32_t pm_key_hash(uint32_t item, const uint8_t* p, uint64_t len) {
    uint64_t h = 0xcbf29ce484222325ull ^ (item * 0x9e3779b97f4a7c15ull);
    for (uint64_t i = 0; i < len; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return rs_mix(h);
}

__device__ static inline bool pm_name_eq(const uint8_t* x, uint64_t nx, const uint8_t* y, uint64_t ny) {
    if (nx != ny) return false;
    uint32_t d = 0;
    for (uint64_t i = 0; i < nx; i++) d |= x[i] ^ y[i];
    return d == 0;
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
    const uint8_t* name = w.names + c.name_off;
    const uint32_t h = pm_key_hash(c.item, name, len);
    for (uint32_t probe = 0; probe < cap; probe++) {
        const uint32_t slot = (h + probe) & (cap - 1);
        const uint32_t cur = atomicCAS(&tab[slot], RS_EMPTY, (uint32_t)n);
        bool same = cur == RS_EMPTY;
        if (!same) {
            const PmChild& o = w.child[cur];  // cur was ok when it was put there, and its name is in place
            same = o.item == c.item && pm_name_eq(w.names + o.name_off, w.root ? 0 : o.name_len, name, len);
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
    const uint64_t item = pm_range_of(w.probe_row0, w.n_items, p);
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
        if (o.item == (uint32_t)item && pm_name_eq(w.names + o.name_off, w.root ? 0 : o.name_len, name, len)) {
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
        pm_copy32(out.hash, c.hash);
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
    const uint64_t j = pm_wave_place(push, &w.ctr[PM_C_NEXT]);
    if (!push) return;  // at most one place per probe: the list holds that many
    PmItem& x = next[j];
    pm_copy32(x.hash, w.child[child].hash);
    x.scan = node;
    x.pad = 0;
}

// ------------------------------------------------------------------ the host's side
static inline dim3 pm_grid(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

// a buffer of at least `need` bytes that keeps its first `keep` bytes
static int pm_grow(bw_ctx* c, DevBuf& b, uint64_t need, uint64_t keep) {
    if (b.cap >= need) return BW_OK;
    DevBuf nb;
    if (int rc = ensure(c, nb, need + need / 2)) return rc;
    if (keep && b.p) {
        hipError_t e = hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            free_dev(nb);
            c->err = std::string("parent match: growing a buffer: ") + hipGetErrorString(e);
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
struct HostSeg {
    uint32_t node, sid;
    uint64_t stage, count;
};

// The walk's host state: what pm_fetch shares with the level loop.
struct PmHost {
    bw_restore* s;
    bw_ctx* c;
    uint32_t flags;
    uint64_t n_e;
    PmWalk w;
    uint64_t err_ub = 0;  // no more errors than this can have been written
    // a level's chains
    std::vector<HostSeg> segs;
    std::vector<uint64_t> item_rows;
    uint64_t stage_rows = 0, name_total = 0;
    // scratch
    std::vector<uint32_t> out, ref_owner, next_owner, located;
    std::vector<uint64_t> eidx;
    std::vector<uint8_t> bst;
    std::vector<RsTreeHdr> hd;
    std::vector<PmTake> take;
};
}  // namespace

static int pm_refuse(bw_ctx* c, const char* why) {
    c->err = std::string("parent match: ") + why;
    return BW_EHIP;
}

static int pm_too_large(bw_ctx* c, const char* what) {
    c->err = std::string("parent match: more than 2^30 ") + what + ": the walk's tables index a level in 32 bits";
    return BW_ENOMEM;
}

static int pm_errs_for(PmHost& H, uint64_t more) {  // room for `more` further errors
    H.err_ub += more;
    DevBuf& b = H.s->pm[PM_B_ERR];
    if (int rc = pm_grow(H.c, b, H.err_ub * sizeof(bw_prune_error) + 16, (H.err_ub - more) * sizeof(bw_prune_error))) return rc;
    H.w.errs = P<bw_prune_error>(b);
    H.w.err_cap = H.err_ub;
    return BW_OK;
}

// n_refs references through the unpack chain, `slots` blobs at a time.  children = false: they are the
// first pieces of the level's items (owner = the item); round r fetches piece r of every chain that
// has one, the rows go to the staging arena and H.segs / H.item_rows say whose they are.  children =
// true: they are the first pieces of the level's parent children (owner = the child): one round.
static int pm_fetch(PmHost& H, const PmRef* d_refs, uint64_t n_refs, bool children) {
    bw_restore* s = H.s;
    bw_ctx* c = H.c;
    PmWalk& w = H.w;
    H.ref_owner.resize(n_refs);
    for (uint64_t i = 0; i < n_refs; i++) H.ref_owner[i] = (uint32_t)i;
    int ch = 0;
    for (uint64_t round = 0; n_refs; round++) {
        const bool overlong = round > H.n_e;
        if (round > H.n_e + 1) return pm_refuse(c, "a chain round past the refused one");
        if (int rc = pm_errs_for(H, n_refs)) return rc;
        if (int rc = ensure(c, s->pm[PM_B_OUT], 4 * n_refs + 16)) return rc;
        hipLaunchKernelGGL(k_pm_resolve, pm_grid(n_refs), dim3(256), 0, c->stream, w, d_refs, n_refs, (int)overlong,
                           P<uint32_t>(s->pm[PM_B_OUT]));
        HIPCHK(c, hipGetLastError());
        H.out.resize(n_refs);
        HIPCHK(c, hipMemcpyAsync(H.out.data(), s->pm[PM_B_OUT].p, 4 * n_refs, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        H.located.clear();
        for (uint64_t i = 0; i < n_refs; i++) {
            if (H.out[i] == RS_EMPTY) continue;
            if (H.out[i] >= H.n_e) return pm_refuse(c, "a reference resolved to an entry outside the table");
            H.located.push_back((uint32_t)i);
        }
        const int nx = ch;  // the next round's references: the chain buffer this round does not read
        DevBuf& next_buf = s->pm[nx ? PM_B_CHAIN1 : PM_B_CHAIN0];
        if (int rc = ensure(c, next_buf, (children ? 0 : H.located.size()) * sizeof(PmRef) + 16)) return rc;
        PmRef* d_next = P<PmRef>(next_buf);  // a child's first piece gives no next reference
        H.next_owner.clear();
        for (uint64_t lo = 0; lo < H.located.size(); lo += s->slots) {
            const uint64_t m = std::min<uint64_t>(s->slots, H.located.size() - lo);
            H.eidx.resize(m);
            for (uint64_t k = 0; k < m; k++) H.eidx[k] = H.out[H.located[lo + k]];
            RsTables t;
            if (int rc = rs_tree_decode(s, H.eidx, H.flags, m, t, H.bst)) return rc;
            if (int rc = rs_tree_parse(s, t, m, &H.hd)) return rc;
            HIPCHK(c, hipStreamSynchronize(c->stream));
            H.take.assign(m, PmTake());
            uint64_t add_rows = 0, add_names = 0, add_segs = 0;
            for (uint64_t k = 0; k < m; k++) {
                PmTake& tk = H.take[k];
                const RsTreeHdr& h = H.hd[k];
                const uint32_t owner = H.ref_owner[H.located[lo + k]];
                tk.ref = H.located[lo + k];
                tk.cst = H.bst[k];
                tk.stage = H.stage_rows + add_rows;
                tk.name_off = H.name_total + add_names;
                tk.n_rows = 0;
                tk.next = tk.seg = PM_NONE;
                if (tk.cst || h.status) continue;
                if (children) {
                    add_names += h.name_len;
                    continue;
                }
                tk.n_rows = h.n_children;
                if (h.n_children) {
                    tk.seg = H.segs.size();
                    H.segs.push_back(HostSeg{owner, (uint32_t)H.segs.size(), tk.stage, h.n_children});
                    add_segs++;
                    add_rows += h.n_children;
                    H.item_rows[owner] += h.n_children;
                }
                if (h.has_next) {
                    tk.next = H.next_owner.size();
                    H.next_owner.push_back(owner);
                }
            }
            if (H.stage_rows + add_rows > PM_MAX_ROWS) return pm_too_large(c, "children rows in a level");
            if (int rc = pm_grow(c, s->pm[PM_B_STAGE], 32 * (H.stage_rows + add_rows) + 32, 32 * H.stage_rows)) return rc;
            if (int rc = pm_grow(c, s->pm[PM_B_SEGHASH], 32 * H.segs.size() + 32, 32 * (H.segs.size() - add_segs))) return rc;
            if (int rc = pm_grow(c, s->pm[PM_B_NAMES], H.name_total + add_names + 16, H.name_total)) return rc;
            if (int rc = pm_errs_for(H, m)) return rc;
            if (int rc = ensure(c, s->pm[PM_B_TAKE], m * sizeof(PmTake) + 16)) return rc;
            w.stage = P<uint8_t>(s->pm[PM_B_STAGE]);
            w.seg_hash = P<uint8_t>(s->pm[PM_B_SEGHASH]);
            w.names = P<uint8_t>(s->pm[PM_B_NAMES]);
            HIPCHK(c, hipMemcpyAsync(s->pm[PM_B_TAKE].p, H.take.data(), m * sizeof(PmTake), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_pm_take, dim3((uint32_t)m), dim3(256), 0, c->stream, w, d_refs, P<PmTake>(s->pm[PM_B_TAKE]),
                               P<uint8_t>(s->slot_buf), t.slot_off, P<RsTreeHdr>(s->q), m, (int)children, d_next);
            HIPCHK(c, hipGetLastError());
            H.stage_rows += add_rows;
            H.name_total += add_names;
            // the slots, the tables and the take table are reused by the next sub-batch
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        d_refs = d_next;
        n_refs = H.next_owner.size();
        H.ref_owner.swap(H.next_owner);
        ch ^= 1;
    }
    return BW_OK;
}

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
    if (n_nodes > PM_MAX_ROWS) return pm_too_large(c, "scan nodes");
    if (const uint64_t bad = pm_scan_invalid(nodes, n_nodes, names_len)) {
        c->err = "parent match: scan node " + std::to_string(bad - 1) + " breaks the scan's rules";
        return BW_EINVAL;
    }
    memset(results, 0, n_nodes * sizeof(*results));  // BW_PARENT_NEW, no hash
    if (!parent_root) return BW_OK;
    hipSetDevice(c->device);

    PmHost H;
    H.s = s;
    H.c = c;
    H.flags = flags;
    H.n_e = n_e;
    PmWalk& w = H.w;
    memset(&w, 0, sizeof(w));
    w.loc = rs_locator(s);
    w.trust_before = trust_before;
    if (int rc = ensure(c, s->pm[PM_B_CTR], 8 * PM_C_COUNT)) return rc;
    if (int rc = ensure(c, s->pm[PM_B_READ], n_e + 16)) return rc;
    if (int rc = ensure(c, s->pm[PM_B_SCAN], n_nodes * sizeof(bw_restore_node) + 16)) return rc;
    if (int rc = ensure(c, s->pm[PM_B_SNAMES], names_len + 16)) return rc;
    if (int rc = ensure(c, s->pm[PM_B_RES], n_nodes * sizeof(bw_parent_result) + 16)) return rc;
    HIPCHK(c, hipMemsetAsync(s->pm[PM_B_CTR].p, 0, 8 * PM_C_COUNT, c->stream));
    HIPCHK(c, hipMemsetAsync(s->pm[PM_B_READ].p, 0, n_e + 16, c->stream));
    HIPCHK(c, hipMemsetAsync(s->pm[PM_B_RES].p, 0, n_nodes * sizeof(bw_parent_result), c->stream));
    HIPCHK(c, hipMemcpyAsync(s->pm[PM_B_SCAN].p, nodes, n_nodes * sizeof(bw_restore_node), hipMemcpyHostToDevice, c->stream));
    if (names_len) HIPCHK(c, hipMemcpyAsync(s->pm[PM_B_SNAMES].p, names, names_len, hipMemcpyHostToDevice, c->stream));
    w.ctr = P<uint64_t>(s->pm[PM_B_CTR]);
    w.read = P<uint8_t>(s->pm[PM_B_READ]);
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
        H.segs.clear();
        H.item_rows.assign(n_items, 0);
        H.stage_rows = H.name_total = 0;
        w.root = root;
        w.n_items = n_items;
        uint64_t n_child = 0, n_seg = 0;

        // ---- the items' chains: every row of every piece
        if (!root) {
            if (int rc = ensure(c, s->pm[PM_B_REFS], n_items * sizeof(PmRef) + 16)) return rc;
            // the items' first pieces as references: read a second time, as the heads of their chains
            std::vector<PmRef> hr(n_items);
            memset(hr.data(), 0, n_items * sizeof(PmRef));
            for (uint64_t i = 0; i < n_items; i++) {
                memcpy(hr[i].hash, h_items[i].hash, 32);
                memcpy(hr[i].by, h_items[i].hash, 32);  // an error of this read names the piece itself
                hr[i].by_pos = PM_NONE;
                hr[i].owner = (uint32_t)i;
            }
            HIPCHK(c, hipMemcpyAsync(s->pm[PM_B_REFS].p, hr.data(), n_items * sizeof(PmRef), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));  // hr leaves scope
            if (int rc = pm_fetch(H, P<PmRef>(s->pm[PM_B_REFS]), n_items, false)) return rc;
            n_child = H.stage_rows;
            std::stable_sort(H.segs.begin(), H.segs.end(), [](const HostSeg& a, const HostSeg& b) { return a.node < b.node; });
            n_seg = H.segs.size();
        } else {
            n_child = 1;
        }

        // ---- the level's layout: [seg_row0 (n_seg + 1) | seg_stage | node_row0 | probe_row0 (n_items + 1) |
        //      item_first | seg_node, seg_sid (u32 each)]
        lvl.assign(2 * n_seg + 1 + 3 * n_items + 1 + n_seg + 1, 0);
        uint64_t* seg_row0 = lvl.data();
        uint64_t* seg_stage = seg_row0 + n_seg + 1;
        uint64_t* node_row0 = seg_stage + n_seg;
        uint64_t* probe_row0 = node_row0 + n_items;
        uint64_t* item_first = probe_row0 + n_items + 1;
        uint32_t* seg_node = (uint32_t*)(item_first + n_items);
        uint32_t* seg_sid = seg_node + n_seg;
        uint64_t run = 0;
        for (uint64_t k = 0; k < n_seg; k++) {
            seg_row0[k] = run;
            seg_stage[k] = H.segs[k].stage;
            seg_node[k] = H.segs[k].node;
            seg_sid[k] = H.segs[k].sid;
            run += H.segs[k].count;
        }
        seg_row0[n_seg] = run;
        if (!root && run != n_child) return pm_refuse(c, "the level's rows do not add up");
        run = 0;
        uint64_t n_probes = 0;
        for (uint64_t i = 0; i < n_items; i++) {
            node_row0[i] = run;
            run += H.item_rows[i];
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
        if (int rc = ensure(c, s->pm[PM_B_CREFS], n_child * sizeof(PmRef) + 16)) return rc;
        HIPCHK(c, hipMemcpyAsync(s->pm[PM_B_LVL].p, lvl.data(), 8 * lvl.size(), hipMemcpyHostToDevice, c->stream));
        const uint64_t* d_lvl = P<uint64_t>(s->pm[PM_B_LVL]);
        w.seg_row0 = d_lvl;
        w.seg_stage = d_lvl + n_seg + 1;
        w.node_row0 = w.seg_stage + n_seg;
        w.probe_row0 = w.node_row0 + n_items;
        w.item_first = w.probe_row0 + n_items + 1;
        w.seg_node = (const uint32_t*)(w.item_first + n_items);
        w.seg_sid = w.seg_node + n_seg;
        w.child = P<PmChild>(s->pm[PM_B_CHILD]);
        w.n_seg = n_seg;
        w.n_child = n_child;
        w.n_probes = n_probes;
        w.stage = P<uint8_t>(s->pm[PM_B_STAGE]);
        w.seg_hash = P<uint8_t>(s->pm[PM_B_SEGHASH]);

        // ---- the parent children and their first pieces
        if (root) {
            PmChild hc;
            PmRef hr;
            memset(&hc, 0, sizeof(hc));
            memset(&hr, 0, sizeof(hr));
            memcpy(hc.hash, parent_root, 32);
            memcpy(hr.hash, parent_root, 32);
            HIPCHK(c, hipMemcpyAsync(s->pm[PM_B_CHILD].p, &hc, sizeof(hc), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(s->pm[PM_B_CREFS].p, &hr, sizeof(hr), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));  // hc and hr leave scope
        } else if (n_child) {
            hipLaunchKernelGGL(k_pm_rows, pm_grid(n_child), dim3(256), 0, c->stream, w, P<PmRef>(s->pm[PM_B_CREFS]));
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));  // lvl is rewritten by the next level
        if (n_child)
            if (int rc = pm_fetch(H, P<PmRef>(s->pm[PM_B_CREFS]), n_child, true)) return rc;
        w.names = P<uint8_t>(s->pm[PM_B_NAMES]);

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
            if (n_child) hipLaunchKernelGGL(k_pm_build, pm_grid(n_child), dim3(256), 0, c->stream, w, d_tab, d_best, cap);
            hipLaunchKernelGGL(k_pm_probe, pm_grid(n_probes), dim3(256), 0, c->stream, w, d_tab, d_best, cap,
                               P<uint32_t>(s->pm[PM_B_MATCH]));
            hipLaunchKernelGGL(k_pm_verdict, pm_grid(n_probes), dim3(256), 0, c->stream, w, P<uint32_t>(s->pm[PM_B_MATCH]),
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
    uint64_t ctr[PM_C_COUNT];
    HIPCHK(c, hipMemcpyAsync(ctr, w.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
    if (n_e) HIPCHK(c, hipMemcpyAsync(read, s->pm[PM_B_READ].p, n_e, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(results, s->pm[PM_B_RES].p, n_nodes * sizeof(bw_parent_result), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t n_err = ctr[PM_C_ERRORS];
    if (n_err > H.err_ub) return pm_refuse(c, "more errors than the kernels can have met");
    const uint64_t take_err = std::min(n_err, err_cap);
    if (take_err) HIPCHK(c, hipMemcpy(errs, s->pm[PM_B_ERR].p, take_err * sizeof(bw_prune_error), hipMemcpyDeviceToHost));
    counts->n_levels = n_levels ? n_levels : 1;
    counts->n_errors = n_err;
    counts->n_unchanged = ctr[PM_C_UNCHANGED];
    counts->unchanged_bytes = ctr[PM_C_BYTES];
    for (uint64_t e = 0; e < n_e; e++) counts->n_read += read[e];
    if (n_err > err_cap) {
        c->err = "parent match: " + std::to_string(n_err) + " errors do not fit err_cap";
        return BW_ENOSPC;
    }
    return BW_OK;
}
