// bw_walk.h -- the tree-chain fetch that the walks over a restore session share (the diff walk,
// bw_diff.hip, the parent match, bw_parent.hip, and impact's report walk, bw_impact.hip): n references through the unpack chain `slots` blobs
// at a time, round r fetching piece r of every next_sibling chain that has one.  Two kernels, written
// once over a walk's policy type and instantiated by each walk:
//   k_wk_resolve  one lane per reference: locate, kind, read[], and the walk's check of a first piece
//   k_wk_take     one workgroup per decoded blob: header and name, or rows and next_sibling, or both
// and the host's rounds loop, wk_fetch, with the buffer, refusal and error-list rules around it.  The
// host arithmetic (the take table, the segment layout) is bw_walk_host.h.  A policy P gives:
//   P::Walk           the walk's device state; its member f is the WkFetch
//   P::NAME           the walk's name in error texts
//   P::ROWS_TOO_MANY  the text for a level of more than P::MAX_ROWS children rows
//   P::ERRS_PER_REF   the errors k_wk_resolve can write for one reference
//   P::first(w, r)    resolve, a first piece: true when the owner is to be read for its header only
//   P::refuse(w, e)   resolve: true when the located Tree entry e is not to be opened (it counts as unread)
//   P::lost(w, owner) a later piece of the owner's chain could not be read
//   P::header(w, owner, h, name_off)  take: where a first piece's header lands
// Private; off the chunk -> hash -> dedup path (backuwup_amd/build.py OFF_PATH), like bw_restore.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/backuwup_gpu.h"
#include "bw_ctx.h"
#include "bw_restore.h"
#include "bw_walk_host.h"

namespace bw {

// the counters of a walk: the errors come first, the walk's own follow
enum { WK_C_ERRORS = 0, WK_C_COUNT = 4 };

// the session's buffers that the fetch owns (bw_restore::wk); two walks of one session never overlap
enum {
    WK_B_CTR, WK_B_READ, WK_B_ERR, WK_B_CHAIN0, WK_B_CHAIN1, WK_B_OUT, WK_B_TAKE, WK_B_STAGE, WK_B_SEGHASH, WK_B_NAMES,
    WK_B_COUNT
};
static_assert(WK_B_COUNT <= sizeof(bw_restore::wk) / sizeof(DevBuf), "bw_restore::wk holds every buffer");

// One tree reference to resolve: a first piece, or the next_sibling of the piece `by`.
struct WkRef {
    uint8_t hash[32];
    uint8_t by[32];       // the piece that names it, zero for a root
    uint64_t by_pos;      // its position there, ~0 for a next_sibling
    uint32_t owner, pad;  // what it is read for: the owner of the chain, or of the header
};

// The fetch's device state: the head of every walk's state.
struct WkFetch {
    RsLocator loc;
    uint8_t* read;    // one byte per session entry
    uint64_t* n_err;  // the error counter
    bw_prune_error* errs;
    uint64_t err_cap;
    uint8_t* stage;     // children rows in the order they were fetched
    uint8_t* seg_hash;  // per fetched segment: the hash of the piece that holds it
    uint8_t* names;     // the names of the first pieces
    // the level's lists, once every chain has ended: segments sorted by (owner, piece)
    const uint64_t *seg_row0, *seg_stage;  // a segment's first row in the lists, and in `stage`
    const uint32_t *seg_node, *seg_sid;    // its owner, and its number in fetch order
    uint64_t n_seg;
};

// ------------------------------------------------------------------ device helpers
__device__ static void wk_error(const WkFetch& f, const uint8_t* hash, const uint8_t* by, uint64_t pos, uint32_t reason) {
    const uint64_t at = atomicAdd((unsigned long long*)f.n_err, 1ull);
    if (at >= f.err_cap) return;  // the host sized the list for every error a launch can give
    bw_prune_error& e = f.errs[at];
    for (int i = 0; i < 32; i++) {
        e.hash[i] = hash[i];
        e.parent[i] = by[i];
    }
    e.child_pos = pos;
    e.reason = reason;
    e.pad = 0;
}

__device__ static inline void wk_copy32(uint8_t* d, const uint8_t* s) {
    for (int i = 0; i < 32; i++) d[i] = s[i];
}

// Every lane of the wave calls this: the lanes with push = true get consecutive places from *ctr
// (one atomic by the first of them, each lane's place from the ballot, as prune's pr_visit does).
__device__ static inline uint64_t wk_wave_place(bool push, uint64_t* ctr) {
    const uint64_t bal = __ballot(push);
    if (!bal) return 0;
    const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__ffsll((unsigned long long)bal) - 1;
    uint64_t base = 0;
    if (lane == leader) base = atomicAdd((unsigned long long*)ctr, (unsigned long long)__popcll(bal));
    const uint32_t lo = __shfl((uint32_t)base, leader), hi = __shfl((uint32_t)(base >> 32), leader);
    return (((uint64_t)hi << 32) | lo) + __popcll(bal & ((1ull << lane) - 1));
}

// the largest i < n with row0[i] <= r (row0 ascends; equal entries are empty ranges and are passed over)
__device__ static inline uint64_t wk_range_of(const uint64_t* row0, uint64_t n, uint64_t r) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (row0[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// row r of the level's lists, which lies in segment seg, where the fetch staged it
__device__ static inline const uint8_t* wk_stage_row(const WkFetch& f, uint64_t seg, uint64_t r) {
    return f.stage + 32 * (f.seg_stage[seg] + (r - f.seg_row0[seg]));
}

// the key of a name join: FNV over the name's bytes from the join's own seed
__device__ static inline uint32_t wk_key_hash(uint64_t seed, const uint8_t* p, uint64_t len) {
    uint64_t h = 0xcbf29ce484222325ull ^ seed;
    for (uint64_t i = 0; i < len; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return rs_mix(h);
}

__device__ static inline bool wk_name_eq(const uint8_t* x, uint64_t nx, const uint8_t* y, uint64_t ny) {
    if (nx != ny) return false;
    uint32_t d = 0;
    for (uint64_t i = 0; i < nx; i++) d |= x[i] ^ y[i];
    return d == 0;
}

// ------------------------------------------------------------------ resolve
// out[i] = the entry the reference names (low 32 bits, RS_EMPTY when there is none to open) and, in
// bit 32, what P::first said of it.  first: the references are first pieces.  overlong: the chain has
// more pieces than the store has entries, so every reference of the round is refused unread.
template <class Pol>
__global__ void __launch_bounds__(256) k_wk_resolve(typename Pol::Walk w, const WkRef* refs, uint64_t n, int first,
                                                    int overlong, uint64_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const WkRef& r = refs[i];
    uint64_t res = RS_EMPTY;
    if (overlong) {
        wk_error(w.f, r.hash, r.by, r.by_pos, BW_RESTORE_EFORMAT);
        Pol::lost(w, r.owner);
        out[i] = res;
        return;
    }
    const bool flag = first && Pol::first(w, r);
    uint64_t e;
    const uint8_t st = rs_locate_one(w.f.loc, r.hash, e);
    if (st) {
        wk_error(w.f, r.hash, r.by, r.by_pos, st);
    } else if (w.f.loc.entries[e].kind != BW_BLOB_TREE) {
        wk_error(w.f, r.hash, r.by, r.by_pos, BW_RESTORE_ENOTTREE);
    } else if (Pol::refuse(w, e)) {
        // the walk does not open it, and that is no error of the fetch's
    } else {
        w.f.read[e] = 1;
        res = e;
    }
    if (res == RS_EMPTY && !first) Pol::lost(w, r.owner);
    out[i] = res | (flag ? 1ull << 32 : 0);
}

// ------------------------------------------------------------------ take
// Workgroup b: blob b of the sub-batch, decoded at slots + off[b] and parsed into hdr[b].  A blob the
// chain or the parser refused is an error of its reference.  A good one gives its owner its header and
// its name (header), and its rows to the staging arena and its next_sibling to the next round (rows).
template <class Pol>
__global__ void __launch_bounds__(256) k_wk_take(typename Pol::Walk w, const WkRef* refs, const WkTake* tab,
                                                 const uint8_t* slots, const uint64_t* off, const RsTreeHdr* hdr, uint64_t m,
                                                 int header, int rows, WkRef* next) {
    const uint64_t b = blockIdx.x;
    if (b >= m) return;
    const WkTake t = tab[b];
    const WkRef& r = refs[t.ref];
    const RsTreeHdr& h = hdr[b];
    const uint32_t bad = t.cst ? t.cst : h.status;
    if (bad) {
        if (threadIdx.x == 0) {
            wk_error(w.f, r.hash, r.by, r.by_pos, bad);
            if (!header) Pol::lost(w, r.owner);
        }
        return;
    }
    const uint8_t* blob = slots + off[b];
    if (header) {
        if (threadIdx.x == 0) Pol::header(w, r.owner, h, t.name_off);
        // the parser bounded the name by the blob, and the host gave it h.name_len bytes of the arena; a
        // name is short and goes byte by byte
        for (uint64_t i = threadIdx.x; i < h.name_len; i += 256) w.f.names[t.name_off + i] = blob[h.name_pos + i];
    }
    if (!rows) return;
    if (threadIdx.x == 0) {
        if (t.seg != WK_NONE) wk_copy32(w.f.seg_hash + 32 * t.seg, r.hash);
        if (t.next != WK_NONE) {
            WkRef& x = next[t.next];
            wk_copy32(x.hash, h.next);
            wk_copy32(x.by, r.hash);
            x.by_pos = WK_NONE;
            x.owner = r.owner;
            x.pad = 0;
        }
    }
    // the rows: each wave takes pieces of RS_PIECE bytes and copies them in 16-byte vectors (the strict
    // form of the gather's copy: ch_pos lies at any byte, and nothing outside the rows is loaded);
    // t.n_rows <= h.n_children, which the parser bounded by the blob
    const uint8_t* src = blob + h.ch_pos;
    uint8_t* dst = w.f.stage + 32 * t.stage;
    const uint64_t nb = 32 * t.n_rows;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t p0 = (uint64_t)(threadIdx.x >> 6) * RS_PIECE; p0 < nb; p0 += 4ull * RS_PIECE)
        rs_copy_piece<true>(src + p0, dst + p0, nb - p0 < RS_PIECE ? nb - p0 : RS_PIECE, lane);
}

// ------------------------------------------------------------------ the host's side
static inline dim3 wk_grid(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

static inline int wk_refuse(bw_ctx* c, const char* walk, const char* why) {
    c->err = std::string(walk) + ": " + why;
    return BW_EHIP;
}

// the walks' hard limit: `what` says which count went past 2^30
static inline int wk_too_large(bw_ctx* c, const char* walk, const char* what) {
    c->err = std::string(walk) + ": " + what + ": the walk's tables index a level in 32 bits";
    return BW_ENOMEM;
}

// a buffer of at least `need` bytes that keeps its first `keep` bytes
static inline int wk_grow(bw_ctx* c, const char* walk, DevBuf& b, uint64_t need, uint64_t keep) {
    if (b.cap >= need) return BW_OK;
    DevBuf nb;
    if (int rc = ensure(c, nb, need + need / 2)) return rc;
    if (keep && b.p) {
        hipError_t e = hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            free_dev(nb);
            c->err = std::string(walk) + ": growing a buffer: " + hipGetErrorString(e);
            return BW_EHIP;
        }
    } else {
        hipStreamSynchronize(c->stream);
    }
    free_dev(b);
    b = nb;
    return BW_OK;
}

// The walk's host state: what wk_fetch shares with the walk's level loop.
template <class Pol>
struct WkHost {
    bw_restore* s;
    bw_ctx* c;
    uint32_t flags;
    uint64_t n_e;
    typename Pol::Walk w;
    uint64_t err_ub = 0;  // no more errors than this can have been written
    uint64_t n_opened = 0;  // the blobs handed to the unpack chain so far (find reports it)
    WkLevel lv;
    std::vector<WkOwner> owners;  // of the level's chains
    // scratch
    std::vector<uint64_t> out, eidx;
    std::vector<uint32_t> ref_owner, next_owner, located;
    std::vector<uint8_t> bst;
    std::vector<RsTreeHdr> hd;
    std::vector<WkTake> take;
};

// The state at the start of a call: the locator, and the counters and read[] cleared.
template <class Pol>
static int wk_open(WkHost<Pol>& H, bw_restore* s, uint32_t flags) {
    bw_ctx* c = s->c;
    H.s = s;
    H.c = c;
    H.flags = flags;
    H.n_e = s->entries.size();
    memset(&H.w, 0, sizeof(H.w));
    H.w.f.loc = rs_locator(s);
    if (int rc = ensure(c, s->wk[WK_B_CTR], 8 * WK_C_COUNT)) return rc;
    if (int rc = ensure(c, s->wk[WK_B_READ], H.n_e + 16)) return rc;
    HIPCHK(c, hipMemsetAsync(s->wk[WK_B_CTR].p, 0, 8 * WK_C_COUNT, c->stream));
    HIPCHK(c, hipMemsetAsync(s->wk[WK_B_READ].p, 0, H.n_e + 16, c->stream));
    H.w.f.n_err = P<uint64_t>(s->wk[WK_B_CTR]) + WK_C_ERRORS;
    H.w.f.read = P<uint8_t>(s->wk[WK_B_READ]);
    return BW_OK;
}

template <class Pol>
static int wk_errs_for(WkHost<Pol>& H, uint64_t more) {  // room for `more` further errors
    H.err_ub += more;
    DevBuf& b = H.s->wk[WK_B_ERR];
    if (int rc = wk_grow(H.c, Pol::NAME, b, H.err_ub * sizeof(bw_prune_error) + 16, (H.err_ub - more) * sizeof(bw_prune_error)))
        return rc;
    H.w.f.errs = P<bw_prune_error>(b);
    H.w.f.err_cap = H.err_ub;
    return BW_OK;
}

// n_refs references through the unpack chain, `slots` blobs at a time.  header: they are first pieces,
// and each gives its owner its header and name (round 0 only).  rows: round r fetches piece r of every
// chain that has one; the rows go to the staging arena and H.lv.segs says whose they are.  owners: the
// chains' owners (H.owners), or null when the owners are not theirs.
template <class Pol>
static int wk_fetch(WkHost<Pol>& H, const WkRef* d_refs, uint64_t n_refs, bool header, bool rows, WkOwner* owners) {
    bw_restore* s = H.s;
    bw_ctx* c = H.c;
    typename Pol::Walk& w = H.w;
    H.ref_owner.resize(n_refs);
    for (uint64_t i = 0; i < n_refs; i++) H.ref_owner[i] = (uint32_t)i;
    int ch = 0;
    for (uint64_t round = 0; n_refs; round++, header = false) {
        const bool overlong = round > H.n_e;
        if (round > H.n_e + 1) return wk_refuse(c, Pol::NAME, "a chain round past the refused one");
        if (int rc = wk_errs_for(H, Pol::ERRS_PER_REF * n_refs)) return rc;
        if (int rc = ensure(c, s->wk[WK_B_OUT], 8 * n_refs + 16)) return rc;
        hipLaunchKernelGGL(k_wk_resolve<Pol>, wk_grid(n_refs), dim3(256), 0, c->stream, w, d_refs, n_refs, (int)header,
                           (int)overlong, P<uint64_t>(s->wk[WK_B_OUT]));
        HIPCHK(c, hipGetLastError());
        H.out.resize(n_refs);
        HIPCHK(c, hipMemcpyAsync(H.out.data(), s->wk[WK_B_OUT].p, 8 * n_refs, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        H.located.clear();
        for (uint64_t i = 0; i < n_refs; i++) {
            const uint32_t e = (uint32_t)H.out[i];
            if (header && owners) owners[H.ref_owner[i]].skip = (H.out[i] >> 32) & 1;
            if (e == RS_EMPTY) continue;
            if (e >= H.n_e) return wk_refuse(c, Pol::NAME, "a reference resolved to an entry outside the table");
            H.located.push_back((uint32_t)i);
        }
        // the next round's references: the chain buffer this round does not read (without rows there are none)
        DevBuf& next_buf = s->wk[ch ? WK_B_CHAIN1 : WK_B_CHAIN0];
        if (int rc = ensure(c, next_buf, (rows ? H.located.size() : 0) * sizeof(WkRef) + 16)) return rc;
        WkRef* d_next = P<WkRef>(next_buf);
        H.next_owner.clear();
        for (uint64_t lo = 0; lo < H.located.size(); lo += s->slots) {
            const uint64_t m = std::min<uint64_t>(s->slots, H.located.size() - lo);
            H.eidx.resize(m);
            for (uint64_t k = 0; k < m; k++) H.eidx[k] = (uint32_t)H.out[H.located[lo + k]];
            RsTables t;
            if (int rc = rs_tree_decode(s, H.eidx, H.flags, m, t, H.bst)) return rc;
            H.n_opened += m;
            if (int rc = rs_tree_parse(s, t, m, &H.hd)) return rc;
            HIPCHK(c, hipStreamSynchronize(c->stream));
            H.take.resize(m);
            const WkAdd add = wk_plan(H.lv, H.located.data() + lo, H.ref_owner.data(), H.bst.data(), H.hd.data(), m, header,
                                      rows, owners, H.take.data(), H.next_owner);
            const uint64_t stage_rows = H.lv.stage_rows, name_total = H.lv.name_total, n_segs = H.lv.segs.size();
            if (stage_rows + add.rows > Pol::MAX_ROWS) return wk_too_large(c, Pol::NAME, Pol::ROWS_TOO_MANY);
            if (int rc = wk_grow(c, Pol::NAME, s->wk[WK_B_STAGE], 32 * (stage_rows + add.rows) + 32, 32 * stage_rows)) return rc;
            if (int rc = wk_grow(c, Pol::NAME, s->wk[WK_B_SEGHASH], 32 * n_segs + 32, 32 * (n_segs - add.segs))) return rc;
            if (int rc = wk_grow(c, Pol::NAME, s->wk[WK_B_NAMES], name_total + add.names + 16, name_total)) return rc;
            if (int rc = wk_errs_for(H, m)) return rc;
            if (int rc = ensure(c, s->wk[WK_B_TAKE], m * sizeof(WkTake) + 16)) return rc;
            w.f.stage = P<uint8_t>(s->wk[WK_B_STAGE]);
            w.f.seg_hash = P<uint8_t>(s->wk[WK_B_SEGHASH]);
            w.f.names = P<uint8_t>(s->wk[WK_B_NAMES]);
            HIPCHK(c, hipMemcpyAsync(s->wk[WK_B_TAKE].p, H.take.data(), m * sizeof(WkTake), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_wk_take<Pol>, dim3((uint32_t)m), dim3(256), 0, c->stream, w, d_refs, P<WkTake>(s->wk[WK_B_TAKE]),
                               P<uint8_t>(s->slot_buf), t.slot_off, P<RsTreeHdr>(s->q), m, (int)header, (int)rows, d_next);
            HIPCHK(c, hipGetLastError());
            H.lv.stage_rows += add.rows;
            H.lv.name_total += add.names;
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

// The level's segment tables at the head of the level's table `lvl` (n_u64 u64 places of the walk's own
// between them): [seg_row0 (n_seg + 1) | seg_stage | the walk's own | seg_node, seg_sid (u32 each)],
// filled on the host by wk_layout and named on the device from d_lvl.  -> the rows in all.
static inline uint64_t wk_level_tables(WkFetch& f, std::vector<WkSeg>& segs, std::vector<uint64_t>& lvl, uint64_t n_own) {
    const uint64_t n_seg = segs.size();
    lvl.assign(2 * n_seg + 1 + n_own + n_seg + 1, 0);
    f.n_seg = n_seg;
    return wk_layout(segs, lvl.data(), lvl.data() + n_seg + 1, (uint32_t*)(lvl.data() + 2 * n_seg + 1 + n_own),
                     (uint32_t*)(lvl.data() + 2 * n_seg + 1 + n_own) + n_seg);
}

static inline void wk_level_pointers(WkFetch& f, const uint64_t* d_lvl, uint64_t n_own) {
    f.seg_row0 = d_lvl;
    f.seg_stage = d_lvl + f.n_seg + 1;
    f.seg_node = (const uint32_t*)(f.seg_stage + f.n_seg + n_own);
    f.seg_sid = f.seg_node + f.n_seg;
}

// The error tail of a call's results: n_err errors were counted; the first min(n_err, err_cap) go to
// the caller.  -> BW_OK, BW_ENOSPC with its text when they do not all fit, or a refusal.
template <class Pol>
static int wk_errors_out(WkHost<Pol>& H, uint64_t n_err, bw_prune_error* errs, uint64_t err_cap) {
    bw_ctx* c = H.c;
    if (n_err > H.err_ub) return wk_refuse(c, Pol::NAME, "more errors than the kernels can have met");
    const uint64_t take_err = std::min(n_err, err_cap);
    if (take_err) HIPCHK(c, hipMemcpy(errs, H.s->wk[WK_B_ERR].p, take_err * sizeof(bw_prune_error), hipMemcpyDeviceToHost));
    if (n_err > err_cap) {
        c->err = std::string(Pol::NAME) + ": " + std::to_string(n_err) + " errors do not fit err_cap";
        return BW_ENOSPC;
    }
    return BW_OK;
}

}  // namespace bw
