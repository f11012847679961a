// bw_restore.h -- private declarations of the restore session (bw_restore.hip): the locator's
// tables and the gather's instance tables (the tree parser's record, RsTreeHdr, is bw_store_layout.h's,
// free of HIP).  Off the chunk -> hash -> dedup path (backuwup_amd/build.py OFF_PATH), like bw_unpack.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/backuwup_gpu.h"
#include "bw_ctx.h"
#include "bw_store_layout.h"

struct bw_restore;

namespace bw {

constexpr uint32_t RS_EMPTY = 0xffffffffu;            // a free table slot (tables hold u32 record indices)
constexpr uint64_t RS_SLOT_STRIDE = BW_BLOB_MAX_UNCOMPRESSED_SIZE + 32;  // a decode slot plus skew and load slack
constexpr uint32_t RS_DEFAULT_SLOTS = 1024;           // 3 GiB of decode room
constexpr uint64_t RS_MAX_INSTANCES = 1u << 20;       // instances of one sub-batch (bounds the tables)

// One instance of a sub-batch: the blob in decode slot `slot` is the next piece of the output
// (valid = 0: the instance is dropped, its file failed earlier or the window is full).
struct RsInst {
    uint32_t slot, valid;
};

// ------------------------------------------------------------------ device code shared with bw_prune.hip and bw_check.hip
// The locator's probes (the tables are described in bw_restore.hip) and the body of the piece copy.
__device__ static inline uint64_t rs_load8(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i);
    return v;
}

__device__ static inline uint32_t rs_mix(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    return (uint32_t)x;
}

__device__ static inline bool rs_eq(const uint8_t* a, const uint8_t* b, uint32_t n) {
    uint32_t d = 0;
    for (uint32_t i = 0; i < n; i++) d |= a[i] ^ b[i];
    return d == 0;
}

// keys of `klen` bytes at rec + idx * stride (+ a u32 salt at salt_at, when salt_at != ~0, that
// must be equal too: the packfile position of a header entry)
struct RsKeys {
    const uint8_t* rec;
    uint32_t stride, klen, salt_at;
};

__device__ static inline uint32_t rs_salt(const RsKeys& k, uint32_t idx) {
    if (k.salt_at == ~0u) return 0;
    uint32_t v;
    memcpy(&v, k.rec + (uint64_t)idx * k.stride + k.salt_at, 4);
    return v;
}

__device__ static void rs_insert(uint32_t* tab, uint32_t cap, const RsKeys& k, uint32_t idx) {
    const uint8_t* key = k.rec + (uint64_t)idx * k.stride;
    const uint32_t salt = rs_salt(k, idx);
    const uint32_t h = rs_mix(rs_load8(key) ^ ((uint64_t)salt << 32));
    for (uint32_t probe = 0; probe < cap; probe++) {
        const uint32_t slot = (h + probe) & (cap - 1);
        uint32_t cur = atomicCAS(&tab[slot], RS_EMPTY, idx);
        if (cur == RS_EMPTY) return;
        if (rs_salt(k, cur) == salt && rs_eq(k.rec + (uint64_t)cur * k.stride, key, k.klen)) {
            atomicMin(&tab[slot], idx);
            return;
        }
    }
}

__device__ static uint32_t rs_find(const uint32_t* tab, uint32_t cap, const RsKeys& k, const uint8_t* key, uint32_t salt) {
    const uint32_t h = rs_mix(rs_load8(key) ^ ((uint64_t)salt << 32));
    for (uint32_t probe = 0; probe < cap; probe++) {
        const uint32_t cur = tab[(h + probe) & (cap - 1)];
        if (cur == RS_EMPTY) return RS_EMPTY;
        if (rs_salt(k, cur) == salt && rs_eq(k.rec + (uint64_t)cur * k.stride, key, k.klen)) return cur;
    }
    return RS_EMPTY;
}

// the session's two tables as a kernel takes them (a cap of 0: the table is empty)
struct RsLocator {
    const uint8_t* items;
    const uint32_t *item_tab, *item_pos;
    const bw_unpack_entry* entries;
    const uint32_t* entry_tab;
    uint32_t item_cap, entry_cap;
};

// bw_restore_locate for one hash: BW_RESTORE_OK and the entry's index, or a locate status and ~0
__device__ static inline uint8_t rs_locate_one(const RsLocator& L, const uint8_t* key, uint64_t& idx) {
    idx = ~0ull;
    const uint32_t item = L.item_cap ? rs_find(L.item_tab, L.item_cap, RsKeys{L.items, BW_INDEX_ENTRY_BYTES, 32, ~0u}, key, 0) : RS_EMPTY;
    if (item == RS_EMPTY) return BW_RESTORE_ENOTFOUND;
    if (L.item_pos[item] == RS_EMPTY) return BW_RESTORE_ENOPACKFILE;
    const uint32_t e = L.entry_cap ? rs_find(L.entry_tab, L.entry_cap,
                                             RsKeys{(const uint8_t*)L.entries, (uint32_t)sizeof(bw_unpack_entry), 32, 32}, key,
                                             L.item_pos[item])
                                   : RS_EMPTY;
    if (e == RS_EMPTY) return BW_RESTORE_EMISMATCH;
    idx = e;
    return BW_RESTORE_OK;
}

typedef uint32_t rs_u4 __attribute__((ext_vector_type(4)));

// One wave copies nb <= RS_PIECE bytes from s to d, both at arbitrary bytes (k_rs_gather describes
// the scheme).  STRICT: no byte outside [s, s + nb) is loaded -- the head grows by one vector when
// the first aligned load would start before s, and the last vector goes to the byte tail when its
// second load would end past s + nb (head and tail stay below 32 bytes, so one lane each).
template <bool STRICT>
__device__ static inline void rs_copy_piece(const uint8_t* s, uint8_t* d, uint64_t nb, uint32_t lane) {
    const uint64_t to16 = (16 - ((uintptr_t)d & 15)) & 15;
    uint64_t head = to16;
    if (STRICT && head < (((uintptr_t)s + head) & 15)) head += 16;
    if (head > nb) head = nb;
    if (lane < head) d[lane] = s[lane];
    uint64_t nvec = (nb - head) / 16;
    const uint8_t* sv = s + head;
    rs_u4* dv = (rs_u4*)(d + head);
    const uint32_t sh = (uint32_t)((uintptr_t)sv & 15);
    if (STRICT && sh && nvec && nb - head - 16 * nvec < 16 - sh) nvec--;
    if (sh == 0) {
        const rs_u4* av = (const rs_u4*)sv;
        for (uint64_t v = lane; v < nvec; v += 64) dv[v] = av[v];
    } else {
        const rs_u4* av = (const rs_u4*)(sv - sh);
        const uint32_t q = sh >> 2, r = sh & 3;
        for (uint64_t v = lane; v < nvec; v += 64) {
            const rs_u4 a = av[v], b = av[v + 1];
            // the five dwords the 16 bytes lie in: dwords q .. q + 4 of the eight loaded, picked by
            // selects (two levels of v_cndmask on q's bits), not by branches
            const bool q1 = q & 1, q2 = q & 2;
            const uint32_t e0 = q1 ? a.y : a.x, e1 = q1 ? a.z : a.y, e2 = q1 ? a.w : a.z, e3 = q1 ? b.x : a.w,
                           e4 = q1 ? b.y : b.x, e5 = q1 ? b.z : b.y, e6 = q1 ? b.w : b.z;
            const uint32_t w0 = q2 ? e2 : e0, w1 = q2 ? e3 : e1, w2 = q2 ? e4 : e2, w3 = q2 ? e5 : e3,
                           w4 = q2 ? e6 : e4;
            rs_u4 o;
            o.x = __builtin_amdgcn_alignbyte(w1, w0, r);
            o.y = __builtin_amdgcn_alignbyte(w2, w1, r);
            o.z = __builtin_amdgcn_alignbyte(w3, w2, r);
            o.w = __builtin_amdgcn_alignbyte(w4, w3, r);
            dv[v] = o;
        }
    }
    const uint64_t done = head + 16 * nvec;
    if (lane < nb - done) d[done + lane] = s[done + lane];
}

// the three tables; cap_* are powers of two
void launch_rs_build_ids(hipStream_t st, const uint8_t* ids, uint64_t n_pf, uint32_t* tab, uint32_t cap);
void launch_rs_build_items(hipStream_t st, const uint8_t* items, uint64_t n_items, const uint8_t* ids,
                           const uint32_t* id_tab, uint32_t id_cap, uint32_t* item_pos, uint32_t* tab, uint32_t cap);
void launch_rs_build_entries(hipStream_t st, const bw_unpack_entry* entries, uint64_t n, uint32_t* tab, uint32_t cap);
void launch_rs_locate(hipStream_t st, const uint8_t* hashes, uint64_t n, const RsLocator& loc, uint64_t* entry_idx,
                      uint8_t* status);
// tree blobs: blob b lies at blobs + off[b], len[b] bytes
void launch_rs_tree_parse(hipStream_t st, const uint8_t* blobs, const uint64_t* off, const uint64_t* len, uint64_t n,
                          RsTreeHdr* out);
// out + dst[k] receives the len[k] bytes at blobs + src[k] (a parsed blob's name, or its children rows)
void launch_rs_tree_emit(hipStream_t st, const uint8_t* blobs, const uint64_t* src, const uint64_t* len,
                         const uint64_t* dst, uint64_t n, uint8_t* out);
// d_len[map[k]] = status[k] ? 0 : len[k]
void launch_rs_scatter_lens(hipStream_t st, const uint64_t* len, const uint32_t* status, const uint64_t* map, uint64_t n,
                            uint64_t* d_len);
// exclusive scan of the instances' lengths from *run (advanced by their sum); piece0[i] = the
// instances' pieces before i, piece0[n] their total
void launch_rs_scan(hipStream_t st, const RsInst* inst, uint64_t n, const uint64_t* slot_len, uint64_t* run,
                    uint64_t* dst_off, uint64_t* piece0);
void launch_rs_gather(hipStream_t st, const RsInst* inst, uint64_t n, const uint8_t* slots, const uint64_t* slot_off,
                      const uint64_t* slot_len, const uint64_t* dst_off, const uint64_t* piece0, uint8_t* dst,
                      uint64_t dst_cap);

// bw_unpack_blobs_device (bw_capi_pack.hip) with the regenerated sizes left on the device as well:
// d_len (device, n x u64, optional) receives out_len[i] (0 for a blob that failed to open or decode),
// d_map (device, n x u64) is scratch.
int unpack_blobs_core(bw_ctx* c, const uint8_t* prk, const uint8_t* d_pf, const bw_packfile* pf, uint64_t npf,
                      const bw_unpack_entry* entries, uint64_t n, uint32_t flags, uint8_t* d_dst, const uint64_t* dst_off,
                      uint64_t* out_len, uint8_t* status, uint64_t* d_len, uint64_t* d_map);

// A sub-batch's device tables, carved from s->tab: per slot its length, offset and scratch, per
// instance its record, destination and piece prefix.
struct RsTables {
    uint64_t *slot_len, *slot_off, *map, *dst_off, *piece0;
    RsInst* inst;
};

// What the range check needs of a packfile (prune's mark, check's structure pass).
struct PrPackfile {
    uint64_t size, header_len;
};

// ------------------------------------------------------------------ the session's shared steps (bw_restore.hip)
RsLocator rs_locator(const bw_restore* s);
std::vector<PrPackfile> rs_packfile_table(const bw_restore* s);

// The nonces of m blobs out of the packfile buffer, 12 bytes each, to `out` (host; synchronous).
// n_off[k] is blob k's nonce (blob_place).  The first 20 * m bytes of `scratch` are used (it is grown
// to hold them); what a caller keeps behind them stays.
int rs_fetch_nonces(bw_ctx* c, const uint8_t* d_pf, const uint64_t* n_off, uint64_t m, DevBuf& scratch, uint8_t* out);

int rs_tables(bw_restore* s, uint64_t m, uint64_t ni, RsTables& t);
// m located blobs (entry indices eidx) opened and decoded into the slots at off[k]; sizes on the
// device in t.slot_len, and with the statuses on the host (synchronous)
int rs_decode(bw_restore* s, const std::vector<uint64_t>& eidx, const std::vector<uint64_t>& off, uint32_t flags,
              const RsTables& t, std::vector<uint64_t>& out_len, std::vector<uint8_t>& st);

// One sub-batch of a tree walk (restore's, prune's mark, check's FULL pass), in two steps.
// rs_tree_decode: the m <= slots blobs eidx, blob k into the slot at k * RS_SLOT_STRIDE (rs_tables
// with ni instance places, then rs_decode); bst[k] = the chain's status.  rs_tree_parse: the parser
// over those slots, the headers to s->q, and to hd (host) when hd is given.  Without hd the launch is
// left unchecked: the caller's next kernel reads the headers where they are, and checks both.
// Neither synchronizes past rs_decode: the caller does, before the slots and the tables are reused.
int rs_tree_decode(bw_restore* s, const std::vector<uint64_t>& eidx, uint32_t flags, uint64_t ni, RsTables& t,
                   std::vector<uint8_t>& bst);
int rs_tree_parse(bw_restore* s, const RsTables& t, uint64_t m, std::vector<RsTreeHdr>* hd);

}  // namespace bw

// the session (bw_restore.hip opens and closes it; bw_prune.hip works over it)
struct bw_restore {
    bw_ctx* c = nullptr;
    uint8_t prk[32];
    const uint8_t* d_pf = nullptr;
    std::vector<bw_packfile> pf;
    std::vector<bw_unpack_entry> entries;
    uint64_t n_items = 0;
    uint32_t slots = 0;
    uint32_t id_cap = 0, item_cap = 0, entry_cap = 0;
    DevBuf ids, items, d_entries, id_tab, item_tab, item_pos, entry_tab;
    DevBuf slot_buf;  // slots x RS_SLOT_STRIDE
    DevBuf q;         // locate: [entry_idx | hashes | status]
    DevBuf tab;       // a sub-batch's tables
    DevBuf run;       // the gather's running output offset
    DevBuf emit;      // the parser's packed names and children rows
    DevBuf win;       // bw_restore_files' window
    DevBuf pf_buf;    // bw_restore_open_host: the packfiles
    DevBuf pr_bits, pr_front[2], pr_ctr, pr_err, pr_stat, pr_tab, pr_hdr;  // prune (bw_prune.hip)
    DevBuf ck_buf;  // check (bw_check.hip)
    DevBuf rk_buf;  // rekey (bw_rekey.hip)
    // the walks over the session; two calls never overlap (one stream, every entry point returns synchronised)
    DevBuf wk[12];  // the tree-chain fetch they share (bw_walk.h): its buffers by WK_B_*
    DevBuf df[12];  // diff (bw_diff.hip): its own buffers by DF_B_*
    DevBuf pm[12];  // parent match (bw_parent.hip): its own buffers by PM_B_*
    DevBuf im[16];  // impact (bw_impact.hip): the mark's and the report walk's buffers by IM_B_*
    DevBuf rt[8];   // retain (bw_retain.hip): its own buffers by RT_B_*; its walk's are impact's mark's
    DevBuf fd[16];  // find (bw_find.hip): its own buffers by FD_B_*
};
