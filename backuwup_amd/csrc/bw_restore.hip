// bw_restore.hip -- the restore session (include/backuwup_gpu_pack.h, "restore"): the data path of
// dir_unpacker.rs:14-130 on the device.  Three parts: the locator (two open-addressing tables over
// whole 32-byte hashes, like bw_dedup.hip's), the tree parser (bincode::deserialize::<Tree>, the
// inverse of bw_tree_serialize) and the file gather (k_rs_gather, the HBM-bound kernel).  Opening
// and decoding blobs goes through the unpack chain unchanged (unpack_blobs_core, bw_capi_pack.hip).
// The session owns all of its state; the context lends its stream and its synchronous scratch.
#include <string.h>

#include <algorithm>
#include <array>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/backuwup_gpu.h"
#include "bw_device.h"
#include "bw_internal.h"
#include "bw_ctx.h"
#include "bw_unpack.h"
#include "bw_restore.h"

using namespace bw;

// ------------------------------------------------------------------ the locator's tables
// A table slot holds the index of a record (an id, an index item, a header entry) or RS_EMPTY; the
// key is read from the record, so equal keys are found by comparing all of their bytes.  Insertion
// claims a free slot with one atomicCAS; on meeting an equal key it keeps the lower record index
// (atomicMin: the records are immutable, so a reader that compares against either index sees the
// same key).  Probing is linear from a mix of the key's first 8 bytes and is bounded by the table
// size; the tables are at most half full.

__global__ void k_rs_build_ids(const uint8_t* ids, uint64_t n, uint32_t* tab, uint32_t cap) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rs_insert(tab, cap, RsKeys{ids, 12, 12, ~0u}, (uint32_t)i);
}

// hash -> packfile position: item i's packfile id is resolved against the id table once, here
__global__ void k_rs_build_items(const uint8_t* items, uint64_t n, const uint8_t* ids, const uint32_t* id_tab,
                                 uint32_t id_cap, uint32_t* item_pos, uint32_t* tab, uint32_t cap) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    item_pos[i] = rs_find(id_tab, id_cap, RsKeys{ids, 12, 12, ~0u}, items + i * BW_INDEX_ENTRY_BYTES + 32, 0);
    rs_insert(tab, cap, RsKeys{items, BW_INDEX_ENTRY_BYTES, 32, ~0u}, (uint32_t)i);
}

// (packfile position, hash) -> lowest entry index
__global__ void k_rs_build_entries(const bw_unpack_entry* entries, uint64_t n, uint32_t* tab, uint32_t cap) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rs_insert(tab, cap, RsKeys{(const uint8_t*)entries, (uint32_t)sizeof(bw_unpack_entry), 32, 32}, (uint32_t)i);
}

__global__ void k_rs_locate(const uint8_t* hashes, uint64_t n, const uint8_t* items, const uint32_t* item_tab,
                            uint32_t item_cap, const uint32_t* item_pos, const bw_unpack_entry* entries,
                            const uint32_t* entry_tab, uint32_t entry_cap, uint64_t* entry_idx, uint8_t* status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t idx;
    status[i] = rs_locate_one(RsLocator{items, item_tab, item_pos, entries, entry_tab, item_cap, entry_cap}, hashes + 32 * i, idx);
    entry_idx[i] = idx;
}

static dim3 rs_grid(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

void bw::launch_rs_build_ids(hipStream_t st, const uint8_t* ids, uint64_t n_pf, uint32_t* tab, uint32_t cap) {
    if (n_pf) hipLaunchKernelGGL(k_rs_build_ids, rs_grid(n_pf), dim3(256), 0, st, ids, n_pf, tab, cap);
}
void bw::launch_rs_build_items(hipStream_t st, const uint8_t* items, uint64_t n_items, const uint8_t* ids,
                               const uint32_t* id_tab, uint32_t id_cap, uint32_t* item_pos, uint32_t* tab, uint32_t cap) {
    if (n_items)
        hipLaunchKernelGGL(k_rs_build_items, rs_grid(n_items), dim3(256), 0, st, items, n_items, ids, id_tab, id_cap,
                           item_pos, tab, cap);
}
void bw::launch_rs_build_entries(hipStream_t st, const bw_unpack_entry* entries, uint64_t n, uint32_t* tab, uint32_t cap) {
    if (n) hipLaunchKernelGGL(k_rs_build_entries, rs_grid(n), dim3(256), 0, st, entries, n, tab, cap);
}
void bw::launch_rs_locate(hipStream_t st, const uint8_t* hashes, uint64_t n, const RsLocator& L, uint64_t* entry_idx,
                          uint8_t* status) {
    if (n)
        hipLaunchKernelGGL(k_rs_locate, rs_grid(n), dim3(256), 0, st, hashes, n, L.items, L.item_tab, L.item_cap, L.item_pos,
                           L.entries, L.entry_tab, L.entry_cap, entry_idx, status);
}

// ------------------------------------------------------------------ the tree parser
// bincode::deserialize::<Tree>(blob) of bincode 1.3.3 (dir_unpacker.rs:128): the legacy free function,
// so fixint little endian and trailing bytes allowed.  Tree { kind: u32 tag, name: u64 length +
// UTF-8, metadata { size, mtime, ctime: one-byte Option tag + u64 }, children: u64 count + 32-byte
// rows, next_sibling: Option tag + 32 bytes }.  One blob per lane.  Every length is compared with
// what is left of the blob before it is used, so a damaged blob cannot send a read outside it.

__device__ static inline bool rs_rd(const uint8_t* p, uint64_t len, uint64_t& at, uint32_t n, uint64_t& v) {
    if (len - at < n) return false;  // at <= len always
    v = 0;
    for (uint32_t i = 0; i < n; i++) v |= (uint64_t)p[at + i] << (8 * i);
    at += n;
    return true;
}

// String::from_utf8 (core::str::from_utf8): well-formed UTF-8 of Unicode's table 3-7 -- no overlong
// forms, no surrogates, nothing above U+10FFFF, no truncated sequence, no stray continuation byte
__device__ static bool rs_utf8(const uint8_t* p, uint64_t n) {
    uint64_t i = 0;
    while (i < n) {
        const uint32_t b = p[i];
        if (b < 0x80) {
            i++;
            continue;
        }
        uint32_t more, lo = 0x80, hi = 0xbf;
        if (b >= 0xc2 && b <= 0xdf) {
            more = 1;
        } else if (b >= 0xe0 && b <= 0xef) {
            more = 2;
            if (b == 0xe0) lo = 0xa0;
            if (b == 0xed) hi = 0x9f;
        } else if (b >= 0xf0 && b <= 0xf4) {
            more = 3;
            if (b == 0xf0) lo = 0x90;
            if (b == 0xf4) hi = 0x8f;
        } else {
            return false;
        }
        if (n - i - 1 < more) return false;
        const uint32_t c1 = p[i + 1];
        if (c1 < lo || c1 > hi) return false;
        for (uint32_t k = 2; k <= more; k++)
            if ((p[i + k] & 0xc0) != 0x80) return false;
        i += more + 1;
    }
    return true;
}

__global__ void k_rs_tree_parse(const uint8_t* blobs, const uint64_t* off, const uint64_t* blen, uint64_t n, RsTreeHdr* out) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const uint8_t* p = blobs + off[b];
    const uint64_t len = blen[b];
    RsTreeHdr h;
    memset(&h, 0, sizeof(h));
    h.status = BW_RESTORE_EFORMAT;
    uint64_t at = 0, v = 0;
    bool ok = rs_rd(p, len, at, 4, v) && v <= 1;
    h.kind = (uint32_t)v;
    ok = ok && rs_rd(p, len, at, 8, v) && v <= len - at;
    if (ok) {
        h.name_pos = at;
        h.name_len = v;
        at += v;
        ok = rs_utf8(p + h.name_pos, h.name_len);
    }
    uint64_t meta[3] = {0, 0, 0};
    for (int k = 0; k < 3 && ok; k++) {
        ok = rs_rd(p, len, at, 1, v) && v <= 1;
        if (ok && v == 1) {
            h.flags |= 1u << k;  // BW_TREE_HAS_SIZE, _MTIME, _CTIME
            ok = rs_rd(p, len, at, 8, meta[k]);
        }
    }
    h.size = meta[0];
    h.mtime = meta[1];
    h.ctime = meta[2];
    ok = ok && rs_rd(p, len, at, 8, v) && v <= (len - at) / 32;
    if (ok) {
        h.ch_pos = at;
        h.n_children = v;
        at += 32 * v;
        ok = rs_rd(p, len, at, 1, v) && v <= 1;
    }
    if (ok && v == 1) {
        ok = len - at >= 32;
        if (ok) {
            h.has_next = 1;
            for (int i = 0; i < 32; i++) h.next[i] = p[at + i];
        }
    }
    if (ok) h.status = 0;
    out[b] = h;
}

// one wave per region
__global__ void k_rs_tree_emit(const uint8_t* blobs, const uint64_t* src, const uint64_t* len, const uint64_t* dst,
                               uint64_t n, uint8_t* out) {
    const uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
    if (k >= n) return;
    const uint8_t* s = blobs + src[k];
    uint8_t* d = out + dst[k];
    for (uint64_t i = threadIdx.x % 64; i < len[k]; i += 64) d[i] = s[i];
}

void bw::launch_rs_tree_parse(hipStream_t st, const uint8_t* blobs, const uint64_t* off, const uint64_t* len, uint64_t n,
                              RsTreeHdr* out) {
    if (n) hipLaunchKernelGGL(k_rs_tree_parse, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, st, blobs, off, len, n, out);
}
void bw::launch_rs_tree_emit(hipStream_t st, const uint8_t* blobs, const uint64_t* src, const uint64_t* len,
                             const uint64_t* dst, uint64_t n, uint8_t* out) {
    if (n) hipLaunchKernelGGL(k_rs_tree_emit, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, st, blobs, src, len, dst, n, out);
}

// ------------------------------------------------------------------ sizes, scan, gather
__global__ void k_rs_scatter_lens(const uint64_t* len, const uint32_t* status, const uint64_t* map, uint64_t n,
                                  uint64_t* d_len) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) d_len[map[k]] = status[k] ? 0 : len[k];
}

void bw::launch_rs_scatter_lens(hipStream_t st, const uint64_t* len, const uint32_t* status, const uint64_t* map,
                                uint64_t n, uint64_t* d_len) {
    if (n) hipLaunchKernelGGL(k_rs_scatter_lens, rs_grid(n), dim3(256), 0, st, len, status, map, n, d_len);
}

__device__ static inline uint64_t rs_pieces(uint64_t len) { return (len + RS_PIECE - 1) / RS_PIECE; }

// One workgroup of 1,024 lanes walks the instances 1,024 at a time: an exclusive scan of their
// lengths (from *run, which it leaves advanced: the running offset that carries a call's place in
// the output across sub-batches without the host) and of their piece counts.
__global__ void __launch_bounds__(1024) k_rs_scan(const RsInst* inst, uint64_t n, const uint64_t* slot_len, uint64_t* run,
                                                  uint64_t* dst_off, uint64_t* piece0) {
    __shared__ uint64_t s_len[1024], s_pc[1024];
    const uint32_t t = threadIdx.x;
    uint64_t base_len = *run, base_pc = 0;
    for (uint64_t lo = 0; lo < n; lo += 1024) {
        const uint64_t i = lo + t;
        uint64_t len = 0;
        if (i < n && inst[i].valid) len = slot_len[inst[i].slot];
        const uint64_t pc = rs_pieces(len);
        s_len[t] = len;
        s_pc[t] = pc;
        __syncthreads();
        for (uint32_t d = 1; d < 1024; d <<= 1) {
            const uint64_t a = t >= d ? s_len[t - d] : 0, b = t >= d ? s_pc[t - d] : 0;
            __syncthreads();
            s_len[t] += a;
            s_pc[t] += b;
            __syncthreads();
        }
        if (i < n) {
            dst_off[i] = base_len + s_len[t] - len;
            piece0[i] = base_pc + s_pc[t] - pc;
        }
        base_len += s_len[1023];
        base_pc += s_pc[1023];
        __syncthreads();
    }
    if (t == 0) {
        *run = base_len;
        piece0[n] = base_pc;
    }
}

void bw::launch_rs_scan(hipStream_t st, const RsInst* inst, uint64_t n, const uint64_t* slot_len, uint64_t* run,
                        uint64_t* dst_off, uint64_t* piece0) {
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, st, inst, n, slot_len, run, dst_off, piece0);
}

// k_rs_gather: every instance's blob copied from its decode slot to its place in its file.  A wave
// takes one piece (RS_PIECE bytes of one instance, found by a binary search of the piece prefix), so
// a 3 MiB chunk is 96 waves' work and a chunk of a few KiB one wave's.  Source and destination start
// at arbitrary bytes: the piece's first bytes up to the destination's next 16-byte boundary and its
// last 0-15 bytes go byte by byte; between them every lane stores 16 aligned bytes per step, built
// from one aligned 16-byte load when source and destination agree mod 16 and otherwise from two
// neighbouring ones shifted together (v_alignbyte, as the leaf pass does).  The second load may reach
// up to 15 bytes past the blob's last byte: the slots carry that slack.  An instance that would
// leave [dst, dst + dst_cap) is not copied at all.
__global__ void __launch_bounds__(256) k_rs_gather(const RsInst* inst, uint64_t n, const uint8_t* slots,
                                                   const uint64_t* slot_off, const uint64_t* slot_len,
                                                   const uint64_t* dst_off, const uint64_t* piece0, uint8_t* dst,
                                                   uint64_t dst_cap) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
    const uint64_t waves = (uint64_t)gridDim.x * blockDim.x / 64;
    const uint64_t total = piece0[n];
    for (uint64_t pc = wave; pc < total; pc += waves) {
        // the last instance whose first piece is <= pc (instances without pieces share a prefix value
        // with their successor and are skipped by taking the last)
        uint64_t lo = 0, hi = n;  // piece0[lo] <= pc < piece0[hi]
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) / 2;
            if (piece0[mid] <= pc) lo = mid; else hi = mid;
        }
        const uint64_t i = lo;
        const uint32_t slot = inst[i].slot;
        const uint64_t len = slot_len[slot], d_at = dst_off[i];
        const uint64_t p0 = (pc - piece0[i]) * RS_PIECE;
        if (!inst[i].valid || p0 >= len || d_at > dst_cap || len > dst_cap - d_at) continue;
        const uint64_t nb = len - p0 < RS_PIECE ? len - p0 : RS_PIECE;
        const uint8_t* s = slots + slot_off[slot] + p0;
        uint8_t* d = dst + d_at + p0;
        rs_copy_piece<false>(s, d, nb, lane);
    }
}

void bw::launch_rs_gather(hipStream_t st, const RsInst* inst, uint64_t n, const uint8_t* slots, const uint64_t* slot_off,
                          const uint64_t* slot_len, const uint64_t* dst_off, const uint64_t* piece0, uint8_t* dst,
                          uint64_t dst_cap) {
    if (!n) return;
    // the piece count is on the device; the host knows only its bound (96 pieces per instance)
    const uint64_t blocks = std::min<uint64_t>(2048, (n * (BW_BLOB_MAX_UNCOMPRESSED_SIZE / RS_PIECE) + 3) / 4);
    hipLaunchKernelGGL(k_rs_gather, dim3((uint32_t)blocks), dim3(256), 0, st, inst, n, slots, slot_off, slot_len, dst_off,
                       piece0, dst, dst_cap);
}

// ------------------------------------------------------------------ the session
namespace {
struct HashKey {
    std::array<uint8_t, 32> h;
    bool operator==(const HashKey& o) const { return h == o.h; }
};
struct HashKeyHash {
    size_t operator()(const HashKey& k) const {
        uint64_t v;
        memcpy(&v, k.h.data(), 8);
        return (size_t)v;
    }
};

uint32_t pow2_cap(uint64_t n) {
    uint64_t c = 16;
    while (c < 2 * n) c <<= 1;
    return (uint32_t)c;
}

uint64_t up16(uint64_t v) { return (v + 15) & ~15ull; }
}  // namespace

static int rs_build_table(bw_ctx* c, DevBuf& b, uint32_t cap) {
    if (int rc = ensure(c, b, (size_t)cap * 4)) return rc;
    HIPCHK(c, hipMemsetAsync(b.p, 0xff, (size_t)cap * 4, c->stream));
    return BW_OK;
}

extern "C" int bw_restore_close(bw_restore* s) {
    if (!s) return BW_EINVAL;
    hipSetDevice(s->c->device);
    hipStreamSynchronize(s->c->stream);
    for (DevBuf* b : {&s->ids, &s->items, &s->d_entries, &s->id_tab, &s->item_tab, &s->item_pos, &s->entry_tab, &s->slot_buf,
                      &s->q, &s->tab, &s->run, &s->emit, &s->win, &s->pf_buf, &s->pr_bits, &s->pr_front[0],
                      &s->pr_front[1], &s->pr_ctr, &s->pr_err, &s->pr_stat, &s->pr_tab, &s->pr_hdr, &s->ck_buf, &s->rk_buf})
        free_dev(*b);
    for (auto* walk : {&s->wk, &s->df, &s->pm})
        for (DevBuf& b : *walk) free_dev(b);
    for (DevBuf& b : s->im) free_dev(b);
    for (DevBuf& b : s->rt) free_dev(b);
    for (DevBuf& b : s->fd) free_dev(b);
    delete s;
    return BW_OK;
}

static int rs_open(bw_restore* s, const uint8_t* ids, uint64_t n_pf, const uint8_t* index_items) {
    bw_ctx* c = s->c;
    const uint64_t n_e = s->entries.size(), n_i = s->n_items;
    if (int rc = ensure(c, s->ids, 12 * n_pf + 16)) return rc;
    if (int rc = ensure(c, s->items, BW_INDEX_ENTRY_BYTES * n_i + 16)) return rc;
    if (int rc = ensure(c, s->d_entries, sizeof(bw_unpack_entry) * n_e + 16)) return rc;
    if (int rc = ensure(c, s->item_pos, 4 * n_i + 16)) return rc;
    if (int rc = ensure(c, s->run, 16)) return rc;
    if (int rc = ensure(c, s->slot_buf, (size_t)s->slots * RS_SLOT_STRIDE + 64)) return rc;
    s->id_cap = pow2_cap(n_pf);
    s->item_cap = pow2_cap(n_i);
    s->entry_cap = pow2_cap(n_e);
    if (int rc = rs_build_table(c, s->id_tab, s->id_cap)) return rc;
    if (int rc = rs_build_table(c, s->item_tab, s->item_cap)) return rc;
    if (int rc = rs_build_table(c, s->entry_tab, s->entry_cap)) return rc;
    if (n_pf) HIPCHK(c, hipMemcpyAsync(s->ids.p, ids, 12 * n_pf, hipMemcpyHostToDevice, c->stream));
    if (n_i) HIPCHK(c, hipMemcpyAsync(s->items.p, index_items, BW_INDEX_ENTRY_BYTES * n_i, hipMemcpyHostToDevice, c->stream));
    if (n_e)
        HIPCHK(c, hipMemcpyAsync(s->d_entries.p, s->entries.data(), sizeof(bw_unpack_entry) * n_e, hipMemcpyHostToDevice,
                                 c->stream));
    launch_rs_build_ids(c->stream, P<uint8_t>(s->ids), n_pf, P<uint32_t>(s->id_tab), s->id_cap);
    launch_rs_build_items(c->stream, P<uint8_t>(s->items), n_i, P<uint8_t>(s->ids), P<uint32_t>(s->id_tab), s->id_cap,
                          P<uint32_t>(s->item_pos), P<uint32_t>(s->item_tab), s->item_cap);
    launch_rs_build_entries(c->stream, P<bw_unpack_entry>(s->d_entries), n_e, P<uint32_t>(s->entry_tab), s->entry_cap);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BW_OK;
}

extern "C" int bw_restore_open(bw_ctx* c, const uint8_t prk[32], const uint8_t* d_pf, const bw_packfile* pf,
                               const uint8_t* ids, uint64_t n_pf, const bw_unpack_entry* entries, uint64_t n_entries,
                               const uint8_t* index_items, uint64_t n_items, uint32_t slots, bw_restore** out) {
    if (!c || !prk || !out) return BW_EINVAL;
    *out = nullptr;
    if ((n_pf && (!d_pf || !pf || !ids)) || (n_entries && !entries) || (n_items && !index_items)) return BW_EINVAL;
    if (slots > 65536) {
        c->err = "restore: more than 65,536 decode slots";
        return BW_EINVAL;
    }
    if (n_pf >= RS_EMPTY / 2 || n_entries >= RS_EMPTY / 2 || n_items >= RS_EMPTY / 2) {
        c->err = "restore: more than 2^31 packfiles, entries or index items";
        return BW_EINVAL;
    }
    for (uint64_t i = 0; i < n_entries; i++)
        if (entries[i].packfile >= n_pf) {
            c->err = "restore: entry " + std::to_string(i) + " names a packfile outside the table";
            return BW_EINVAL;
        }
    hipSetDevice(c->device);
    bw_restore* s = new bw_restore;
    s->c = c;
    memcpy(s->prk, prk, 32);
    s->d_pf = d_pf;
    s->pf.assign(pf, pf + n_pf);
    s->entries.assign(entries, entries + n_entries);
    s->n_items = n_items;
    s->slots = slots ? slots : RS_DEFAULT_SLOTS;
    if (int rc = rs_open(s, ids, n_pf, index_items)) {
        bw_restore_close(s);
        return rc;
    }
    *out = s;
    return BW_OK;
}

extern "C" int bw_restore_open_host(bw_ctx* c, const uint8_t prk[32], const uint8_t* data, const bw_packfile* pf,
                                    const uint8_t* ids, uint64_t n_pf, const bw_unpack_entry* entries,
                                    uint64_t n_entries, const uint8_t* index_items, uint64_t n_items, uint32_t slots,
                                    bw_restore** out) {
    if (!c || !prk || !out || (n_pf && (!data || !pf))) return BW_EINVAL;
    hipSetDevice(c->device);
    const uint64_t end = store_extent(pf, n_pf);
    DevBuf buf;
    if (int rc = ensure(c, buf, end + 16)) return rc;
    hipError_t e = end ? hipMemcpy(buf.p, data, end, hipMemcpyHostToDevice) : hipSuccess;
    int rc = e == hipSuccess ? bw_restore_open(c, prk, (const uint8_t*)buf.p, pf, ids, n_pf, entries, n_entries,
                                               index_items, n_items, slots, out)
                             : BW_EHIP;
    if (rc) {
        free_dev(buf);
        return rc;
    }
    (*out)->pf_buf = buf;
    return BW_OK;
}

// ------------------------------------------------------------------ the shared steps
RsLocator bw::rs_locator(const bw_restore* s) {
    const uint32_t item_cap = s->n_items ? s->item_cap : 0, entry_cap = s->entries.empty() ? 0 : s->entry_cap;
    return RsLocator{(const uint8_t*)s->items.p,  (const uint32_t*)s->item_tab.p,  (const uint32_t*)s->item_pos.p,
                     (const bw_unpack_entry*)s->d_entries.p, (const uint32_t*)s->entry_tab.p, item_cap, entry_cap};
}

std::vector<PrPackfile> bw::rs_packfile_table(const bw_restore* s) {
    std::vector<PrPackfile> t(s->pf.size());
    for (size_t p = 0; p < t.size(); p++) t[p] = PrPackfile{s->pf[p].size, s->pf[p].header_len};
    return t;
}

// scratch: [offsets, 8 m | nonces, 12 m]
int bw::rs_fetch_nonces(bw_ctx* c, const uint8_t* d_pf, const uint64_t* n_off, uint64_t m, DevBuf& scratch, uint8_t* out) {
    if (int rc = ensure(c, scratch, 20 * m + 16)) return rc;
    uint8_t* b = P<uint8_t>(scratch);
    if (m) {
        HIPCHK(c, hipMemcpyAsync(b, n_off, 8 * m, hipMemcpyHostToDevice, c->stream));
        launch_gather12(c->stream, d_pf, (const uint64_t*)b, m, b + 8 * m);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(out, b + 8 * m, 12 * m, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BW_OK;
}

// hashes (host, n x 32) -> entry index and status (host)
static int rs_locate(bw_restore* s, const uint8_t* hashes, uint64_t n, uint64_t* idx, uint8_t* st) {
    bw_ctx* c = s->c;
    if (!n) return BW_OK;
    if (int rc = ensure(c, s->q, 41 * n + 16)) return rc;
    uint64_t* d_idx = P<uint64_t>(s->q);
    uint8_t* d_h = P<uint8_t>(s->q) + 8 * n;
    uint8_t* d_st = d_h + 32 * n;
    HIPCHK(c, hipMemcpyAsync(d_h, hashes, 32 * n, hipMemcpyHostToDevice, c->stream));
    launch_rs_locate(c->stream, d_h, n, rs_locator(s), d_idx, d_st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(idx, d_idx, 8 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(st, d_st, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BW_OK;
}

extern "C" int bw_restore_locate(bw_restore* s, const uint8_t* hashes, uint64_t n, uint64_t* entry_idx, uint8_t* status) {
    if (!s || (n && (!hashes || !entry_idx || !status))) return BW_EINVAL;
    hipSetDevice(s->c->device);
    return rs_locate(s, hashes, n, entry_idx, status);
}

int bw::rs_tables(bw_restore* s, uint64_t m, uint64_t ni, RsTables& t) {
    if (int rc = ensure(s->c, s->tab, 24 * m + 24 * ni + 64)) return rc;
    uint64_t* p = P<uint64_t>(s->tab);
    t.slot_len = p;
    t.slot_off = p + m;
    t.map = p + 2 * m;
    t.dst_off = p + 3 * m;
    t.piece0 = t.dst_off + ni;
    t.inst = (RsInst*)(t.piece0 + ni + 1);
    return BW_OK;
}

// m located blobs (entry indices eidx) opened and decoded into the slots at off[k]; sizes on the
// device in t.slot_len, and with the statuses on the host
int bw::rs_decode(bw_restore* s, const std::vector<uint64_t>& eidx, const std::vector<uint64_t>& off, uint32_t flags,
                     const RsTables& t, std::vector<uint64_t>& out_len, std::vector<uint8_t>& st) {
    const uint64_t m = eidx.size();
    out_len.assign(m, 0);
    st.assign(m, 0);
    if (!m) return BW_OK;
    bw_ctx* c = s->c;
    std::vector<bw_unpack_entry> en(m);
    for (uint64_t k = 0; k < m; k++) en[k] = s->entries[eidx[k]];
    HIPCHK(c, hipMemcpyAsync(t.slot_off, off.data(), 8 * m, hipMemcpyHostToDevice, c->stream));
    return unpack_blobs_core(c, s->prk, s->d_pf, s->pf.data(), s->pf.size(), en.data(), m, flags & BW_UNPACK_VERIFY,
                             P<uint8_t>(s->slot_buf), off.data(), out_len.data(), st.data(), t.slot_len, t.map);
}

int bw::rs_tree_decode(bw_restore* s, const std::vector<uint64_t>& eidx, uint32_t flags, uint64_t ni, RsTables& t,
                       std::vector<uint8_t>& bst) {
    const uint64_t m = eidx.size();
    std::vector<uint64_t> off(m), blen;
    for (uint64_t k = 0; k < m; k++) off[k] = k * RS_SLOT_STRIDE;
    if (int rc = rs_tables(s, m, ni, t)) return rc;
    return rs_decode(s, eidx, off, flags, t, blen, bst);
}

int bw::rs_tree_parse(bw_restore* s, const RsTables& t, uint64_t m, std::vector<RsTreeHdr>* hd) {
    bw_ctx* c = s->c;
    if (int rc = ensure(c, s->q, m * sizeof(RsTreeHdr) + 16)) return rc;
    launch_rs_tree_parse(c->stream, P<uint8_t>(s->slot_buf), t.slot_off, t.slot_len, m, P<RsTreeHdr>(s->q));
    if (!hd) return BW_OK;
    HIPCHK(c, hipGetLastError());
    hd->resize(m);
    HIPCHK(c, hipMemcpyAsync(hd->data(), s->q.p, m * sizeof(RsTreeHdr), hipMemcpyDeviceToHost, c->stream));
    return BW_OK;
}

// ------------------------------------------------------------------ the tree walk
namespace {
struct TreeReq {
    std::array<uint8_t, 32> hash;
    uint64_t slot;  // which of the level's chains it continues
};

// The walk's state: the nodes found so far (node i's tree blob has hash node_hash[i]), their packed
// names, the chunk rows of the File nodes, and the level being fetched.
struct TreeWalk {
    bw_restore* s;
    uint32_t flags;
    bw_restore_error* err;
    std::vector<bw_restore_node> N;
    std::vector<std::array<uint8_t, 32>> node_hash;
    std::vector<uint8_t> nm, rows;
    std::vector<uint64_t> level;             // nodes whose trees this level fetches, in node order
    std::vector<std::vector<uint8_t>> kids;  // per node of the level: its chain's children rows, in chain order
};

// What one sub-batch's blobs hold: the parsed headers, and the names and children rows the emit
// kernel packed.  The emit table has two regions per blob, its name and its rows, in three columns.
struct TreeBatch {
    std::vector<RsTreeHdr> hd;
    std::vector<uint64_t> reg;  // src[2m] | len[2m] | dst[2m]
    std::vector<uint8_t> pk;
    uint64_t m = 0;
    static uint64_t name(uint64_t k) { return 2 * k; }
    static uint64_t rows(uint64_t k) { return 2 * k + 1; }
    uint64_t* src() { return reg.data(); }
    uint64_t* len() { return reg.data() + 2 * m; }
    uint64_t* dst() { return reg.data() + 4 * m; }
};

int tw_fail(TreeWalk& w, const uint8_t* h, uint32_t reason, const char* why) {
    memcpy(w.err->hash, h, 32);
    w.err->reason = reason;
    w.s->c->err = std::string("restore: tree blob refused: ") + why;
    return BW_EFORMAT;
}

// m <= slots requests located, opened, decoded and parsed; names (a chain's first piece only) and
// children rows packed by one kernel and brought back
int tw_fetch(TreeWalk& w, const TreeReq* rq, uint64_t m, bool first_piece, TreeBatch& b) {
    bw_restore* s = w.s;
    bw_ctx* c = s->c;
    std::vector<uint8_t> hs(32 * m), lst(m), bst;
    std::vector<uint64_t> eidx(m);
    for (uint64_t k = 0; k < m; k++) memcpy(&hs[32 * k], rq[k].hash.data(), 32);
    if (int rc = rs_locate(s, hs.data(), m, eidx.data(), lst.data())) return rc;
    for (uint64_t k = 0; k < m; k++) {
        if (lst[k]) return tw_fail(w, &hs[32 * k], lst[k], "not found");
        if (s->entries[eidx[k]].kind != BW_BLOB_TREE) return tw_fail(w, &hs[32 * k], BW_RESTORE_ENOTTREE, "not a tree");
    }
    RsTables t;
    if (int rc = rs_tree_decode(s, eidx, w.flags, 5 * m, t, bst)) return rc;  // the instance part holds the emit table
    for (uint64_t k = 0; k < m; k++)
        if (bst[k]) return tw_fail(w, &hs[32 * k], bst[k], "failed to open or decode");
    if (int rc = rs_tree_parse(s, t, m, &b.hd)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.m = m;
    b.reg.assign(6 * m, 0);
    uint64_t packed = 0;
    for (uint64_t k = 0; k < m; k++) {
        const RsTreeHdr& h = b.hd[k];
        if (h.status) return tw_fail(w, &hs[32 * k], h.status, "bincode::deserialize::<Tree> fails");
        // the parser bounded both regions by the blob (<= 3 MiB)
        b.src()[b.name(k)] = k * RS_SLOT_STRIDE + h.name_pos;
        b.len()[b.name(k)] = first_piece ? h.name_len : 0;
        b.dst()[b.name(k)] = packed;
        packed += b.len()[b.name(k)];
        b.src()[b.rows(k)] = k * RS_SLOT_STRIDE + h.ch_pos;
        b.len()[b.rows(k)] = 32 * h.n_children;
        b.dst()[b.rows(k)] = packed;
        packed += 32 * h.n_children;
    }
    b.pk.resize(packed);
    if (!packed) return BW_OK;
    if (int rc = ensure(c, s->emit, packed + 16)) return rc;
    uint64_t* d_reg = t.dst_off;  // 6m of the 10m + 1 words behind the slot tables
    HIPCHK(c, hipMemcpyAsync(d_reg, b.reg.data(), 48 * m, hipMemcpyHostToDevice, c->stream));
    launch_rs_tree_emit(c->stream, P<uint8_t>(s->slot_buf), d_reg, d_reg + 2 * m, d_reg + 4 * m, 2 * m, P<uint8_t>(s->emit));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(b.pk.data(), s->emit.p, packed, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BW_OK;
}

// a sub-batch's blobs into the walk: a chain's first piece describes its node, every piece adds
// children, and the next round follows every next_sibling
void tw_append(TreeWalk& w, const TreeReq* rq, bool first_piece, TreeBatch& b, std::vector<TreeReq>& next) {
    for (uint64_t k = 0; k < b.m; k++) {
        const RsTreeHdr& h = b.hd[k];
        const uint64_t j = rq[k].slot;
        if (first_piece) {
            bw_restore_node& nd = w.N[w.level[j]];
            nd.kind = h.kind;
            nd.flags = h.flags;
            nd.size = h.size;
            nd.mtime = h.mtime;
            nd.ctime = h.ctime;
            nd.name_off = w.nm.size();
            nd.name_len = h.name_len;
            const uint8_t* n0 = b.pk.data() + b.dst()[b.name(k)];
            w.nm.insert(w.nm.end(), n0, n0 + h.name_len);
        }
        const uint8_t* r0 = b.pk.data() + b.dst()[b.rows(k)];
        w.kids[j].insert(w.kids[j].end(), r0, r0 + 32 * h.n_children);
        if (h.has_next) {
            TreeReq rq_next;
            memcpy(rq_next.hash.data(), h.next, 32);
            rq_next.slot = j;
            next.push_back(rq_next);
        }
    }
}

// one level: round r fetches piece r of every sibling chain that has one, `slots` blobs at a time
int tw_level(TreeWalk& w) {
    const uint64_t slots = w.s->slots, max_pieces = w.s->entries.size();
    w.kids.assign(w.level.size(), std::vector<uint8_t>());
    std::vector<TreeReq> cur(w.level.size()), next;
    for (uint64_t j = 0; j < w.level.size(); j++) cur[j] = TreeReq{w.node_hash[w.level[j]], j};
    TreeBatch b;
    for (uint64_t round = 0; !cur.empty(); round++) {
        if (round > max_pieces) return tw_fail(w, cur[0].hash.data(), BW_RESTORE_EFORMAT, "a sibling chain longer than the store");
        next.clear();
        for (uint64_t lo = 0; lo < cur.size(); lo += slots) {
            const uint64_t m = std::min<uint64_t>(slots, cur.size() - lo);
            if (int rc = tw_fetch(w, &cur[lo], m, round == 0, b)) return rc;
            tw_append(w, &cur[lo], round == 0, b, next);
        }
        cur.swap(next);
    }
    return BW_OK;
}

// the next level: the children of every Dir node, parents in node order; a File node's rows are its chunks
int tw_close_level(TreeWalk& w) {
    const uint64_t hard_cap = 1ull << 32;  // a walk that grows past this is reported as it stands
    std::vector<uint64_t> nl;
    for (uint64_t j = 0; j < w.level.size(); j++) {
        const uint64_t p = w.level[j], nch = w.kids[j].size() / 32;
        w.N[p].n_children = nch;
        if (w.N[p].kind == BW_TREE_FILE) {
            w.N[p].child_first = w.rows.size() / 32;
            w.rows.insert(w.rows.end(), w.kids[j].begin(), w.kids[j].end());
            continue;
        }
        w.N[p].child_first = w.N.size();
        for (uint64_t k = 0; k < nch; k++) {
            std::array<uint8_t, 32> h;
            memcpy(h.data(), &w.kids[j][32 * k], 32);
            // a tree that is its own ancestor never ends (the reference's queue never drains)
            for (uint64_t a = p; a != ~0ull; a = w.N[a].parent)
                if (w.node_hash[a] == h) return tw_fail(w, h.data(), BW_RESTORE_EFORMAT, "a directory that contains itself");
            bw_restore_node nd;
            memset(&nd, 0, sizeof(nd));
            nd.parent = p;
            nl.push_back(w.N.size());
            w.N.push_back(nd);
            w.node_hash.push_back(h);
        }
        if (w.N.size() > hard_cap || w.rows.size() / 32 > hard_cap) {
            nl.clear();
            break;
        }
    }
    w.level.swap(nl);
    return BW_OK;
}
}  // namespace

extern "C" int bw_restore_trees(bw_restore* s, const uint8_t root_hash[32], uint32_t flags, bw_restore_node* nodes,
                                uint64_t node_cap, uint8_t* names, uint64_t names_cap, uint8_t* chunks,
                                uint64_t chunks_cap, bw_restore_counts* counts, bw_restore_error* err) {
    if (!s || !root_hash || !counts || !err || (flags & ~BW_UNPACK_VERIFY)) return BW_EINVAL;
    if ((node_cap && !nodes) || (names_cap && !names) || (chunks_cap && !chunks)) return BW_EINVAL;
    hipSetDevice(s->c->device);
    memset(counts, 0, sizeof(*counts));
    memset(err, 0, sizeof(*err));
    TreeWalk w;
    w.s = s;
    w.flags = flags;
    w.err = err;
    w.N.resize(1);
    w.node_hash.resize(1);
    memset(&w.N[0], 0, sizeof(w.N[0]));
    w.N[0].parent = ~0ull;
    memcpy(w.node_hash[0].data(), root_hash, 32);
    w.level.assign(1, 0);
    while (!w.level.empty()) {
        if (int rc = tw_level(w)) return rc;
        if (int rc = tw_close_level(w)) return rc;
    }
    counts->n_nodes = w.N.size();
    counts->name_bytes = w.nm.size();
    counts->n_chunks = w.rows.size() / 32;
    if (w.N.size() > node_cap || w.nm.size() > names_cap || w.rows.size() / 32 > chunks_cap) return BW_ENOSPC;
    memcpy(nodes, w.N.data(), w.N.size() * sizeof(bw_restore_node));
    if (!w.nm.empty()) memcpy(names, w.nm.data(), w.nm.size());
    if (!w.rows.empty()) memcpy(chunks, w.rows.data(), w.rows.size());
    return BW_OK;
}

// ------------------------------------------------------------------ file assembly
extern "C" int bw_restore_files_device(bw_restore* s, const uint8_t* chunks, const uint64_t* file_first, uint64_t n_files,
                                       uint32_t flags, uint8_t* d_dst, uint64_t dst_cap, uint64_t* file_off,
                                       uint64_t* file_len, uint8_t* file_status, uint64_t* file_bad_child,
                                       uint64_t* n_done) {
    if (!s || !n_done || (flags & ~(BW_UNPACK_VERIFY | BW_RESTORE_SKEW_SLOTS))) return BW_EINVAL;
    *n_done = 0;
    if (n_files && (!file_first || !file_off || !file_len || !file_status || !file_bad_child)) return BW_EINVAL;
    if (!n_files) return BW_OK;
    bw_ctx* c = s->c;
    for (uint64_t f = 0; f < n_files; f++)
        if (file_first[f] > file_first[f + 1]) {
            c->err = "restore: file_first must not decrease";
            return BW_EINVAL;
        }
    const uint64_t first = file_first[0], n_rows = file_first[n_files];
    if ((n_rows > first && !chunks) || (dst_cap && !d_dst)) return BW_EINVAL;
    hipSetDevice(c->device);
    for (uint64_t f = 0; f < n_files; f++) {
        file_off[f] = file_len[f] = 0;
        file_status[f] = BW_RESTORE_OK;
        file_bad_child[f] = ~0ull;
    }
    HIPCHK(c, hipMemsetAsync(s->run.p, 0, 8, c->stream));

    uint64_t f = 0;        // the file of row `row`
    uint64_t row = first;  // the next row to take
    uint64_t out = 0;      // bytes placed so far: the host's copy of the device's running offset
    uint64_t seq = 0;      // distinct blobs decoded so far (the skew hook counts them)
    bool full = false;     // the window cannot take file `stop`
    uint64_t stop = n_files;
    auto enter = [&]() {  // f moves on to the file that holds `row`; files passed over start here
        while (f < n_files && row >= file_first[f + 1]) {
            f++;
            if (f < n_files) file_off[f] = out;
        }
    };
    file_off[0] = 0;
    enter();
    while (row < n_rows && !full) {
        // a sub-batch: rows in order until it would hold more than `slots` distinct blobs
        std::unordered_map<HashKey, uint32_t, HashKeyHash> seen;
        std::vector<uint8_t> hs;          // distinct hashes
        std::vector<uint64_t> irow;       // per instance: its row
        std::vector<uint32_t> iblob;      // per instance: its distinct blob
        uint64_t r = row, fr = f;
        for (; r < n_rows && irow.size() < RS_MAX_INSTANCES; r++) {
            while (r >= file_first[fr + 1]) fr++;
            if (file_status[fr]) continue;  // the file failed in an earlier sub-batch: the rest of it is dropped
            HashKey k;
            memcpy(k.h.data(), chunks + 32 * r, 32);
            auto it = seen.find(k);
            if (it == seen.end()) {
                if (seen.size() == s->slots) break;
                it = seen.emplace(k, (uint32_t)seen.size()).first;
                hs.insert(hs.end(), k.h.begin(), k.h.end());
            }
            irow.push_back(r);
            iblob.push_back(it->second);
        }
        const uint64_t nd = seen.size(), ni = irow.size();
        // 1. locate; the located blobs take the slots
        std::vector<uint64_t> eidx(nd);
        std::vector<uint8_t> bst(nd);
        if (int rc = rs_locate(s, hs.data(), nd, eidx.data(), bst.data())) return rc;
        std::vector<uint64_t> sl_e, sl_off, blen(nd, 0);
        std::vector<uint32_t> slot_of(nd, 0);
        for (uint64_t j = 0; j < nd; j++) {
            if (bst[j]) continue;
            slot_of[j] = (uint32_t)sl_e.size();
            sl_off.push_back(sl_e.size() * RS_SLOT_STRIDE + ((flags & BW_RESTORE_SKEW_SLOTS) ? ((seq + j) & 15) : 0));
            sl_e.push_back(eidx[j]);
        }
        seq += nd;
        // 2. open and decode
        RsTables t;
        if (int rc = rs_tables(s, std::max<uint64_t>(sl_e.size(), 1), ni, t)) return rc;
        std::vector<uint64_t> sl_len;
        std::vector<uint8_t> sl_st;
        if (int rc = rs_decode(s, sl_e, sl_off, flags, t, sl_len, sl_st)) return rc;
        for (uint64_t j = 0; j < nd; j++)
            if (!bst[j]) {
                bst[j] = sl_st[slot_of[j]];
                blen[j] = bst[j] ? 0 : sl_len[slot_of[j]];
            }
        // which instances are written: a file ends at its first failing child; the window ends the call
        std::vector<RsInst> inst(ni);
        for (uint64_t i = 0; i < ni; i++) {
            row = irow[i];
            enter();
            const uint32_t j = iblob[i];
            inst[i] = RsInst{slot_of[j], 0};
            if (full) {
                if (f == stop && !bst[j]) file_len[f] += blen[j];  // its size as far as this sub-batch shows it
                continue;
            }
            if (file_status[f]) continue;
            if (bst[j]) {
                file_status[f] = bst[j];
                file_bad_child[f] = row - file_first[f];
                continue;
            }
            if (blen[j] > dst_cap - out || out > dst_cap) {
                full = true;
                stop = f;
                file_len[f] += blen[j];
                continue;
            }
            inst[i].valid = 1;
            file_len[f] += blen[j];
            out += blen[j];
        }
        if (!full) {
            row = r;
            enter();
        }
        // 3. the instances' places: a scan on the device, from the device's sizes; 4. the gather
        if (ni) {
            HIPCHK(c, hipMemcpyAsync(t.inst, inst.data(), ni * sizeof(RsInst), hipMemcpyHostToDevice, c->stream));
            launch_rs_scan(c->stream, t.inst, ni, t.slot_len, P<uint64_t>(s->run), t.dst_off, t.piece0);
            launch_rs_gather(c->stream, t.inst, ni, P<uint8_t>(s->slot_buf), t.slot_off, t.slot_len, t.dst_off, t.piece0,
                             d_dst, dst_cap);
            HIPCHK(c, hipGetLastError());
            // the tables and the slots are reused by the next sub-batch, on the same stream
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (full) {
        *n_done = stop;
        c->err = "restore: file " + std::to_string(stop) + " does not fit the window";
        return BW_ENOSPC;
    }
    *n_done = n_files;
    return BW_OK;
}

extern "C" int bw_restore_files(bw_restore* s, const uint8_t* chunks, const uint64_t* file_first, uint64_t n_files,
                                uint32_t flags, uint8_t* dst, uint64_t dst_cap, uint64_t* file_off, uint64_t* file_len,
                                uint8_t* file_status, uint64_t* file_bad_child, uint64_t* n_done) {
    if (!s || !n_done || (dst_cap && !dst)) return BW_EINVAL;
    bw_ctx* c = s->c;
    hipSetDevice(c->device);
    if (int rc = ensure(c, s->win, dst_cap + 16)) return rc;
    const int rc = bw_restore_files_device(s, chunks, file_first, n_files, flags, P<uint8_t>(s->win), dst_cap, file_off,
                                           file_len, file_status, file_bad_child, n_done);
    if (rc != BW_OK && rc != BW_ENOSPC) return rc;
    // the whole files lie back to back from 0
    const uint64_t end = *n_done ? file_off[*n_done - 1] + file_len[*n_done - 1] : 0;
    if (end) HIPCHK(c, hipMemcpy(dst, s->win.p, end, hipMemcpyDeviceToHost));
    return rc;
}
