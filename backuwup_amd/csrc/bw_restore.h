// bw_restore.h -- private declarations of the restore session (bw_restore.hip): the locator's
// tables, the tree parser's records and the gather's instance tables.  Off the chunk -> hash ->
// dedup path (backuwup_amd/build.py OFF_PATH), like bw_unpack.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/backuwup_gpu.h"

namespace bw {

constexpr uint32_t RS_EMPTY = 0xffffffffu;            // a free table slot (tables hold u32 record indices)
constexpr uint64_t RS_SLOT_STRIDE = BW_BLOB_MAX_UNCOMPRESSED_SIZE + 32;  // a decode slot plus skew and load slack
constexpr uint32_t RS_PIECE = 32768;                  // bytes of one instance a wave copies
constexpr uint32_t RS_DEFAULT_SLOTS = 1024;           // 3 GiB of decode room
constexpr uint64_t RS_MAX_INSTANCES = 1u << 20;       // instances of one sub-batch (bounds the tables)

// What the tree parser reports for one blob (bincode::deserialize::<Tree>, trailing bytes allowed).
struct RsTreeHdr {
    uint32_t status;  // 0, or BW_RESTORE_EFORMAT
    uint32_t kind, flags, has_next;
    uint64_t size, mtime, ctime;
    uint64_t name_pos, name_len;  // the name's bytes inside the blob
    uint64_t ch_pos, n_children;  // the children's 32-byte rows inside the blob
    uint8_t next[32];
};

// One instance of a sub-batch: the blob in decode slot `slot` is the next piece of the output
// (valid = 0: the instance is dropped, its file failed earlier or the window is full).
struct RsInst {
    uint32_t slot, valid;
};

// the three tables; cap_* are powers of two
void launch_rs_build_ids(hipStream_t st, const uint8_t* ids, uint64_t n_pf, uint32_t* tab, uint32_t cap);
void launch_rs_build_items(hipStream_t st, const uint8_t* items, uint64_t n_items, const uint8_t* ids,
                           const uint32_t* id_tab, uint32_t id_cap, uint32_t* item_pos, uint32_t* tab, uint32_t cap);
void launch_rs_build_entries(hipStream_t st, const bw_unpack_entry* entries, uint64_t n, uint32_t* tab, uint32_t cap);
void launch_rs_locate(hipStream_t st, const uint8_t* hashes, uint64_t n, const uint8_t* items, const uint32_t* item_tab,
                      uint32_t item_cap, const uint32_t* item_pos, const bw_unpack_entry* entries,
                      const uint32_t* entry_tab, uint32_t entry_cap, uint64_t* entry_idx, uint8_t* status);
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

}  // namespace bw
