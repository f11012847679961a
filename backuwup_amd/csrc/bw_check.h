// bw_check.h -- private declarations of check (bw_check.hip): the per-packfile sums as the kernels
// keep them and the launches.  Off the chunk -> hash -> dedup path (backuwup_amd/build.py OFF_PATH),
// like bw_prune.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/backuwup_gpu.h"
#include "bw_restore.h"
#include "bw_prune.h"

namespace bw {

constexpr uint32_t CK_SCAN = 1024;  // entries per workgroup of the segmented scan
// u64 sums per packfile: entries, the four flags, claimed bytes
enum { CK_S_ENTRIES = 0, CK_S_RANGE, CK_S_ORDER, CK_S_UNINDEXED, CK_S_SHADOWED, CK_S_CLAIMED, CK_S_COUNT };

// Segmented exclusive sum of 12 + length (segments: runs of equal entries[].packfile).  Step 1, one
// workgroup per CK_SCAN entries: excl[e] = the sum over the earlier entries of e's packfile inside the
// workgroup's range, open[e] = 1 when that packfile began before the range; blk_sum[b] / blk_head[b]
// = the sum behind the range's last segment start, and whether it has one.  Step 2, one workgroup:
// carry[b] = what the ranges before b add to b's open entries.
void launch_check_scan(hipStream_t st, const bw_unpack_entry* entries, uint64_t n, uint64_t* excl, uint8_t* open,
                       uint64_t* blk_sum, uint32_t* blk_head, uint64_t* carry);
// one lane per item: status[i] = ENOPACKFILE / EMISMATCH, or OK with owner[entry] = min(owner[entry], i)
void launch_check_items(hipStream_t st, const RsLocator& loc, uint64_t n_items, uint32_t* owner, uint8_t* status);
// one lane per item: an OK item that does not own its entry is a duplicate
void launch_check_item_dups(hipStream_t st, const RsLocator& loc, uint64_t n_items, const uint32_t* owner, uint8_t* status);
// one lane per entry: the four flags and the per-packfile sums (sums zeroed by the caller)
void launch_check_entries(hipStream_t st, const RsLocator& loc, uint64_t n, const PrPackfile* pf, const uint64_t* excl,
                          const uint8_t* open, const uint64_t* carry, const uint32_t* owner, uint8_t* flags, uint64_t* sums);

}  // namespace bw
