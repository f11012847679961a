// bw_prune.h -- private declarations of prune (bw_prune.hip): the mark bits, the device records of
// the walk and of the repack.  Off the chunk -> hash -> dedup path (backuwup_amd/build.py OFF_PATH),
// like bw_restore.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/backuwup_gpu.h"
#include "bw_restore.h"

namespace bw {

// One byte of mark bits per entry, four entries to the u32 word the atomic OR works on.
constexpr uint32_t PR_LIVE = 1;    // a kept root reaches the entry
constexpr uint32_t PR_QUEUED = 2;  // a tree reference reached it: it is, or was, on a frontier
constexpr uint32_t PR_EXPAND_Y = 4;  // workgroups that share one tree blob's references
constexpr uint64_t PR_ERR_DEVICE = 65536;  // records of the device error list of a first walk (5 MiB)

// counters of a walk
enum { PR_C_NEXT = 0, PR_C_ERRORS = 1, PR_C_EXPANDED = 2, PR_C_COUNT = 4 };

// The walk's device state as the kernels take it.
struct PrWalk {
    RsLocator loc;
    const PrPackfile* pf;
    uint32_t* bits;
    uint64_t* next;  // the next frontier: entry indices
    uint64_t* ctr;   // PR_C_*
    bw_prune_error* errs;
    uint64_t err_cap;
};

// every root marked and, when it names a tree entry, queued
void launch_prune_roots(hipStream_t st, const PrWalk& w, const uint8_t* roots, uint64_t n);
// the m parsed tree blobs of a sub-batch (entry front[b], decoded at slots + off[b], header hdr[b],
// chain status cst[b]): every children row and next_sibling marked, tree references queued
void launch_prune_expand(hipStream_t st, const PrWalk& w, const uint64_t* front, const uint8_t* slots, const uint64_t* off,
                         const RsTreeHdr* hdr, const uint32_t* cst, uint64_t m);
// live[e] = the live bit; stats[4 p ..] = {live blobs, live bytes, blobs, bytes} of packfile p (zeroed by the caller)
void launch_prune_account(hipStream_t st, const bw_unpack_entry* entries, uint64_t n, const uint32_t* bits, uint8_t* live,
                          uint64_t* stats);
// bw_pack.hip: header entry i (entries[order[i]] with offset sect[i]) in bincode varint form at hdr + hoff[i]
void launch_pack_meta_sealed(hipStream_t st, const bw_unpack_entry* entries, const uint64_t* order, const uint64_t* sect,
                       const uint64_t* hoff, uint64_t n, uint8_t* hdr);
// blob i: len[i] bytes from pf + src[i] to out + dst[i]; piece0 = the prefix of their piece counts (n + 1)
void launch_prune_move(hipStream_t st, const uint8_t* pf, const uint64_t* src, const uint64_t* dst, const uint64_t* len,
                       const uint64_t* piece0, uint64_t n, uint64_t total_pieces, uint8_t* out);

}  // namespace bw
