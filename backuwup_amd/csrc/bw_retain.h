// bw_retain.h -- private declarations of retain (bw_retain.hip): the session's buffers and the state of
// the mark as the kernels take it.  The walk, its bits and its edge lists are impact's (bw_impact.h,
// im_walk<RtReach>).  Off the chunk -> hash -> dedup path (backuwup_amd/build.py OFF_PATH).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/backuwup_gpu.h"
#include "bw_impact.h"
#include "bw_retain_host.h"

namespace bw {

// the session's buffers (bw_restore::rt)
enum {
    RT_B_LEAF,   // the edges that pass nothing on
    RT_B_REACH,  // n_e x W words: which roots reach the entry (the public masks)
    RT_B_OPEN,   // n_e x W words: which roots open it
    RT_B_ROOT,   // bw_retain_root per root, then the four totals
    RT_B_DMG,    // one byte per entry
    RT_B_MASK,   // the drop: the caller's masks, then the drop sets
    RT_B_LIVE,   // the drop: live bytes of one batch of sets
    RT_B_STAT,   // the drop: per-packfile sums, then bw_retain_freed, of one batch of sets
    RT_B_COUNT
};
static_assert(RT_B_COUNT <= sizeof(bw_restore::rt) / sizeof(DevBuf), "bw_restore::rt holds every buffer");

constexpr uint32_t RT_SUMS = 5;  // the u64 sums at the head of bw_retain_root
enum { RT_T_REACHED_BLOBS, RT_T_REACHED_BYTES, RT_T_ORPHAN_BLOBS, RT_T_ORPHAN_BYTES, RT_T_COUNT };
constexpr uint64_t RT_DROP_BATCH_BYTES = 1ull << 28;  // live bytes on the device per batch of drop sets
constexpr uint64_t RT_DROP_BATCH_SETS = 65535;        // a grid's y

}  // namespace bw
