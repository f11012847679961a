// bw_parent.h -- private declarations of the parent match (bw_parent.hip): the items and parent children
// of a level and the walk's state as the kernels take it.  References, the take table and the fetch's
// state are bw_walk.h's, shared with the diff walk.  Off the chunk -> hash -> dedup path
// (backuwup_amd/build.py OFF_PATH), like bw_diff.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/backuwup_gpu.h"
#include "../../include/backuwup_gpu_pack.h"
#include "bw_walk.h"
#include "bw_parent_host.h"

namespace bw {

// the walk's counters behind WK_C_ERRORS
enum { PM_C_NEXT = 1, PM_C_UNCHANGED = 2, PM_C_BYTES = 3 };
static_assert(PM_C_BYTES < WK_C_COUNT, "the counters fit the fetch's buffer");

// the session's buffers (bw_restore::pm)
enum { PM_B_SCAN, PM_B_SNAMES, PM_B_RES, PM_B_ITEMS, PM_B_REFS, PM_B_LVL, PM_B_CHILD, PM_B_CREFS, PM_B_TAB, PM_B_MATCH, PM_B_COUNT };
static_assert(PM_B_COUNT <= sizeof(bw_restore::pm) / sizeof(DevBuf), "bw_restore::pm holds every buffer");

// A Dir against Dir pair: the scan Dir and the parent snapshot's hash for it.
struct PmItem {
    uint8_t hash[32];
    uint32_t scan, pad;
};

// One row of an item's list in the parent snapshot, and what its first piece said.
struct PmChild {
    uint8_t hash[32];
    uint32_t item, ok;  // ok: the first piece was read and parsed
    uint32_t kind, tflags;
    uint64_t pos;  // its position in the item's list
    uint64_t size, mtime, ctime;
    uint64_t name_off, name_len;  // in the level's name arena
};

// The walk's device state as the kernels take it.
struct PmWalk {
    WkFetch f;                    // the shared fetch; f.names holds the level's parent children's names
    const bw_restore_node* scan;  // the caller's scan
    const uint8_t* scan_names;
    bw_parent_result* res;        // one per scan node
    uint64_t* ctr;                // WK_C_ERRORS, PM_C_*
    const uint64_t* node_row0;                // an item's first row
    const uint64_t *probe_row0, *item_first;  // an item's first probe, and its scan Dir's first child
    PmChild* child;  // the level's parent children: the lists, item after item
    uint64_t n_child, n_items, n_probes;
    uint32_t root;   // level 0: the roots pair whatever their names
    uint64_t trust_before;
};

}  // namespace bw
