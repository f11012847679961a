// bw_parent.h -- private declarations of the parent match (bw_parent.hip): the device records of a
// level (references, items, parent children, the per-blob take table) and the walk's state as the
// kernels take it.  Off the chunk -> hash -> dedup path (backuwup_amd/build.py OFF_PATH), like bw_diff.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/backuwup_gpu.h"
#include "../../include/backuwup_gpu_pack.h"
#include "bw_restore.h"
#include "bw_parent_host.h"

namespace bw {

constexpr uint64_t PM_NONE = ~0ull;

// counters of a walk
enum { PM_C_ERRORS = 0, PM_C_NEXT = 1, PM_C_UNCHANGED = 2, PM_C_BYTES = 3, PM_C_COUNT = 4 };

// the session's buffers (bw_restore::pm)
enum {
    PM_B_CTR, PM_B_READ, PM_B_ERR, PM_B_SCAN, PM_B_SNAMES, PM_B_RES, PM_B_ITEMS, PM_B_REFS, PM_B_CHAIN0,
    PM_B_CHAIN1, PM_B_OUT, PM_B_TAKE, PM_B_STAGE, PM_B_SEGHASH, PM_B_LVL, PM_B_CHILD, PM_B_CREFS, PM_B_NAMES, PM_B_TAB,
    PM_B_MATCH, PM_B_COUNT
};
static_assert(PM_B_COUNT <= sizeof(bw_restore::pm) / sizeof(DevBuf), "bw_restore::pm holds every buffer");

// One tree reference to resolve: an item's first piece, the next_sibling of the piece `by`, or a
// parent child's first piece.
struct PmRef {
    uint8_t hash[32];
    uint8_t by[32];   // the piece that names it, zero for the root
    uint64_t by_pos;  // its position there, ~0 for a next_sibling, 0 for the root
    uint32_t owner, pad;  // the item (a chain piece) or the child (a first piece) it is read for
};

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

// What the host tells k_pm_take about blob b of a sub-batch.
struct PmTake {
    uint32_t ref, cst;  // the reference it answers; the unpack chain's status
    uint64_t stage;     // where its children rows go in the staging arena (rows)
    uint64_t n_rows;    // how many are taken (0 for a child's first piece)
    uint64_t name_off;  // where its name goes (a child's first piece)
    uint64_t next;      // its next_sibling's place among the next round's references, or ~0
    uint64_t seg;       // its segment, or ~0 when it has no rows
};

// The walk's device state as the kernels take it.
struct PmWalk {
    RsLocator loc;
    const bw_restore_node* scan;  // the caller's scan
    const uint8_t* scan_names;
    bw_parent_result* res;        // one per scan node
    uint8_t* read;                // one byte per session entry
    uint64_t* ctr;                // PM_C_*
    bw_prune_error* errs;
    uint64_t err_cap;
    uint8_t* stage;     // children rows in the order they were fetched
    uint8_t* seg_hash;  // per fetched segment: the hash of the piece that holds it
    // the level's lists, once every chain has ended: segments sorted by (item, piece)
    const uint64_t *seg_row0, *seg_stage;  // a segment's first row in the lists, and in `stage`
    const uint32_t *seg_node, *seg_sid;    // its item, and its number in fetch order
    const uint64_t* node_row0;             // an item's first row
    const uint64_t *probe_row0, *item_first;  // an item's first probe, and its scan Dir's first child
    PmChild* child;  // the level's parent children: the lists, item after item
    uint8_t* names;  // their names
    uint64_t n_seg, n_child, n_items, n_probes;
    uint32_t root;   // level 0: the roots pair whatever their names
    uint64_t trust_before;
};

}  // namespace bw
