// bw_diff.h -- private declarations of the diff walk (bw_diff.hip): the nodes of a level and the walk's
// state as the kernels take it.  References, the take table and the fetch's state are bw_walk.h's, shared
// with the parent match.  Off the chunk -> hash -> dedup path (backuwup_amd/build.py OFF_PATH), like bw_prune.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/backuwup_gpu.h"
#include "bw_walk.h"
#include "bw_diff_host.h"

namespace bw {

constexpr uint32_t DF_OK = 1;      // the node's first piece was read and parsed
constexpr uint32_t DF_CYCLIC = 2;  // its hash is one of its ancestors' on its side: its list counts as empty
constexpr uint32_t DF_TRUNC = 4;   // a later piece of its chain could not be read
constexpr uint64_t DF_NONE = ~0ull;

// the walk's counters behind WK_C_ERRORS
enum { DF_C_RECORDS = 1, DF_C_NEXT = 2 };
static_assert(DF_C_NEXT < WK_C_COUNT, "the counters fit the fetch's buffer");

// the session's buffers (bw_restore::df): a level's nodes and references (this level, the next), tables and records
enum { DF_B_NODES0, DF_B_NODES1, DF_B_REFS0, DF_B_REFS1, DF_B_LVL, DF_B_ROWS, DF_B_ROWSEG, DF_B_TAB, DF_B_RTAB, DF_B_REC, DF_B_COUNT };
static_assert(DF_B_COUNT <= sizeof(bw_restore::df) / sizeof(DevBuf), "bw_restore::df holds every buffer");

// One side of an item of the level: an unmatched child (or a root) whose first piece is asked for.
struct DfNode {
    uint8_t hash[32];
    uint64_t parent;  // the parent item's record, ~0 for a root
    uint64_t pos;     // its position in the parent's list on its side
    uint32_t side, state;
    uint32_t kind, tflags;
    uint64_t size, mtime, ctime;
    uint64_t name_off, name_len;  // in the walk's name arena
    uint64_t rec;                 // the record it belongs to (k_df_pair)
    uint32_t partner;             // the node of the other side it pairs with, or RS_EMPTY
    uint32_t slot;                // its place in the name table (k_df_join)
};

// The walk's device state as the kernels take it.
struct DfWalk {
    WkFetch f;                // the shared fetch; f.names holds every name so far
    DfNode* nodes;            // the level's nodes
    bw_diff_record* recs;     // every record so far
    uint64_t* ctr;            // WK_C_ERRORS, DF_C_*
    const uint64_t *node_row0, *node_rows;
    uint8_t* rows;      // the lists, node after node
    uint32_t* row_seg;  // per row: its segment
    uint64_t n_rows, n_nodes, level;
};

}  // namespace bw
