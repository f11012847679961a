// bw_diff.h -- private declarations of the diff walk (bw_diff.hip): the device records of a level
// (references, nodes, the per-blob take table) and the walk's state as the kernels take it.  Off the
// chunk -> hash -> dedup path (backuwup_amd/build.py OFF_PATH), like bw_prune.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/backuwup_gpu.h"
#include "bw_restore.h"
#include "bw_diff_host.h"

namespace bw {

constexpr uint32_t DF_OK = 1;      // the node's first piece was read and parsed
constexpr uint32_t DF_CYCLIC = 2;  // its hash is one of its ancestors' on its side: its list counts as empty
constexpr uint32_t DF_TRUNC = 4;   // a later piece of its chain could not be read
constexpr uint64_t DF_NONE = ~0ull;

// counters of a walk
enum { DF_C_ERRORS = 0, DF_C_RECORDS = 1, DF_C_NEXT = 2, DF_C_COUNT = 4 };

// One tree reference to resolve: a node's first piece (round 0) or the next_sibling of the piece `by`.
struct DfRef {
    uint8_t hash[32];
    uint8_t by[32];   // the piece that names it, zero for a root
    uint64_t by_pos;  // its position there, ~0 for a next_sibling, 0 / 1 for root A / B
    uint32_t node, pad;
};

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

// What the host tells k_df_take about blob b of a sub-batch.
struct DfTake {
    uint32_t ref, cst;  // the reference it answers; the unpack chain's status
    uint64_t stage;     // where its children rows go in the staging arena (rows)
    uint64_t n_rows;    // how many are taken (0 for a cyclic node)
    uint64_t name_off;  // where its name goes (round 0)
    uint64_t next;      // its next_sibling's place among the next round's references, or ~0
    uint64_t seg;       // its segment, or ~0 when it has no rows
};

// The walk's device state as the kernels take it.
struct DfWalk {
    RsLocator loc;
    DfNode* nodes;            // the level's nodes
    bw_diff_record* recs;     // every record so far
    uint8_t* names;           // every name so far
    uint8_t* read;            // one byte per session entry
    uint64_t* ctr;            // DF_C_*
    bw_prune_error* errs;
    uint64_t err_cap;
    uint8_t* stage;           // children rows in the order they were fetched
    uint8_t* seg_hash;        // per fetched segment: the hash of the piece that holds it
    // the level's lists, once every chain has ended: segments sorted by (node, piece)
    const uint64_t *seg_row0, *seg_stage;  // a segment's first row in `rows`, and in `stage`
    const uint32_t *seg_node, *seg_sid;    // its node, and its number in fetch order
    const uint64_t *node_row0, *node_rows;
    uint8_t* rows;      // the lists, node after node
    uint32_t* row_seg;  // per row: its segment
    uint64_t n_seg, n_rows, n_nodes, level;
};

}  // namespace bw
