// bw_impact.h -- private declarations of impact (bw_impact.hip): the mark's bits and device state, the
// items of the report walk and its state as the kernels take it.  References, the take table and the
// fetch's state are bw_walk.h's, shared with the diff walk and the parent match.  Off the chunk -> hash
// -> dedup path (backuwup_amd/build.py OFF_PATH), like bw_prune.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/backuwup_gpu.h"
#include "bw_walk.h"
#include "bw_impact_host.h"

namespace bw {

// One byte of bits per entry, four entries to the u32 word the atomic OR works on (prune's layout):
// the two public taint bits, then the walk's own.
constexpr uint32_t IM_REACHED = 4;  // a root reaches the entry
constexpr uint32_t IM_QUEUED = 8;   // a tree reference reached it and it may be opened: it is, or was, on a frontier
constexpr uint32_t IM_EXPAND_Y = 4;  // workgroups that share one tree blob's references
constexpr uint64_t IM_ERR_DEVICE = 65536;  // records of the device error list of a first walk
constexpr uint64_t IM_MAX_ROWS = 1ull << 30;  // the report walk indexes a level in 32 bits

// counters of the mark
enum { IM_C_NEXT = 0, IM_C_ERRORS = 1, IM_C_EXPANDED = 2, IM_C_EDGES = 3, IM_C_CHANGED = 4, IM_C_DROPPED = 5, IM_C_LEAF = 6, IM_C_COUNT = 8 };
// the report walk's counter behind WK_C_ERRORS
enum { IM_C_ITEMS = 1 };
static_assert(IM_C_ITEMS < WK_C_COUNT, "the counters fit the fetch's buffer");

// the session's buffers (bw_restore::im)
enum {
    IM_B_BITS, IM_B_FRONT0, IM_B_FRONT1, IM_B_CTR, IM_B_ERR, IM_B_PF, IM_B_BAD, IM_B_EDGES, IM_B_OUT,  // the mark
    IM_B_TAINT, IM_B_ITEMS0, IM_B_ITEMS1, IM_B_REFS0, IM_B_REFS1, IM_B_LVL, IM_B_REC,                  // the report walk
    IM_B_COUNT
};
static_assert(IM_B_COUNT <= sizeof(bw_restore::im) / sizeof(DevBuf), "bw_restore::im holds every buffer");

struct ImEdge {
    uint32_t parent, child;  // entry indices; IM_EDGE_SELF_ONLY on the child of a File row
};

// The mark's device state as the kernels take it.
struct ImMark {
    RsLocator loc;
    const PrPackfile* pf;
    const uint8_t* bad;  // one byte per entry, or null
    uint32_t* bits;
    uint64_t* next;  // the next frontier: entry indices
    uint64_t* ctr;   // IM_C_*
    bw_prune_error* errs;
    uint64_t err_cap;
    ImEdge* edges;
    uint64_t edge_cap;
    ImEdge* leaf;  // RtReach: the edges that pass nothing on (IM_C_LEAF of them, edge_cap places too); else null
};

// What the mark's walk leaves to the walk that uses it, as the tree-chain fetch has ImFetch, DfFetch and
// PmFetch.  ALL_EDGES false: an edge per reference that resolves to a Tree entry, a chunk's taint settles
// into its parent's BELOW at once (impact).  ALL_EDGES true: an edge per reference that locates; those that
// can pass something on (a tree reference to a Tree entry) go to `edges` by level, the rest to `leaf`, and
// BELOW is set only for a reference that fails to locate or is a tree reference to a chunk (retain,
// bw_retain.hip: SELF | BELOW is then the entry's own damage, and nothing is propagated over them).
struct ImTaint {
    static constexpr bool ALL_EDGES = false;
};
struct RtReach {
    static constexpr bool ALL_EDGES = true;
};

// What im_walk leaves: on the device the bits, the edge lists and the counters (w), here the rest.
struct ImWalked {
    ImMark w;
    ImLevels levels;  // `edges` by the level that appended them
    uint64_t ctr[IM_C_COUNT];
    std::vector<bw_prune_error> herr;  // what the chain refused: the host knows it first
    uint8_t* d_out;    // out_bytes of IM_B_OUT for the caller's results
    uint8_t* d_roots;  // behind them, the roots
};

// The walk both marks share (bw_impact.hip): roots, frontier loop, expansion.  dev_cap: the records of
// the device error list.  leaf: the buffer of the leaf edges (RtReach), or null.
template <class Pol>
int im_walk(bw_restore* s, const uint8_t* roots, uint64_t n_roots, const uint8_t* bad, uint32_t flags, uint64_t dev_cap,
            uint64_t out_bytes, DevBuf* leaf, ImWalked& wd);
// The walk's errors to the caller's list, bw_prune_mark's way: *n_dev = what the kernels met, *n_errors = all.
int im_errors_out(bw_restore* s, const ImWalked& wd, const char* walk, bw_prune_error* errs, uint64_t err_cap, uint64_t dev_cap,
                  uint64_t* n_dev, uint64_t* n_errors);

constexpr uint32_t IM_OK = 1;      // the item's first piece was read and parsed
constexpr uint32_t IM_CYCLIC = 2;  // its hash is one of its ancestors': its list counts as empty
constexpr uint32_t IM_TRUNC = 4;   // a later piece of its chain is lost
constexpr uint64_t IM_NONE = ~0ull;

// One item of a level of the report walk.
struct ImItem {
    uint8_t hash[32];
    uint64_t parent;  // the parent item's record, ~0 for a root
    uint32_t root, state;
    uint32_t kind, tflags;
    uint64_t size, mtime, ctime;
    uint64_t name_off, name_len;  // in the walk's name arena
    uint64_t n_affected, first_affected;
};

// The report walk's device state.
struct ImWalk {
    WkFetch f;  // the shared fetch; f.names holds every name so far
    ImItem* items;
    bw_impact_record* recs;  // every record so far; item i of the level owns record rec0 + i
    uint64_t* ctr;           // WK_C_ERRORS, IM_C_ITEMS
    const uint8_t* taint;
    const uint64_t *item_row0, *item_rows;
    uint64_t n_rows, n_items, level, rec0;
};

}  // namespace bw
