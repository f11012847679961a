// bw_parent_host.h -- the parent match's host-only rules (bw_parent.hip): what a scan has to be, and the
// sizing of a level's tables.  Free of HIP so that a plain C++ test can include it
// (tests/test_parent_host.py).  Off the chunk -> hash -> dedup path.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/backuwup_gpu_pack.h"
#include "bw_diff_host.h"

namespace bw {

// Rows, nodes and scan nodes of one level: the diff walk's limit, for the same reason (u32 indices,
// tables of twice the keys).  A level or a scan beyond this ends the call (BW_ENOMEM).
constexpr uint64_t PM_MAX_ROWS = DF_MAX_ROWS;

// The (item, name) table over n parent children: the diff walk's rule.
static inline uint32_t pm_table_cap(uint64_t n) { return df_table_cap(n); }

// A scan is what a stat-only directory walk yields, in the layout of a bw_restore_trees listing: node 0
// the root, a Dir's children the nodes [child_first, child_first + n_children), a File without children.
// Children come after their parent, the ranges lie inside the scan and no node is the child of two
// (counted by a difference array, so the whole check is O(n) in whatever order the ranges come).  An
// empty Dir's child_first says nothing, and nodes that no Dir names are allowed: they are never probed.
// -> 0, or 1 + the index of the first node that breaks a rule.
static inline uint64_t pm_scan_invalid(const bw_restore_node* nodes, uint64_t n_nodes, uint64_t names_len) {
    std::vector<int32_t> cover(n_nodes + 1, 0);
    for (uint64_t i = 0; i < n_nodes; i++) {
        const bw_restore_node& n = nodes[i];
        if (n.kind != BW_TREE_FILE && n.kind != BW_TREE_DIR) return i + 1;
        if (n.name_off > names_len || n.name_len > names_len - n.name_off) return i + 1;
        if (n.kind == BW_TREE_FILE) {
            if (n.n_children) return i + 1;
            continue;
        }
        if (!n.n_children) continue;
        if (n.child_first <= i || n.child_first > n_nodes || n.n_children > n_nodes - n.child_first) return i + 1;
        cover[n.child_first]++;
        cover[n.child_first + n.n_children]--;
    }
    // the first node two ranges hold is reported through the later of the Dirs that name it
    int64_t depth = 0;
    for (uint64_t k = 0; k < n_nodes; k++) {
        depth += cover[k];
        if (depth <= 1) continue;
        uint64_t bad = 0;
        for (uint64_t i = 0; i < k; i++)
            if (nodes[i].kind == BW_TREE_DIR && nodes[i].n_children && nodes[i].child_first <= k &&
                k - nodes[i].child_first < nodes[i].n_children)
                bad = i;
        return bad + 1;
    }
    return 0;
}

}  // namespace bw
