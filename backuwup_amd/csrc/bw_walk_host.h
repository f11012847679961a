// bw_walk_host.h -- the host arithmetic of a tree-chain fetch (bw_walk.h), shared by the diff walk and the
// parent match: the take table of one sub-batch and the layout of a level's segments.  Free of HIP so
// that a plain C++ test can include it (tests/test_walk_host.py).  Off the chunk -> hash -> dedup path.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "bw_store_layout.h"

namespace bw {

constexpr uint64_t WK_NONE = ~0ull;

// What the host tells the take kernel about blob b of a sub-batch.
struct WkTake {
    uint32_t ref, cst;  // the reference it answers; the unpack chain's status
    uint64_t stage;     // where its children rows go in the staging arena (rows)
    uint64_t n_rows;    // how many are taken (0 for a skipped owner, or when only the header is asked for)
    uint64_t name_off;  // where its name goes (when the header is asked for)
    uint64_t next;      // its next_sibling's place among the next round's references, or ~0
    uint64_t seg;       // its segment, or ~0 when it has no rows
};

// The rows one piece gave: `count` rows at row `stage` of the staging arena, for owner `node`.
struct WkSeg {
    uint32_t node, sid;  // sid: its number in fetch order
    uint64_t stage, count;
};

// What the fetch knows of an owner of chains (a diff node, a parent-match item).
struct WkOwner {
    uint64_t n_rows = 0;
    uint8_t skip = 0;  // read for its header only: no rows, no chain (the diff walk's cyclic node)
    uint8_t dir = 0;   // its header said Dir
};

// What a level's fetches have staged so far.
struct WkLevel {
    std::vector<WkSeg> segs;
    uint64_t stage_rows = 0, name_total = 0;
};

struct WkAdd {
    uint64_t rows = 0, names = 0, segs = 0;
};

// The take table of one sub-batch of m blobs: blob k answers reference ref[k], read for owner
// ref_owner[ref[k]]; cst[k] is the unpack chain's status and hd[k] the parser's header.  header: a good
// blob gives its header and name; rows: it gives its rows and its next_sibling.  A good blob's segment
// joins L.segs and its next_sibling's owner joins next_owner; owners (may be null) keeps the per-owner
// sums.  -> what the sub-batch adds to the level; the caller adds rows and names to L once it is taken.
static inline WkAdd wk_plan(WkLevel& L, const uint32_t* ref, const uint32_t* ref_owner, const uint8_t* cst,
                            const RsTreeHdr* hd, uint64_t m, bool header, bool rows, WkOwner* owners, WkTake* take,
                            std::vector<uint32_t>& next_owner) {
    WkAdd add;
    for (uint64_t k = 0; k < m; k++) {
        WkTake& tk = take[k];
        const RsTreeHdr& h = hd[k];
        const uint32_t owner = ref_owner[ref[k]];
        tk.ref = ref[k];
        tk.cst = cst[k];
        tk.stage = L.stage_rows + add.rows;
        tk.name_off = L.name_total + add.names;
        tk.n_rows = 0;
        tk.next = tk.seg = WK_NONE;
        if (tk.cst || h.status) continue;
        if (header) {
            add.names += h.name_len;
            if (owners) owners[owner].dir = h.kind == BW_TREE_DIR;
        }
        if (!rows || (owners && owners[owner].skip)) continue;
        tk.n_rows = h.n_children;
        if (h.n_children) {
            tk.seg = L.segs.size();
            L.segs.push_back(WkSeg{owner, (uint32_t)L.segs.size(), tk.stage, h.n_children});
            add.segs++;
            add.rows += h.n_children;
            if (owners) owners[owner].n_rows += h.n_children;
        }
        if (h.has_next) {
            tk.next = next_owner.size();
            next_owner.push_back(owner);
        }
    }
    return add;
}

// The level's lists, owner after owner, a chain's segments in chain order (the sort is stable and the
// fetch met a chain's pieces in order).  seg_row0 has a place more than the segments.  -> the rows in all.
static inline uint64_t wk_layout(std::vector<WkSeg>& segs, uint64_t* seg_row0, uint64_t* seg_stage, uint32_t* seg_node,
                                 uint32_t* seg_sid) {
    std::stable_sort(segs.begin(), segs.end(), [](const WkSeg& a, const WkSeg& b) { return a.node < b.node; });
    uint64_t run = 0;
    for (uint64_t k = 0; k < segs.size(); k++) {
        seg_row0[k] = run;
        seg_stage[k] = segs[k].stage;
        seg_node[k] = segs[k].node;
        seg_sid[k] = segs[k].sid;
        run += segs[k].count;
    }
    seg_row0[segs.size()] = run;
    return run;
}

}  // namespace bw
