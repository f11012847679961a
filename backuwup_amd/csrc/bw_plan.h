// bw_plan.h -- the batch plan: what the host derives from a batch's file list before anything is
// enqueued (which files go through CDC, segment length, the counts and bounds that size the buffers,
// the tables the kernels read).  No device, context or HIP header: tests/cpp/plan_selftest.cpp.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../include/backuwup_gpu.h"
#include "bw_tables.inc"

namespace bw {

#ifndef BW_SCAN_STRIP
#define BW_SCAN_STRIP 2048
#endif
constexpr int SCAN_STRIP = BW_SCAN_STRIP;                          // bytes per lane
constexpr uint64_t SCAN_TILE = 64ull * SCAN_STRIP;                 // one wave's sub-tile (128 KiB)
constexpr uint32_t SCAN_TILE_SHIFT = __builtin_ctzll(SCAN_TILE);
constexpr int CHAIN_CAP = 128;                                    // cuts stored per segment

struct Masks {
    uint32_t min, avg, max, s0;  // s0 = 2 * (min / 2): first position the crate hashes
    uint64_t mask_s, mask_l, mask_pre;  // mask_pre = mask_s & mask_l (scan prefilter)
    uint32_t pre_shift;  // the scan carries h << pre_shift; 63 - top bit of (mask_s | mask_l)
    uint32_t pre_hi;     // bits of mask_pre inside the high dword of h << pre_shift
    uint32_t tile_shift; // log2 of the scan tile in bytes (SCAN_TILE, or half of it for small batches)
};

// One boundary-resolution segment: a window [start, end) of one CDC file.
struct SegDesc {
    uint64_t start, end, file_end;
    uint32_t cfile;  // index among the batch's CDC files
    uint32_t last;   // 1 = last segment of its file
};

struct CFileDesc {
    uint64_t start, end;  // global byte range of the file
    uint64_t fb_off;      // offset into the serial-walker output buffer
    uint32_t first_seg, nseg;
};

// Canonical-order unit: either a whole small file (kind 0) or one CDC segment (kind 1).
struct UnitDesc {
    uint64_t start, len;  // small file: its range; segment: unused
    uint32_t file;        // batch file index
    uint32_t kind;        // 0 = small-file blob, 1 = CDC segment
    uint32_t seg;         // segment index (kind 1)
    uint32_t cfile;       // CDC file index (kind 1)
};
static_assert(sizeof(SegDesc) % 8 == 0 && sizeof(CFileDesc) % 8 == 0 && sizeof(UnitDesc) % 8 == 0, "staging alignment");

// fn(lo, hi) over [0, n) on up to 16 threads: the host-side table work of million-item batches
// (16 = this GPU's share of the box's cores).  `work` (default n) sizes the thread count; small
// work runs inline.
template <typename F>
void parallel_ranges(uint64_t n, F fn, uint64_t work = 0) {
    if (!work) work = n;
    // (no core count for small work: the C library reads /sys for it, and a small batch's count precedes its scan)
    uint64_t t = 1;
    if (work >= 65536) {
        const uint64_t hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        t = std::min<uint64_t>(std::min<uint64_t>(hw, work / 32768), n);
    }
    if (t <= 1) {
        fn(0, n);
        return;
    }
    std::vector<std::thread> th;
    for (uint64_t k = 0; k < t; k++) th.emplace_back(fn, n * k / t, n * (k + 1) / t);
    for (auto& x : th) x.join();
}

inline int make_masks(uint32_t mn, uint32_t av, uint32_t mx, Masks* mk) {
    static const uint64_t masks[26] = BW_MASKS_INIT;
    // FastCDC::with_level asserts (fastcdc 3.0.3 v2020) -> BW_EINVAL instead of a panic.
    if (mn < BW_MINIMUM_MIN || mn > BW_MINIMUM_MAX) return BW_EINVAL;
    if (av < BW_AVERAGE_MIN || av > BW_AVERAGE_MAX) return BW_EINVAL;
    if (mx < BW_MAXIMUM_MIN || mx > BW_MAXIMUM_MAX) return BW_EINVAL;
    // avg > max passes the crate's asserts, but then cut() keeps center = avg past remaining = max:
    // its first loop reads beyond max (a cut there makes a chunk longer than max) and, where the
    // source ends first, indexes out of bounds -- a panic, on most inputs (oracle/bw_oracle.c
    // ORC_CUT_PANIC restates it).  backuwup never passes such sizes (dir_packer.rs:254-259); the
    // ABI refuses them instead of returning chunks the crate would not.
    if (av > mx) return BW_EINVAL;
    const uint32_t bits = (uint32_t)lround(log2((double)av));  // logarithm2(): round(log2(avg))
    mk->min = mn;
    mk->avg = av;
    mk->max = mx;
    mk->s0 = 2 * (mn / 2);
    mk->mask_s = masks[bits + 1];  // Normalization::Level1
    mk->mask_l = masks[bits - 1];
    mk->mask_pre = mk->mask_s & mk->mask_l;
    mk->pre_shift = (uint32_t)__builtin_clzll(mk->mask_s | mk->mask_l);  // 63 - top bit
    mk->pre_hi = (uint32_t)((mk->mask_pre << mk->pre_shift) >> 32);
    mk->tile_shift = SCAN_TILE_SHIFT;
    return BW_OK;
}

inline uint64_t seg_len_for(const Masks& mk, bool small_batch) {
    // Segments are a multiple of max_size so that chains through data without candidates
    // (e.g. zeros: every chunk is exactly max) stay phase-aligned and merge immediately; the
    // multiple keeps a segment's own cuts within CHAIN_CAP / 2.  Small batches take at most 2 x max:
    // their chain walk is latency on the critical path (one wave walks a segment's cuts one after
    // another, ~1.7 us each), and more, shorter segments walk in parallel.
    uint64_t k = (uint64_t)(CHAIN_CAP / 2) * std::min<uint64_t>(mk.s0, mk.max) / mk.max;
    if (k < 1) k = 1;
    if (k > (small_batch ? 2 : 8)) k = small_batch ? 2 : 8;
    return k * mk.max;
}

// Upper bound of the chunks CDC cuts `len` bytes into: every chunk but the last is at least
// min(s0, max) bytes (s0 = 2 * (min / 2) is the first position the crate tests, so an odd min
// counts one less; max < min is legal in the crate and then max is the shorter), the last may be
// shorter, and one more keeps the bound strict.
inline uint64_t chunk_bound(const Masks& mk, uint64_t len) { return len / std::min<uint64_t>(mk.s0, mk.max) + 2; }

// process_file's policy (dir_packer.rs:231-282): a file above the threshold is chunked by CDC, a
// smaller or an empty one is a single blob.
inline bool is_cdc_file(uint64_t len, uint64_t small_file_threshold) { return len > small_file_threshold && len > 0; }

struct PlanSums {
    uint64_t nseg = 0, ncf = 0, nunits = 0, fb_total = 0, max_blobs = 0, total_len = 0, max_blob_len = 0;
};

// The batch plan.  init() checks the caller's file list, once per public call (files(): a part of a
// checked list).  count() and fill() are two passes over file ranges (in parallel for large batches:
// C4's million files took ~4 ms on one thread); the tables are the same as one serial walk in file order.
struct BatchPlan : PlanSums {
    static constexpr uint64_t RANGES = 64, RANGES_FROM = 65536;  // files from which the walk is split

    uint64_t data_len = 0, nf = 0;
    const uint64_t *foff = nullptr, *flen = nullptr;
    const bw_params* prm = nullptr;
    Masks mk;  // (tile_shift is the batch's after count())
    uint64_t tile_bytes = 0, n_tiles = 0, seg_bytes = 0;
    size_t meta_bytes = 0;       // the four tables back to back
    std::vector<PlanSums> base;  // per range: the sums of the ranges before it; the last: the batch's

    int init(uint64_t len, const uint64_t* off, const uint64_t* lens, uint64_t n, const bw_params* p, std::string* err) {
        if (int rc = make_masks(p->min_size, p->avg_size, p->max_size, &mk)) {
            *err = "fastcdc parameters out of range";
            return rc;
        }
        if (n && (!off || !lens)) return BW_EINVAL;
        for (uint64_t f = 0; f < n; f++)
            if (off[f] > len || lens[f] > len - off[f]) {
                *err = "file " + std::to_string(f) + " lies outside the data buffer";
                return BW_EINVAL;
            }
        data_len = len, foff = off, flen = lens, nf = n, prm = p;
        return BW_OK;
    }
    BatchPlan files(uint64_t f0, uint64_t n) const {
        BatchPlan r = *this;
        if (n) r.foff += f0, r.flen += f0;
        r.nf = n;
        return r;
    }

    uint64_t first_file(uint64_t k) const { return nf * k / (base.size() - 1); }
    bool cdc(uint64_t f) const { return is_cdc_file(flen[f], prm->small_file_threshold); }
    uint64_t segs_of(uint64_t f) const { return (flen[f] + seg_bytes - 1) / seg_bytes; }

    void count(uint64_t scan_small_bytes) {
        // small batches scan half-size tiles: with one 128 KiB tile per wave the per-tile start
        // costs dominate (C1: 0.50 -> 0.33 ms per GiB); large ones keep the longer strips
        // (BW_OPT_SCAN_SMALL_BYTES moves the threshold, so the tests can run either tile size on any input)
        const bool small_batch = data_len < scan_small_bytes;
        mk.tile_shift = small_batch ? SCAN_TILE_SHIFT - 1 : SCAN_TILE_SHIFT;
        tile_bytes = 1ull << mk.tile_shift;
        seg_bytes = seg_len_for(mk, small_batch);
        const uint64_t T = nf >= RANGES_FROM ? RANGES : 1;
        base.assign(T + 1, PlanSums());
        parallel_ranges(T, [&](uint64_t k0, uint64_t k1) {
            for (uint64_t k = k0; k < k1; k++) {
                PlanSums& q = base[k + 1];
                for (uint64_t f = first_file(k); f < first_file(k + 1); f++) {
                    q.total_len += flen[f];
                    if (cdc(f)) {
                        const uint64_t ns = segs_of(f), nb = chunk_bound(mk, flen[f]);
                        q.nseg += ns, q.nunits += ns, q.ncf++;
                        q.fb_total += nb, q.max_blobs += nb;
                    } else {
                        q.nunits++, q.max_blobs++;
                        q.max_blob_len = std::max<uint64_t>(q.max_blob_len, flen[f]);
                    }
                }
            }
        }, nf);
        // a CDC chunk is <= max, or <= min where cut() returns a remainder <= min whole before clipping
        // to max (min > max is legal in the crate; round-6 fuzz: a 70,325 B chunk under max = 1,520)
        base[0].max_blob_len = std::max<uint64_t>(mk.max, mk.min);
        for (uint64_t k = 1; k <= T; k++) {
            PlanSums& q = base[k];
            const PlanSums& b = base[k - 1];
            q.nseg += b.nseg, q.ncf += b.ncf, q.nunits += b.nunits, q.fb_total += b.fb_total;
            q.max_blobs += b.max_blobs, q.total_len += b.total_len;
            q.max_blob_len = std::max(q.max_blob_len, b.max_blob_len);
        }
        PlanSums::operator=(base[T]);
        n_tiles = ncf ? (data_len + tile_bytes - 1) / tile_bytes : 0;
        meta_bytes = nseg * sizeof(SegDesc) + ncf * sizeof(CFileDesc) + nunits * sizeof(UnitDesc) + nf * 8;
    }

    // the tables inside a buffer of meta_bytes (host staging or its device copy: the same layout)
    SegDesc* segs(void* buf) const { return (SegDesc*)buf; }
    CFileDesc* cfiles(void* buf) const { return (CFileDesc*)(segs(buf) + nseg); }
    UnitDesc* units(void* buf) const { return (UnitDesc*)(cfiles(buf) + ncf); }
    uint64_t* fstart(void* buf) const { return (uint64_t*)(units(buf) + nunits); }

    void fill(void* buf) const {
        SegDesc* const sg = segs(buf);
        CFileDesc* const cfs = cfiles(buf);
        UnitDesc* const un = units(buf);
        const uint64_t L = seg_bytes;
        parallel_ranges(base.size() - 1, [&](uint64_t k0, uint64_t k1) {
            for (uint64_t k = k0; k < k1; k++) {
                uint64_t si = base[k].nseg, ci = base[k].ncf, ui = base[k].nunits, fb = base[k].fb_total;
                const uint64_t f0 = first_file(k), f1 = first_file(k + 1);
                if (f1 > f0) memcpy(fstart(buf) + f0, foff + f0, (f1 - f0) * 8);
                for (uint64_t f = f0; f < f1; f++) {
                    const uint64_t start = foff[f], len = flen[f];
                    if (!cdc(f)) {
                        un[ui++] = UnitDesc{start, len, (uint32_t)f, 0, 0, 0};
                        continue;
                    }
                    const uint64_t ns = segs_of(f), end = start + len;
                    for (uint64_t j = 0; j < ns; j++) {
                        un[ui++] = UnitDesc{0, 0, (uint32_t)f, 1, (uint32_t)si, (uint32_t)ci};
                        sg[si++] = SegDesc{start + j * L, std::min(start + (j + 1) * L, end), end, (uint32_t)ci, j + 1 == ns};
                    }
                    cfs[ci++] = CFileDesc{start, end, fb, (uint32_t)(si - ns), (uint32_t)ns};
                    fb += chunk_bound(mk, len);
                }
            }
        }, nf);
    }
};

}  // namespace bw
