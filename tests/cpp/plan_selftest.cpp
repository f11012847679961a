// plan_selftest.cpp -- the batch plan (backuwup_amd/csrc/bw_plan.h) against one serial walk.
//
// bw_plan.h counts a batch's segments, CDC files, units and bounds over file ranges and fills the
// SegDesc | CFileDesc | UnitDesc | fstart tables at the ranges' prefix offsets, on host threads from
// 65,536 files on.  Its comment claims that the tables equal one serial walk in file order: naive()
// below is that walk, pushing onto vectors, with the segment length, the blob bound and the CDC rule
// restated from their definitions, and every case compares every table byte and plan field with it.
// tests/test_plan.py builds this once with ASan + UBSan and once with TSan (the parallel fill is
// the only threaded code on the path), and pins `model` mode's output to tests/cdc_chain_plant.py.
#include <stdio.h>
#include <stdlib.h>

#include "../../backuwup_amd/csrc/bw_plan.h"

using namespace bw;

static int g_failed = 0;
#define CHECK(name, cond)                                                          \
    do {                                                                           \
        if (!(cond)) {                                                             \
            printf("FAIL %s: %s (line %d)\n", (name).c_str(), #cond, __LINE__);    \
            g_failed++;                                                            \
        }                                                                          \
    } while (0)

static bw_params params(uint32_t mn, uint32_t av, uint32_t mx, uint64_t threshold) {
    bw_params p;
    memset(&p, 0, sizeof p);
    p.min_size = mn;
    p.avg_size = av;
    p.max_size = mx;
    p.small_file_threshold = threshold;
    return p;
}

struct Naive {
    std::vector<SegDesc> segs;
    std::vector<CFileDesc> cfs;
    std::vector<UnitDesc> units;
    std::vector<uint64_t> fstart;
    uint64_t seg_bytes = 0, tile_bytes = 0, n_tiles = 0, fb = 0, max_blobs = 0, total_len = 0, max_blob_len = 0;
    std::vector<PlanSums> base;  // the running sums where each of the plan's ranges starts
};

static Naive naive(uint64_t data_len, const std::vector<uint64_t>& foff, const std::vector<uint64_t>& flen,
                   const bw_params& p, bool small_batch) {
    Naive r;
    const uint64_t nf = flen.size();
    const uint64_t s0 = 2 * (uint64_t)(p.min_size / 2), shortest = s0 < p.max_size ? s0 : p.max_size;
    uint64_t k = 64 * shortest / p.max_size;  // CHAIN_CAP / 2 cuts of the shortest chunk, in max_size
    const uint64_t most = small_batch ? 2 : 8;
    k = k < 1 ? 1 : (k > most ? most : k);
    const uint64_t L = r.seg_bytes = k * p.max_size;
    r.tile_bytes = small_batch ? 65536 : 131072;
    r.max_blob_len = p.max_size > p.min_size ? p.max_size : p.min_size;
    const uint64_t T = nf >= 65536 ? 64 : 1;
    uint64_t next_range = 0;
    for (uint64_t f = 0; f <= nf; f++) {
        while (next_range < T && nf * next_range / T == f) {
            PlanSums b;
            b.nseg = r.segs.size(), b.ncf = r.cfs.size(), b.nunits = r.units.size(), b.fb_total = r.fb;
            b.max_blobs = r.max_blobs, b.total_len = r.total_len, b.max_blob_len = r.max_blob_len;
            r.base.push_back(b);
            next_range++;
        }
        if (f == nf) break;
        r.fstart.push_back(foff[f]);
        r.total_len += flen[f];
        if (flen[f] > p.small_file_threshold && flen[f] > 0) {
            const uint64_t bound = flen[f] / shortest + 2, end = foff[f] + flen[f];
            CFileDesc cf;
            cf.start = foff[f], cf.end = end, cf.fb_off = r.fb;
            cf.first_seg = (uint32_t)r.segs.size(), cf.nseg = 0;
            for (uint64_t at = foff[f]; at < end; at += L) {
                SegDesc sd;
                sd.start = at, sd.end = at + L < end ? at + L : end, sd.file_end = end;
                sd.cfile = (uint32_t)r.cfs.size(), sd.last = at + L >= end;
                UnitDesc u;
                u.start = 0, u.len = 0, u.file = (uint32_t)f, u.kind = 1;
                u.seg = (uint32_t)r.segs.size(), u.cfile = sd.cfile;
                r.units.push_back(u);
                r.segs.push_back(sd);
                cf.nseg++;
            }
            r.cfs.push_back(cf);
            r.fb += bound;
            r.max_blobs += bound;
        } else {
            UnitDesc u;
            u.start = foff[f], u.len = flen[f], u.file = (uint32_t)f, u.kind = 0, u.seg = 0, u.cfile = 0;
            r.units.push_back(u);
            r.max_blobs++;
            if (flen[f] > r.max_blob_len) r.max_blob_len = flen[f];
        }
    }
    r.n_tiles = r.cfs.empty() ? 0 : (data_len + r.tile_bytes - 1) / r.tile_bytes;
    return r;
}

static bool same_sums(const PlanSums& a, const PlanSums& b) {
    return a.nseg == b.nseg && a.ncf == b.ncf && a.nunits == b.nunits && a.fb_total == b.fb_total && a.max_blobs == b.max_blobs &&
           a.total_len == b.total_len && a.max_blob_len == b.max_blob_len;
}

// Files back to back from offset `lead` on; `first`/`count` plan a sub-range of the validated list
// (the two parts of a split batch).
static BatchPlan check(const std::string& name, const std::vector<uint64_t>& lens, const bw_params& p, bool small_batch,
                       uint64_t lead = 0, uint64_t first = 0, uint64_t count = ~0ull) {
    std::vector<uint64_t> foff(lens.size());
    uint64_t data_len = lead;
    for (size_t f = 0; f < lens.size(); f++) {
        foff[f] = data_len;
        data_len += lens[f];
    }
    BatchPlan whole;
    std::string err;
    const int rc = whole.init(data_len, lens.empty() ? nullptr : foff.data(), lens.empty() ? nullptr : lens.data(),
                              lens.size(), &p, &err);
    CHECK(name, rc == BW_OK && err.empty());
    if (rc) return whole;
    if (count == ~0ull) count = lens.size() - first;
    const std::vector<uint64_t> sub_off(foff.begin() + first, foff.begin() + first + count),
        sub_len(lens.begin() + first, lens.begin() + first + count);
    BatchPlan pl = whole.files(first, count);
    pl.count(small_batch ? ~0ull : 0);
    const Naive want = naive(data_len, sub_off, sub_len, p, small_batch);

    Masks mk;
    CHECK(name, make_masks(p.min_size, p.avg_size, p.max_size, &mk) == BW_OK);
    mk.tile_shift = small_batch ? 16 : 17;
    CHECK(name, mk.min == pl.mk.min && mk.avg == pl.mk.avg && mk.max == pl.mk.max && mk.s0 == pl.mk.s0);
    CHECK(name, mk.mask_s == pl.mk.mask_s && mk.mask_l == pl.mk.mask_l && mk.mask_pre == pl.mk.mask_pre);
    CHECK(name, mk.pre_shift == pl.mk.pre_shift && mk.pre_hi == pl.mk.pre_hi && mk.tile_shift == pl.mk.tile_shift);
    CHECK(name, pl.tile_bytes == want.tile_bytes && pl.tile_bytes == 1ull << pl.mk.tile_shift);
    CHECK(name, pl.n_tiles == want.n_tiles);
    CHECK(name, pl.seg_bytes == want.seg_bytes);
    CHECK(name, pl.nseg == want.segs.size());
    CHECK(name, pl.ncf == want.cfs.size());
    CHECK(name, pl.nunits == want.units.size());
    CHECK(name, pl.fb_total == want.fb);
    CHECK(name, pl.max_blobs == want.max_blobs);
    CHECK(name, pl.total_len == want.total_len);
    CHECK(name, pl.max_blob_len == want.max_blob_len);
    CHECK(name, pl.meta_bytes == 32 * (want.segs.size() + want.cfs.size() + want.units.size()) + 8 * count);
    // the per-range prefix bases (max_blob_len's running maximum starts from max(min, max) in both)
    CHECK(name, pl.base.size() == want.base.size() + 1 && same_sums(pl.base.back(), pl));  // the last: the batch's
    for (size_t k = 0; k + 1 < pl.base.size() && k < want.base.size(); k++)
        CHECK(name, same_sums(pl.base[k], want.base[k]));

    std::vector<uint8_t> buf(pl.meta_bytes, 0xa5);  // exactly meta_bytes: a write past it is ASan's
    pl.fill(buf.data());
    std::vector<uint8_t> ref;
    auto put = [&](const void* q, size_t n) {
        if (n) ref.insert(ref.end(), (const uint8_t*)q, (const uint8_t*)q + n);
    };
    put(want.segs.data(), want.segs.size() * sizeof(SegDesc));
    put(want.cfs.data(), want.cfs.size() * sizeof(CFileDesc));
    put(want.units.data(), want.units.size() * sizeof(UnitDesc));
    put(want.fstart.data(), want.fstart.size() * 8);
    CHECK(name, ref.size() == buf.size());
    CHECK(name, ref.size() == buf.size() && (ref.empty() || memcmp(ref.data(), buf.data(), ref.size()) == 0));
    CHECK(name, (uint8_t*)pl.fstart(buf.data()) + 8 * count == buf.data() + buf.size());
    return pl;
}

static void reject(const std::string& name, uint64_t data_len, const uint64_t* foff, const uint64_t* flen, uint64_t nf,
                   const bw_params& p, const char* text) {
    BatchPlan pl;
    std::string err;
    CHECK(name, pl.init(data_len, foff, flen, nf, &p, &err) == BW_EINVAL);
    CHECK(name, err == text);
}

// 65,536 + 7 files over 64 ranges of 1,024 or 1,025: empty, small and CDC files mixed, range 3
// without a CDC file, range 5 with nothing else
static std::vector<uint64_t> many_files(uint64_t nf, uint64_t threshold) {
    const uint64_t whole = 65536 + 7;
    std::vector<uint64_t> lens(nf);
    for (uint64_t f = 0; f < nf; f++) {
        const uint64_t range = (f * 64 + 63) / whole;  // the k with whole * k / 64 <= f < whole * (k + 1) / 64
        const uint64_t tiny = f % 3 ? (f * 7919) % 49 : 0, big = threshold + 1 + (f * 104729) % 5000;
        lens[f] = range == 3 ? tiny : range == 5 ? big : (f % 11 == 4 ? big : tiny);
    }
    return lens;
}

static int selftest() {
    const bw_params def = params(262144, 1u << 20, 3u << 20, 1u << 20);  // backuwup's (defaults.rs:61-68)
    const bw_params odd = params(65, 256, 1024, 256);                    // odd min: s0 = 64
    const bw_params narrow = params(4096, 1024, 1024, 0);                // max < min
    const bw_params pf = params(64, 256, 1024, 256);

    for (int small = 0; small < 2; small++) {
        const std::string s = small ? " small" : " large";
        check("no files" + s, {}, def, small);
        check("no files, bytes" + s, {}, def, small, 100);
        check("one empty file" + s, {0}, def, small);
        check("around the threshold" + s, {(1u << 20) - 1, 1u << 20, (1u << 20) + 1}, def, small, 48);
        check("threshold 0" + s, {0, 1, 0, 5000, 0}, narrow, small);
        const struct {
            const char* name;
            bw_params p;
        } sets[] = {{"default", def}, {"odd min", odd}, {"max < min", params(4096, 1024, 1024, 256)}};
        for (const auto& ps : sets) {
            Masks mk;
            if (make_masks(ps.p.min_size, ps.p.avg_size, ps.p.max_size, &mk)) return 1;
            const uint64_t L = seg_len_for(mk, small);
            const BatchPlan pl = check(std::string("segment lengths, ") + ps.name + s,
                                       {L - 1, L, L + 1, 8 * L + 1, 0, 17, L}, ps.p, small, 16);
            CHECK(s, pl.nseg == 1 + 1 + 2 + 9 + 1 && pl.ncf == 5 && pl.nunits == pl.nseg + 2);
        }
        // the bound that min = 65 once missed: chunks of 64 bytes are legal there
        Masks mk;
        if (make_masks(65, 256, 1024, &mk)) return 1;
        CHECK(s, mk.s0 == 64 && chunk_bound(mk, 6400) == 102);

        const std::vector<uint64_t> many = many_files(65536 + 7, pf.small_file_threshold);
        const BatchPlan pl = check("65,543 files" + s, many, pf, small);
        CHECK(s, pl.base.size() == 65);
        if (pl.base.size() == 65) {
            CHECK(s, pl.base[4].ncf == pl.base[3].ncf);                                          // range 3: no CDC file
            CHECK(s, pl.base[6].ncf - pl.base[5].ncf == pl.first_file(6) - pl.first_file(5));    // range 5: only CDC files
            CHECK(s, pl.base[6].nunits - pl.base[5].nunits == pl.base[6].nseg - pl.base[5].nseg);
            CHECK(s, pl.ncf > 5000 && pl.nunits > pl.ncf + 50000);
        }
        std::vector<uint64_t> fewer(many.begin(), many.begin() + 65535);
        CHECK(s, check("65,535 files" + s, fewer, pf, small).base.size() == 2);
        // the parts of a split batch plan sub-ranges of the validated list
        check("head part" + s, many, pf, small, 0, 0, 30000);
        check("tail part" + s, many, pf, small, 0, 30000);
        check("part from 65,536 files on" + s, many, pf, small, 0, 3, 65536);
    }

    const uint64_t off[3] = {0, 101, 50}, len[3] = {50, 0, 51}, len2[3] = {50, 0, 50};
    BatchPlan ok;
    std::string err;
    CHECK(err, ok.init(100, off, len2, 1, &def, &err) == BW_OK);
    reject("foff > data_len", 100, off, len2, 3, def, "file 1 lies outside the data buffer");
    reject("flen > data_len - foff", 100, off + 2, len + 2, 1, def, "file 0 lies outside the data buffer");
    reject("null offsets", 100, nullptr, len, 1, def, "");
    reject("null lengths", 100, off, nullptr, 1, def, "");
    const char* range = "fastcdc parameters out of range";
    reject("avg > max", 100, off, len2, 1, params(64, 2048, 1024, 0), range);
    reject("min low", 100, off, len2, 1, params(BW_MINIMUM_MIN - 1, 256, 1024, 0), range);
    reject("min high", 100, off, len2, 1, params(BW_MINIMUM_MAX + 1, 1u << 20, 3u << 20, 0), range);
    reject("avg low", 100, off, len2, 1, params(64, BW_AVERAGE_MIN - 1, 1024, 0), range);
    reject("avg high", 100, off, len2, 1, params(64, BW_AVERAGE_MAX + 1, BW_MAXIMUM_MAX, 0), range);
    reject("max low", 100, off, len2, 1, params(64, 256, BW_MAXIMUM_MIN - 1, 0), range);
    reject("max high", 100, off, len2, 1, params(64, 256, BW_MAXIMUM_MAX + 1, 0), range);
    reject("bad parameters before bad files", 100, off, len2, 3, params(64, 2048, 1024, 0), range);

    if (g_failed) return 1;
    printf("plan selftest ok\n");
    return 0;
}

// model <min> <avg> <max> <threshold> <small 0|1> <len>...: the geometry of files laid back to back
static int model(int argc, char** argv) {
    if (argc < 7) return 2;
    const bw_params p = params((uint32_t)strtoull(argv[2], 0, 10), (uint32_t)strtoull(argv[3], 0, 10),
                               (uint32_t)strtoull(argv[4], 0, 10), strtoull(argv[5], 0, 10));
    const bool small = atoi(argv[6]) != 0;
    std::vector<uint64_t> off, len;
    uint64_t total = 0;
    for (int i = 7; i < argc; i++) {
        off.push_back(total);
        len.push_back(strtoull(argv[i], 0, 10));
        total += len.back();
    }
    BatchPlan pl;
    std::string err;
    if (pl.init(total, off.data(), len.data(), len.size(), &p, &err)) return 3;
    pl.count(small ? ~0ull : 0);
    printf("seg_bytes %llu segments %llu cdc_files %llu\n", (unsigned long long)pl.seg_bytes,
           (unsigned long long)pl.nseg, (unsigned long long)pl.ncf);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "model")) return model(argc, argv);
    return selftest();
}
