// bw_parity.hip -- parity (include/backuwup_gpu_pack.h, "parity"): systematic Reed-Solomon shards over
// packfiles and repair from them.  The reference has no redundancy.  GF(2^8) with the polynomial 0x11d
// and the generator 2; the parity coefficients are a Cauchy matrix, C[i][j] = inv(i ^ (m + j)).
// One kernel does the arithmetic of both directions: k_gf_matmul, dst_r = XOR_c M[r][c] * src_c over
// byte ranges, driven by a job table so that every group of a store goes into one launch.  Planning and
// the Gauss-Jordan solve are host code; the digests come from the batch hashing the verified unpack
// chain uses (bw_submit_device with BW_F_NO_DEDUP and whole-blob files).
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/backuwup_gpu.h"
#include "bw_device.h"
#include "bw_internal.h"
#include "bw_ctx.h"
#include "bw_store_layout.h"

using namespace bw;

namespace {

// ------------------------------------------------------------------ the field (host)
struct GfTables {
    uint8_t exp[512], log[256];
    GfTables() {
        uint32_t x = 1;
        for (int i = 0; i < 255; i++) {
            exp[i] = (uint8_t)x;
            log[x] = (uint8_t)i;
            x <<= 1;
            if (x & 0x100) x ^= 0x11d;
        }
        for (int i = 255; i < 512; i++) exp[i] = exp[i - 255];
        log[0] = 0;
    }
    uint8_t mul(uint8_t a, uint8_t b) const { return a && b ? exp[log[a] + log[b]] : 0; }
    uint8_t inv(uint8_t a) const { return exp[255 - log[a]]; }  // a != 0
};
const GfTables& gf() {
    static const GfTables t;
    return t;
}
inline uint8_t cauchy(uint32_t m, uint32_t i, uint32_t j) { return gf().inv((uint8_t)(i ^ (m + j))); }

// ------------------------------------------------------------------ k_gf_matmul
// One job is one matrix times its sources.  Its wave tasks are (pass, chunk): GF_ROW_TILE destination
// rows over GF_WAVE_BYTES bytes; task t of the launch belongs to the last job with tile0 <= t.
struct GfJob {
    uint64_t len;      // bytes of every destination row
    uint64_t tile0;    // the job's first wave task
    uint64_t coef_at;  // tab[coef_at + pass * cols + c]: byte t = M[pass * GF_ROW_TILE + t][c] (0 past the last row)
    uint64_t tab_at;   // tab[tab_at ..]: src_off[cols], src_len[cols], dst_off[rows]
    uint32_t rows, cols, chunks, passes;
};

typedef uint32_t gf_u4 __attribute__((ext_vector_type(4)));
typedef gf_u4 gf_u4_unaligned __attribute__((aligned(1)));

// the four bytes of x times 2: the high bits leave, 0x1d comes in where one was set
__device__ __forceinline__ uint32_t gf_x2(uint32_t x) {
    const uint32_t hi = x & 0x80808080u;
    return ((x ^ hi) << 1) ^ ((hi - (hi >> 7)) & 0x1d1d1d1du);
}

// bytes [b, b + 16) of a source of n bytes, zero at and beyond n: no byte outside the source is read
__device__ __forceinline__ gf_u4 gf_load16(const uint8_t* __restrict__ s, uint64_t n, uint64_t b) {
    gf_u4 v = {0, 0, 0, 0};
    if (b + 16 <= n) {
        v = *(const gf_u4_unaligned*)(s + b);
    } else if (b < n) {
        const uint32_t nb = (uint32_t)(n - b);
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 16; i++)
            if ((uint32_t)i < nb) w[i >> 2] |= (uint32_t)s[b + i] << (8 * (i & 3));
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    }
    return v;
}

// The coefficients are wave-uniform (one u64 per column holds the pass's GF_ROW_TILE of them), so the
// bit tests are scalar branches: a source word's seven doublings are computed once and xored into the
// accumulators the bits select.  No table lookup from memory.
__global__ __launch_bounds__(256) void k_gf_matmul(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                   const GfJob* __restrict__ jobs, uint32_t n_jobs,
                                                   const uint64_t* __restrict__ tab, uint64_t n_tiles) {
    constexpr int T = GF_ROW_TILE;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t first = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    for (uint64_t t = first; t < n_tiles; t += (uint64_t)gridDim.x * 4) {
        uint32_t lo = 0, hi = n_jobs - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (jobs[mid].tile0 <= t) lo = mid; else hi = mid - 1;
        }
        const GfJob J = jobs[lo];
        const uint64_t lt = t - J.tile0;
        const uint32_t pass = (uint32_t)(lt / J.chunks), chunk = (uint32_t)(lt - (uint64_t)pass * J.chunks);
        BW_ASSERT(pass < J.passes);
        const uint32_t rows_here = min((uint32_t)T, J.rows - pass * T);
        const uint64_t* cf = tab + J.coef_at + (uint64_t)pass * J.cols;
        const uint64_t* so = tab + J.tab_at;
        const uint64_t* sl = so + J.cols;
        const uint64_t* dof = sl + J.cols + (uint64_t)pass * T;
        for (uint32_t step = 0; step < GF_WAVE_BYTES / 1024; step++) {
            const uint64_t b0 = (uint64_t)chunk * GF_WAVE_BYTES + step * 1024;
            if (b0 >= J.len) break;
            const uint64_t b = b0 + 16 * lane;
            const bool live = b < J.len;
            gf_u4 acc[T];
#pragma unroll
            for (int r = 0; r < T; r++) acc[r] = gf_u4{0, 0, 0, 0};
            gf_u4 next = gf_load16(src + so[0], live ? sl[0] : 0, b);
            for (uint32_t c = 0; c < J.cols; c++) {
                gf_u4 d[8];
                d[0] = next;
                if (c + 1 < J.cols) next = gf_load16(src + so[c + 1], live ? sl[c + 1] : 0, b);  // under this column's arithmetic
                const uint64_t m8 = cf[c];
                if (!m8) continue;
#pragma unroll
                for (int k = 1; k < 8; k++) {
                    d[k].x = gf_x2(d[k - 1].x); d[k].y = gf_x2(d[k - 1].y);
                    d[k].z = gf_x2(d[k - 1].z); d[k].w = gf_x2(d[k - 1].w);
                }
#pragma unroll
                for (int r = 0; r < T; r++) {
                    const uint32_t m = (uint32_t)(m8 >> (8 * r)) & 0xff;
                    if (!m) continue;
#pragma unroll
                    for (int k = 0; k < 8; k++)
                        if (m & (1u << k)) {
                            asm volatile("");  // keeps the branch: if-converted, every bit costs 4 xors and 4 selects
                            acc[r] ^= d[k];
                        }
                }
            }
#pragma unroll
            for (int r = 0; r < T; r++) {
                if ((uint32_t)r >= rows_here) break;
                uint8_t* o = dst + dof[r] + b;
                if (b + 16 <= J.len) {
                    *(gf_u4*)o = acc[r];
                } else if (live) {
                    const uint32_t nb = (uint32_t)(J.len - b);
                    const uint32_t w[4] = {acc[r].x, acc[r].y, acc[r].z, acc[r].w};
#pragma unroll
                    for (int i = 0; i < 16; i++)
                        if ((uint32_t)i < nb) o[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
                }
            }
        }
    }
}

// one wave per range: flag[i] != 0 where a byte of [off, off + len) is not zero (a rebuilt data shard's tail)
struct GfRange {
    uint64_t off, len;
};
__global__ __launch_bounds__(64) void k_gf_nonzero(const uint8_t* __restrict__ p, const GfRange* __restrict__ ranges,
                                                   uint32_t* __restrict__ flag) {
    const GfRange r = ranges[blockIdx.x];
    uint32_t any = 0;
    for (uint64_t i = threadIdx.x; i < r.len; i += 64) any |= p[r.off + i];
    if (any) atomicOr(&flag[blockIdx.x], 1u);
}

struct GfCall {
    const uint8_t* matrix;  // rows x cols, row-major
    uint32_t rows, cols;
    const uint64_t *src_off, *src_len, *dst_off;
    uint64_t len;
};

bool overlap(uint64_t a, uint64_t an, uint64_t b, uint64_t bn) { return an && bn && a < b + bn && b < a + an; }

// every check that can refuse a call: before the first byte is written
int gf_validate(bw_ctx* c, const uint8_t* d_src, const uint8_t* d_dst, const GfCall& g) {
    if (!g.rows || !g.cols || g.cols > 255 || !g.matrix || !g.src_off || !g.src_len || !g.dst_off) return BW_EINVAL;
    if (!g.len) return BW_OK;
    if (!d_src || !d_dst || ((uintptr_t)d_dst & 15)) return BW_EINVAL;
    for (uint32_t r = 0; r < g.rows; r++)
        if (g.dst_off[r] & 15) {
            c->err = "gf_matmul: destination " + std::to_string(r) + " is not 16-byte aligned";
            return BW_EINVAL;
        }
    // destinations against each other (sorted) and against the sources
    std::vector<uint64_t> d(g.dst_off, g.dst_off + g.rows);
    std::sort(d.begin(), d.end());
    for (uint32_t r = 1; r < g.rows; r++)
        if (d[r] - d[r - 1] < g.len) {
            c->err = "gf_matmul: destinations overlap";
            return BW_EINVAL;
        }
    for (uint32_t s = 0; s < g.cols; s++) {
        const uint64_t a = (uint64_t)(uintptr_t)d_src + g.src_off[s], an = std::min(g.src_len[s], g.len);
        auto it = std::upper_bound(d.begin(), d.end(), a - (uint64_t)(uintptr_t)d_dst);
        for (int k = 0; k < 2; k++) {  // the destination at or before the source's start, and the one after
            if (k == 0 ? it == d.begin() : it == d.end()) continue;
            const uint64_t o = k == 0 ? *(it - 1) : *it;
            if (overlap(a, an, (uint64_t)(uintptr_t)d_dst + o, g.len)) {
                c->err = "gf_matmul: a destination overlaps source " + std::to_string(s);
                return BW_EINVAL;
            }
        }
    }
    return BW_OK;
}

// all calls in one launch on the context's stream; not synchronized
int gf_launch(bw_ctx* c, const uint8_t* d_src, uint8_t* d_dst, const std::vector<GfCall>& calls) {
    std::vector<GfJob> jobs;
    std::vector<uint64_t> tab;
    uint64_t tiles = 0;
    for (const GfCall& g : calls) {
        if (!g.len) continue;
        GfJob j;
        j.len = g.len;
        j.tile0 = tiles;
        j.rows = g.rows;
        j.cols = g.cols;
        j.chunks = (uint32_t)((g.len + GF_WAVE_BYTES - 1) / GF_WAVE_BYTES);
        j.passes = (g.rows + GF_ROW_TILE - 1) / GF_ROW_TILE;
        j.coef_at = tab.size();
        for (uint32_t p = 0; p < j.passes; p++)
            for (uint32_t col = 0; col < g.cols; col++) {
                uint64_t m8 = 0;
                for (uint32_t t = 0; t < (uint32_t)GF_ROW_TILE && p * GF_ROW_TILE + t < g.rows; t++)
                    m8 |= (uint64_t)g.matrix[(uint64_t)(p * GF_ROW_TILE + t) * g.cols + col] << (8 * t);
                tab.push_back(m8);
            }
        j.tab_at = tab.size();
        tab.insert(tab.end(), g.src_off, g.src_off + g.cols);
        tab.insert(tab.end(), g.src_len, g.src_len + g.cols);
        tab.insert(tab.end(), g.dst_off, g.dst_off + g.rows);
        tab.resize(tab.size() + GF_ROW_TILE, 0);  // the last pass's dst_off window ends inside the table
        tiles += (uint64_t)j.chunks * j.passes;
        jobs.push_back(j);
    }
    if (jobs.empty()) return BW_OK;
    const uint64_t tab_bytes = tab.size() * 8, job_bytes = jobs.size() * sizeof(GfJob);
    if (int rc = ensure(c, c->gf_tab, tab_bytes + job_bytes)) return rc;
    uint8_t* t = P<uint8_t>(c->gf_tab);
    HIPCHK(c, hipMemcpyAsync(t, tab.data(), tab_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(t + tab_bytes, jobs.data(), job_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the host tables go out of scope
    const uint64_t grid = std::min<uint64_t>((tiles + 3) / 4, GF_GRID_BLOCKS);
    hipLaunchKernelGGL(k_gf_matmul, dim3((unsigned)grid), dim3(256), 0, c->stream, d_src, d_dst, (const GfJob*)(t + tab_bytes),
                       (uint32_t)jobs.size(), (const uint64_t*)t, tiles);
    HIPCHK(c, hipGetLastError());
    return BW_OK;
}

// BLAKE3 of n nonempty ranges of a device buffer, whole (no chunking, no index): out is n x 32 on the host
int hash_ranges(bw_ctx* c, const uint8_t* d_base, const uint64_t* off, const uint64_t* len, uint64_t n, uint8_t* out) {
    if (!n) return BW_OK;
    const uint64_t skew = (uintptr_t)d_base & 15;  // bw_submit_device wants a 16-byte aligned base
    std::vector<uint64_t> o(n);
    uint64_t end = 0;
    for (uint64_t i = 0; i < n; i++) {
        o[i] = off[i] + skew;
        end = std::max(end, o[i] + len[i]);
    }
    bw_params p;
    bw_params_default(&p);
    p.flags = BW_F_NO_DEDUP;
    p.small_file_threshold = ~0ull;  // every range is hashed whole
    uint64_t ticket = 0, got = 0;
    std::vector<bw_blob> rec(n);
    if (int rc = bw_submit_device(c, d_base - skew, end, o.data(), len, n, &p, &ticket)) return rc;
    if (int rc = bw_wait(c, ticket, rec.data(), rec.size(), &got)) return rc;
    if (got != n) {
        c->err = "parity: the hash pass returned another number of blobs";
        return BW_EHIP;
    }
    for (uint64_t i = 0; i < n; i++) {
        if (rec[i].file >= n) return BW_EHIP;
        memcpy(out + 32 * rec[i].file, rec[i].digest, 32);
    }
    return BW_OK;
}

bool group_ok(const bw_parity_group& g) {
    return g.k && g.m && (uint64_t)g.k + g.m <= 256 && g.shard_len && !(g.shard_len & 15);
}

}  // namespace

// ------------------------------------------------------------------ C ABI: the primitive
extern "C" int bw_gf_matmul_device(bw_ctx* c, const uint8_t* matrix, uint32_t rows, uint32_t cols, const uint8_t* d_src,
                                   const uint64_t* src_off, const uint64_t* src_len, uint8_t* d_dst, const uint64_t* dst_off,
                                   uint64_t len) {
    if (!c) return BW_EINVAL;
    const GfCall g{matrix, rows, cols, src_off, src_len, dst_off, len};
    if (int rc = gf_validate(c, d_src, d_dst, g)) return rc;
    if (!len) return BW_OK;
    hipSetDevice(c->device);
    if (int rc = gf_launch(c, d_src, d_dst, {g})) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BW_OK;
}

extern "C" int bw_gf_matmul(bw_ctx* c, const uint8_t* matrix, uint32_t rows, uint32_t cols, const uint8_t* src,
                            const uint64_t* src_off, const uint64_t* src_len, uint8_t* dst, const uint64_t* dst_off,
                            uint64_t len) {
    if (!c || !rows || !cols || cols > 255 || !matrix || !src_off || !src_len || !dst_off) return BW_EINVAL;
    if (!len) return BW_OK;
    if (!src || !dst) return BW_EINVAL;
    hipSetDevice(c->device);
    // the sources packed 16-aligned in front of the destinations' extent, in one device buffer
    std::vector<uint64_t> so(cols);
    uint64_t at = 0, d_end = 0;
    for (uint32_t s = 0; s < cols; s++) {
        so[s] = at;
        at += (std::min(src_len[s], len) + 15) & ~15ull;
    }
    for (uint32_t r = 0; r < rows; r++) d_end = std::max(d_end, dst_off[r] + len);
    if (int rc = ensure(c, c->gf_io, at + d_end + 16)) return rc;
    uint8_t* b = P<uint8_t>(c->gf_io);
    const GfCall g{matrix, rows, cols, so.data(), src_len, dst_off, len};
    if (int rc = gf_validate(c, b, b + at, g)) return rc;
    for (uint32_t s = 0; s < cols; s++)
        if (std::min(src_len[s], len))
            HIPCHK(c, hipMemcpyAsync(b + so[s], src + src_off[s], std::min(src_len[s], len), hipMemcpyHostToDevice, c->stream));
    if (int rc = gf_launch(c, b, b + at, {g})) return rc;
    for (uint32_t r = 0; r < rows; r++)
        HIPCHK(c, hipMemcpyAsync(dst + dst_off[r], b + at + dst_off[r], len, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BW_OK;
}

// ------------------------------------------------------------------ C ABI: plan and build
extern "C" int bw_parity_plan(const uint64_t* sizes, uint64_t n_pf, uint32_t k, uint32_t m, bw_parity_group* out, uint64_t cap,
                              uint64_t* n_groups, uint64_t* out_bytes) {
    if (!k || !m || (uint64_t)k + m > 256 || !n_groups || !out_bytes || (n_pf && !sizes)) return BW_EINVAL;
    for (uint64_t p = 0; p < n_pf; p++)
        if (!sizes[p]) return BW_EINVAL;
    const uint64_t ng = (n_pf + k - 1) / k;
    uint64_t at = 0;
    for (uint64_t g = 0; g < ng; g++) {
        const uint64_t first = g * k, kk = std::min<uint64_t>(k, n_pf - first);
        uint64_t len = 0;
        for (uint64_t j = 0; j < kk; j++) len = std::max(len, sizes[first + j]);
        len = (len + 15) & ~15ull;
        if (g < cap && out) out[g] = bw_parity_group{first, (uint32_t)kk, m, len, at};
        at += len * m;
    }
    *n_groups = ng;
    *out_bytes = at;
    return ng > cap || (ng && !out) ? BW_ENOSPC : BW_OK;
}

extern "C" int bw_parity_build_device(bw_ctx* c, const uint8_t* d_pf, const bw_packfile* pf, uint64_t n_pf,
                                      const bw_parity_group* groups, uint64_t n_groups, uint8_t* d_out, uint64_t out_cap,
                                      uint8_t* digests) {
    if (!c || !n_groups || !groups || !pf || !n_pf || !d_pf || !d_out || !digests || ((uintptr_t)d_out & 15)) return BW_EINVAL;
    uint64_t n_shards = 0;
    for (uint64_t g = 0; g < n_groups; g++) {
        const bw_parity_group& G = groups[g];
        bool ok = group_ok(G) && G.first_packfile < n_pf && G.k <= n_pf - G.first_packfile && !(G.out_offset & 15) &&
                  G.out_offset <= out_cap && G.shard_len <= (out_cap - G.out_offset) / G.m;
        for (uint32_t j = 0; ok && j < G.k; j++) {
            const uint64_t size = pf[G.first_packfile + j].size;
            ok = size && size <= G.shard_len;
        }
        if (!ok) {
            c->err = "parity: group " + std::to_string(g) + " does not fit the packfile table or the output";
            return BW_EINVAL;
        }
        n_shards += G.k + G.m;
    }
    hipSetDevice(c->device);
    // per group: the Cauchy rows, the members as sources, the parity shards as destinations
    std::vector<std::vector<uint8_t>> mats(n_groups);
    std::vector<std::vector<uint64_t>> tabs(n_groups);
    std::vector<GfCall> calls(n_groups);
    std::vector<uint64_t> h_off, h_len, p_off, p_len;  // what is hashed: data shards, parity shards
    std::vector<uint64_t> d_at, p_at;                   // their positions in `digests`
    uint64_t at = 0;
    for (uint64_t g = 0; g < n_groups; g++) {
        const bw_parity_group& G = groups[g];
        mats[g].resize((uint64_t)G.m * G.k);
        tabs[g].resize(2 * (uint64_t)G.k + G.m);
        for (uint32_t i = 0; i < G.m; i++)
            for (uint32_t j = 0; j < G.k; j++) mats[g][(uint64_t)i * G.k + j] = cauchy(G.m, i, j);
        for (uint32_t j = 0; j < G.k; j++) {
            const bw_packfile& f = pf[G.first_packfile + j];
            tabs[g][j] = f.offset;
            tabs[g][G.k + j] = f.size;
            h_off.push_back(f.offset);
            h_len.push_back(f.size);
            d_at.push_back(at++);
        }
        for (uint32_t i = 0; i < G.m; i++) {
            tabs[g][2 * (uint64_t)G.k + i] = G.out_offset + (uint64_t)i * G.shard_len;
            p_off.push_back(tabs[g][2 * (uint64_t)G.k + i]);
            p_len.push_back(G.shard_len);
            p_at.push_back(at++);
        }
        calls[g] = GfCall{mats[g].data(), G.m, G.k, &tabs[g][0], &tabs[g][G.k], &tabs[g][2 * (uint64_t)G.k], G.shard_len};
        if (int rc = gf_validate(c, d_pf, d_out, calls[g])) return rc;
    }
    {  // parity shards of different groups must not overlap either
        std::vector<std::pair<uint64_t, uint64_t>> r;
        for (uint64_t g = 0; g < n_groups; g++) r.push_back({groups[g].out_offset, groups[g].shard_len * groups[g].m});
        std::sort(r.begin(), r.end());
        for (uint64_t g = 1; g < n_groups; g++)
            if (r[g - 1].first + r[g - 1].second > r[g].first) {
                c->err = "parity: the groups' outputs overlap";
                return BW_EINVAL;
            }
    }
    if (int rc = gf_launch(c, d_pf, d_out, calls)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the hash pass may use other streams of the context
    std::vector<uint8_t> dh(32 * h_off.size()), ph(32 * p_off.size());
    if (int rc = hash_ranges(c, d_pf, h_off.data(), h_len.data(), h_off.size(), dh.data())) return rc;
    if (int rc = hash_ranges(c, d_out, p_off.data(), p_len.data(), p_off.size(), ph.data())) return rc;
    for (uint64_t i = 0; i < d_at.size(); i++) memcpy(digests + 32 * d_at[i], &dh[32 * i], 32);
    for (uint64_t i = 0; i < p_at.size(); i++) memcpy(digests + 32 * p_at[i], &ph[32 * i], 32);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BW_OK;
}

extern "C" int bw_parity_build(bw_ctx* c, const uint8_t* data, const bw_packfile* pf, uint64_t n_pf,
                               const bw_parity_group* groups, uint64_t n_groups, uint8_t* out, uint64_t out_cap,
                               uint8_t* digests) {
    if (!c || !n_groups || !groups || !pf || !n_pf || !data || !out || !digests) return BW_EINVAL;
    hipSetDevice(c->device);
    const uint64_t end = store_extent(pf, n_pf);
    const uint64_t at = (end + 255) & ~255ull;
    if (int rc = ensure(c, c->gf_io, at + out_cap + 16)) return rc;
    uint8_t* b = P<uint8_t>(c->gf_io);
    for (uint64_t p = 0; p < n_pf; p++)
        if (pf[p].size)
            HIPCHK(c, hipMemcpyAsync(b + pf[p].offset, data + pf[p].offset, pf[p].size, hipMemcpyHostToDevice, c->stream));
    if (int rc = bw_parity_build_device(c, b, pf, n_pf, groups, n_groups, b + at, out_cap, digests)) return rc;
    for (uint64_t g = 0; g < n_groups; g++)
        HIPCHK(c, hipMemcpyAsync(out + groups[g].out_offset, b + at + groups[g].out_offset, groups[g].shard_len * groups[g].m,
                                 hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BW_OK;
}

// ------------------------------------------------------------------ C ABI: solve and repair
extern "C" int bw_parity_solve(uint32_t k, uint32_t m, const uint8_t* present, uint32_t* used, uint32_t* missing,
                               uint32_t* n_missing, uint8_t* matrix) {
    if (!k || !m || (uint64_t)k + m > 256 || !present || !used || !missing || !n_missing || !matrix) return BW_EINVAL;
    const GfTables& F = gf();
    const uint32_t n = k + m;
    uint32_t nu = 0, nm = 0;
    for (uint32_t s = 0; s < k; s++)
        if (present[s]) used[nu++] = s;
    for (uint32_t s = k; s < n && nu < k; s++)
        if (present[s]) used[nu++] = s;
    for (uint32_t s = 0; s < n; s++)
        if (!present[s]) missing[nm++] = s;
    *n_missing = nm;
    if (nu < k) return BW_ETOOFEW;
    // row s of the generator [I; C]
    auto gen = [&](uint32_t s, uint32_t j) -> uint8_t { return s < k ? (uint8_t)(s == j) : cauchy(m, s - k, j); };
    // A = the used rows; [A | I] -> [I | A^-1]: data = A^-1 * inputs
    std::vector<uint8_t> a((uint64_t)k * 2 * k, 0);
    const uint64_t w = 2ull * k;
    for (uint32_t r = 0; r < k; r++) {
        for (uint32_t j = 0; j < k; j++) a[r * w + j] = gen(used[r], j);
        a[r * w + k + r] = 1;
    }
    for (uint32_t col = 0; col < k; col++) {
        uint32_t p = col;
        while (p < k && !a[p * w + col]) p++;
        if (p == k) return BW_EINVAL;  // cannot happen: every k rows of [I; C] are independent
        if (p != col)
            for (uint64_t j = 0; j < w; j++) std::swap(a[col * w + j], a[p * w + j]);
        const uint8_t iv = F.inv(a[col * w + col]);
        for (uint64_t j = 0; j < w; j++) a[col * w + j] = F.mul(iv, a[col * w + j]);
        for (uint32_t r = 0; r < k; r++) {
            const uint8_t f = a[r * w + col];
            if (r == col || !f) continue;
            for (uint64_t j = 0; j < w; j++) a[r * w + j] ^= F.mul(f, a[col * w + j]);
        }
    }
    // a missing data shard is its row of A^-1; a missing parity shard its Cauchy row times A^-1
    for (uint32_t r = 0; r < nm; r++) {
        const uint32_t s = missing[r];
        for (uint32_t j = 0; j < k; j++) {
            uint8_t v = 0;
            if (s < k) {
                v = a[s * w + k + j];
            } else {
                for (uint32_t t = 0; t < k; t++) v ^= F.mul(cauchy(m, s - k, t), a[t * w + k + j]);
            }
            matrix[(uint64_t)r * k + j] = v;
        }
    }
    return BW_OK;
}

extern "C" int bw_parity_repair_device(bw_ctx* c, const bw_parity_group* group, const uint8_t* present_in, const uint8_t* d_shards,
                                       const uint64_t* shard_off, const uint64_t* shard_size, const uint8_t* digests,
                                       uint8_t* d_out, const uint64_t* out_off, uint8_t* status) {
    if (!c || !group || !present_in || !shard_off || !shard_size || !out_off || !status) return BW_EINVAL;
    const bw_parity_group& G = *group;
    if (!group_ok(G)) return BW_EINVAL;
    const uint32_t k = G.k, n = G.k + G.m;
    for (uint32_t s = 0; s < n; s++)
        if (s < k ? (!shard_size[s] || shard_size[s] > G.shard_len) : shard_size[s] != G.shard_len) {
            c->err = "parity: shard " + std::to_string(s) + " has a size its group cannot hold";
            return BW_EINVAL;
        }
    hipSetDevice(c->device);
    std::vector<uint8_t> present(present_in, present_in + n), demoted(n, 0);
    for (uint32_t s = 0; s < n; s++) {
        present[s] = present[s] != 0;
        status[s] = BW_PARITY_OK;
    }
    bool any = false;
    for (uint32_t s = 0; s < n; s++) any = any || present[s];
    if (any && !d_shards) return BW_EINVAL;
    if (digests && any) {  // a damaged survivor must never be an input
        std::vector<uint64_t> idx, off, len;
        for (uint32_t s = 0; s < n; s++)
            if (present[s]) {
                idx.push_back(s);
                off.push_back(shard_off[s]);
                len.push_back(shard_size[s]);
            }
        std::vector<uint8_t> h(32 * idx.size());
        if (int rc = hash_ranges(c, d_shards, off.data(), len.data(), idx.size(), h.data())) return rc;
        for (uint64_t i = 0; i < idx.size(); i++)
            if (memcmp(&h[32 * i], digests + 32 * idx[i], 32)) {
                present[idx[i]] = 0;
                demoted[idx[i]] = 1;
            }
    }
    std::vector<uint32_t> used(k), missing(n);
    std::vector<uint8_t> matrix((uint64_t)n * k);
    uint32_t nm = 0;
    const int rc = bw_parity_solve(k, G.m, present.data(), used.data(), missing.data(), &nm, matrix.data());
    if (rc == BW_ETOOFEW) {
        for (uint32_t r = 0; r < nm; r++) status[missing[r]] = BW_PARITY_LOST;
        return BW_OK;
    }
    if (rc) return rc;
    if (!nm) return BW_OK;
    if (!d_out) return BW_EINVAL;
    std::vector<uint64_t> so(k), sl(k), dof(nm);
    for (uint32_t j = 0; j < k; j++) {
        so[j] = shard_off[used[j]];
        sl[j] = shard_size[used[j]];
    }
    for (uint32_t r = 0; r < nm; r++) dof[r] = out_off[missing[r]];
    const GfCall g{matrix.data(), nm, k, so.data(), sl.data(), dof.data(), G.shard_len};
    if (int rc2 = gf_validate(c, d_shards, d_out, g)) return rc2;
    if (int rc2 = gf_launch(c, d_shards, d_out, {g})) return rc2;
    for (uint32_t r = 0; r < nm; r++) status[missing[r]] = demoted[missing[r]] ? BW_PARITY_DAMAGED : BW_PARITY_REBUILT;
    // a rebuilt data shard is zero beyond its size, or an input was not what was encoded
    std::vector<GfRange> tails;
    std::vector<uint32_t> tail_of;
    for (uint32_t r = 0; r < nm; r++)
        if (shard_size[missing[r]] < G.shard_len) {
            tails.push_back(GfRange{dof[r] + shard_size[missing[r]], G.shard_len - shard_size[missing[r]]});
            tail_of.push_back(missing[r]);
        }
    if (!tails.empty()) {
        const uint64_t nt = tails.size(), flag_at = (nt * sizeof(GfRange) + 15) & ~15ull;
        HIPCHK(c, hipStreamSynchronize(c->stream));  // k_gf_matmul still reads gf_tab
        if (int rc2 = ensure(c, c->gf_tab, flag_at + 4 * nt)) return rc2;
        uint8_t* t = P<uint8_t>(c->gf_tab);
        std::vector<uint32_t> flags(nt);
        HIPCHK(c, hipMemcpyAsync(t, tails.data(), nt * sizeof(GfRange), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(t + flag_at, 0, 4 * nt, c->stream));
        hipLaunchKernelGGL(k_gf_nonzero, dim3((unsigned)nt), dim3(64), 0, c->stream, d_out, (const GfRange*)t,
                           (uint32_t*)(t + flag_at));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(flags.data(), t + flag_at, 4 * nt, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (uint64_t i = 0; i < nt; i++)
            if (flags[i]) status[tail_of[i]] = BW_PARITY_REBUILT_BAD;
    }
    if (digests) {
        std::vector<uint64_t> len(nm);
        for (uint32_t r = 0; r < nm; r++) len[r] = shard_size[missing[r]];
        std::vector<uint8_t> h(32 * (uint64_t)nm);
        if (int rc2 = hash_ranges(c, d_out, dof.data(), len.data(), nm, h.data())) return rc2;
        for (uint32_t r = 0; r < nm; r++)
            if (memcmp(&h[32 * (uint64_t)r], digests + 32 * (uint64_t)missing[r], 32)) status[missing[r]] = BW_PARITY_REBUILT_BAD;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BW_OK;
}

extern "C" int bw_parity_repair(bw_ctx* c, const bw_parity_group* group, const uint8_t* present, const uint8_t* shards,
                                const uint64_t* shard_off, const uint64_t* shard_size, const uint8_t* digests, uint8_t* out,
                                const uint64_t* out_off, uint8_t* status) {
    if (!c || !group || !present || !shard_off || !shard_size || !out_off || !status) return BW_EINVAL;
    if (!group_ok(*group)) return BW_EINVAL;
    const uint32_t n = group->k + group->m;
    hipSetDevice(c->device);
    // the present shards packed 16-aligned, then the outputs' extent
    std::vector<uint64_t> so(n, 0);
    uint64_t at = 0, o_end = 0;
    for (uint32_t s = 0; s < n; s++) {
        if (shard_size[s] > group->shard_len) return BW_EINVAL;
        if (present[s]) {
            if (!shards) return BW_EINVAL;
            so[s] = at;
            at += (shard_size[s] + 15) & ~15ull;
        }
        o_end = std::max(o_end, out_off[s] + group->shard_len);
    }
    if (int rc = ensure(c, c->gf_io, at + o_end + 16)) return rc;
    uint8_t* b = P<uint8_t>(c->gf_io);
    for (uint32_t s = 0; s < n; s++)
        if (present[s] && shard_size[s])
            HIPCHK(c, hipMemcpyAsync(b + so[s], shards + shard_off[s], shard_size[s], hipMemcpyHostToDevice, c->stream));
    if (int rc = bw_parity_repair_device(c, group, present, b, so.data(), shard_size, digests, b + at, out_off, status)) return rc;
    for (uint32_t s = 0; s < n; s++)
        if (status[s] == BW_PARITY_DAMAGED || status[s] == BW_PARITY_REBUILT || status[s] == BW_PARITY_REBUILT_BAD) {
            if (!out) return BW_EINVAL;
            HIPCHK(c, hipMemcpyAsync(out + out_off[s], b + at + out_off[s], group->shard_len, hipMemcpyDeviceToHost, c->stream));
        }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BW_OK;
}
