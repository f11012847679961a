// bw_zstd_dec.hip -- zstd frame decoding on the GPU (the read side): the
// decompression of Manager::get_blob (unpack.rs:65-67) for a batch of magicless frames, and the
// parse of opened packfile headers (unpack.rs:47-48).
//
// k_zd_frame: one wave per frame (a workgroup is one wave; a grid of at most ZD_MAX_WAVES waves
// strides over the batch).  Every lane runs the serial driver of bw_zstd_dec_core.h with the same
// inputs, so control flow is uniform; the frame's tables live in LDS (zd::State + zd::Scratch,
// about 11 KiB per wave), the Huffman streams of a block are decoded by lanes 0-3 into a 128 KiB
// literals buffer per wave, and every copy -- raw and RLE blocks, literals, matches -- is done by
// all 64 lanes.  A match whose source was written since the wave's last barrier waits for those
// stores first; matches that reach further back (most of them, in text) do not.
// All bounds checks are the core's: they run before the copy they guard.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bw_device.h"
#include "bw_internal.h"
#include "bw_unpack.h"
#include "bw_zstd_dec_core.h"

namespace bw {

namespace {

struct __attribute__((packed, aligned(1))) Vec16 {
    uint32_t a, b, c, d;
};

// The execution policy of a wave (see bw_zstd_dec_core.h).
struct WaveExec {
    uint32_t lane;
    zd::Hazard hz;  // what the wave stored since its last barrier

    template <class F>
    __device__ void for_streams(uint32_t n, F f) {
        if (lane < n) f(lane);
    }
    __device__ int any(int v) { return __any(v != 0) ? 1 : 0; }
    __device__ void sync() {
        __syncthreads();
        hz.synced();
    }
    // d and s do not overlap
    __device__ void copy(uint8_t* d, const uint8_t* s, uint32_t n) {
        hz.wrote(d);
        if (n >= 256) {
            const uint32_t head = (uint32_t)(-(uintptr_t)d) & 15u;
            if (lane < head) d[lane] = s[lane];
            d += head;
            s += head;
            n -= head;
            const uint32_t body = n & ~15u;
            for (uint32_t i = lane * 16; i < body; i += 64 * 16) *(Vec16*)(d + i) = *(const Vec16*)(s + i);
            d += body;
            s += body;
            n -= body;
        }
        for (uint32_t i = lane; i < n; i += 64) d[i] = s[i];
    }
    __device__ void fill(uint8_t* d, uint8_t b, uint32_t n) {
        hz.wrote(d);
        for (uint32_t i = lane; i < n; i += 64) d[i] = b;
    }
    // n bytes at d from d - off (off >= 1; the source may run into the bytes being written)
    __device__ void match(uint8_t* d, size_t off, uint32_t n) {
        if (hz.must_wait(d, off, n)) sync();
        const uint8_t* s = d - off;
        if (off >= n) {
            copy(d, s, n);
            return;
        }
        hz.wrote(d);
        const uint32_t o = (uint32_t)off;  // < n <= 128 KiB + 2
        for (uint32_t i = lane; i < n; i += 64) d[i] = s[i % o];
    }
};

}  // namespace

__global__ __launch_bounds__(64) void k_zd_frame(const uint8_t* __restrict__ src, uint8_t* dst, const ZdItem* items,
                                                 uint64_t n, uint8_t* lit, uint64_t* out_len, uint32_t* status) {
    __shared__ zd::State st;
    __shared__ zd::Scratch sc;
    uint8_t* litbuf = lit + (uint64_t)blockIdx.x * ZD_LIT_STRIDE;
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const ZdItem it = items[i];
        WaveExec x{threadIdx.x, {nullptr}};
        size_t got = 0;
        const int e = zd::decode_frame(src + it.src_off, (size_t)it.src_len, dst + it.dst_off, (size_t)it.dst_cap, &st,
                                       &sc, litbuf, &got, x);
        if (threadIdx.x == 0) {
            out_len[i] = got;
            status[i] = (uint32_t)e;
        }
        __syncthreads();  // the next frame rebuilds the tables
    }
}

void launch_zd_frames(hipStream_t st, const uint8_t* src, uint8_t* dst, const ZdItem* items, uint64_t n, uint32_t waves,
                      uint8_t* lit, uint64_t* out_len, uint32_t* status) {
    if (!n) return;
    hipLaunchKernelGGL(k_zd_frame, dim3(waves), dim3(64), 0, st, src, dst, items, n, lit, out_len, status);
}

// ------------------------------------------------------------------ blob nonces
// out[12 k ..] = the 12 bytes at src + off[k] (the nonce in front of sealed blob k, unpack.rs:58)
__global__ void k_gather12(const uint8_t* __restrict__ src, const uint64_t* off, uint64_t n, uint8_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 12 * n) return;
    out[i] = src[off[i / 12] + i % 12];
}

void launch_gather12(hipStream_t st, const uint8_t* src, const uint64_t* off, uint64_t n, uint8_t* out) {
    if (!n) return;
    hipLaunchKernelGGL(k_gather12, dim3((uint32_t)((12 * n + 255) / 256)), dim3(256), 0, st, src, off, n, out);
}

// ------------------------------------------------------------------ packfile headers
// bincode::options().with_varint_encoding().deserialize::<Vec<PackfileHeaderBlob>>(pt)
// (unpack.rs:47-48): a varint count, then per entry hash[32], kind and compression (enum tags, u32
// varints that must name a variant: 0 or 1), length and offset (u64 varints); nothing may follow.
// One thread per packfile; with `out` null only the count is produced (parsed[f] = entries or
// ~0 for a malformed header), otherwise the entries land at out[rec0[f] ..].

__device__ static bool rd_varint(const uint8_t* p, uint64_t len, uint64_t& at, uint64_t max, uint64_t& v) {
    if (at >= len) return false;
    const uint32_t t = p[at++];
    if (t < 251) {
        v = t;
        return v <= max;
    }
    if (t > 253) return false;  // u128 or a reserved tag
    const uint32_t size = t == 251 ? 2 : (t == 252 ? 4 : 8);
    if (size > len - at) return false;
    v = 0;
    for (uint32_t k = 0; k < size; k++) v |= (uint64_t)p[at + k] << (8 * k);
    at += size;
    return v <= max;
}

__global__ void k_unpack_parse(const uint8_t* __restrict__ pt, const uint64_t* pt_off, const uint64_t* pt_len,
                               uint64_t n_files, const uint64_t* rec0, uint64_t* parsed, bw_unpack_entry* out) {
    const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_files) return;
    const uint8_t* p = pt + pt_off[f];
    const uint64_t len = pt_len[f];
    uint64_t at = 0, cnt = 0;
    bool ok = rd_varint(p, len, at, ~0ull, cnt);
    // an entry is at least 36 bytes: a count the plaintext cannot hold is malformed (bincode stops
    // at the end of its input)
    if (ok && cnt > len / 36) ok = false;
    for (uint64_t k = 0; ok && k < cnt; k++) {
        if (len - at < 32) {
            ok = false;
            break;
        }
        const uint8_t* h = p + at;
        at += 32;
        uint64_t kind, comp, length, offset;
        ok = rd_varint(p, len, at, 1, kind) && rd_varint(p, len, at, 1, comp) && rd_varint(p, len, at, ~0ull, length) &&
             rd_varint(p, len, at, ~0ull, offset);
        if (ok && out) {
            bw_unpack_entry& e = out[rec0[f] + k];
            for (int b = 0; b < 32; b++) e.hash[b] = h[b];
            e.packfile = (uint32_t)f;
            e.kind = (uint8_t)kind;
            e.compression = (uint8_t)comp;
            e.pad[0] = e.pad[1] = 0;
            e.length = length;
            e.offset = offset;
        }
    }
    if (ok && at != len) ok = false;  // trailing bytes
    if (!out) parsed[f] = ok ? cnt : ~0ull;
}

void launch_unpack_parse(hipStream_t st, const uint8_t* pt, const uint64_t* pt_off, const uint64_t* pt_len,
                         uint64_t n_files, const uint64_t* rec0, uint64_t* parsed, bw_unpack_entry* out) {
    if (!n_files) return;
    hipLaunchKernelGGL(k_unpack_parse, dim3((uint32_t)((n_files + 63) / 64)), dim3(64), 0, st, pt, pt_off, pt_len, n_files,
                       rec0, parsed, out);
}

}  // namespace bw
