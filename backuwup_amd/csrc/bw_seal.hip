// bw_seal.hip -- per-blob sealing on gfx950: HKDF-SHA-256 key derivation + AES-256-GCM.
//
// Replaces the encryption half of Manager::compress_encrypt_blob (client/src/backup/filesystem/
// packfile/pack.rs:70-80):
//     key  = KEYS.derive_backup_key(&blob.hash)      key_manager.rs:80-86:
//            Hkdf::<Sha256>::from_prk(backup_secret_key).expand(info, [0u8; 32])
//     data = Aes256Gcm::new(key).encrypt_in_place(nonce, b"", data)   -> ciphertext || tag
// and its inverse (unpack.rs:58-63, blob_index.rs:185-191).  Crates aes-gcm 0.10 / hkdf 0.12 /
// sha2 0.10: standard AES-256, GCM with a 96-bit nonce and a 128-bit tag, RFC 5869 HKDF-Expand
// (L = 32 is one HMAC-SHA-256 block: T(1) = HMAC(prk, info || 0x01)).
//
//   k_seal_prep  one lane per item: HMAC-SHA-256 (the pads' states come from the host), AES-256
//                key schedule, H = E(0), E(J0), and the GHASH multipliers H^(2^k) (k <= 5),
//                H^64 and H^PIECE_BLOCKS.
//   k_seal_ctr   one wave per piece (up to PIECE_BLOCKS 16-byte blocks of one item): CTR
//                keystream + xor, and the piece's GHASH partial.  Lane l takes blocks
//                l, l+64, l+128, ... (every load and store is a coalesced 1 KiB per wave); each
//                lane runs Horner with the multiplier H^64 (Shoup 8-bit table in LDS, built per
//                piece), and a 6-level shuffle tree folds the 64 lane partials with H^(2^k)
//                (Shoup 4-bit tables).  AES is T-table: Te0 and Te1 as 32 lane replicas per
//                256-byte row at LDS address 0, so one v_perm_b32 forms a conflict-free lookup
//                address and Te1 is the same address + 128 (ds_read offset); Te2/Te3 are one
//                rotation of (Te0 ^ Te1) terms.
//   k_seal_tag   one lane per item: folds the piece partials with H^PIECE_BLOCKS (pieces are
//                cut from the item's end, so only the first is ragged), appends the length block and masks with E(J0); sealing
//                stores the tag after the ciphertext, opening compares it (ok flag).
//   k_seal_auth  the GHASH half of k_seal_ctr alone: tags recomputed, nothing decrypted (check).
//   k_reseal_ctr, k_reseal_tag
//                k_seal_ctr and k_seal_tag with two keys: ciphertext under one key to ciphertext under
//                another in one pass, both GHASH side by side, no plaintext stored (rekey).
//
// The three piece kernels (k_seal_ctr, k_seal_auth, k_reseal_ctr) differ in their block loops only
// (two, four and two-by-two blocks in flight; round keys in registers, none, in LDS).  What is the same
// is written once: piece_of (piece -> item and blocks), GhashLds (the GHASH tables of a workgroup, a
// member of each kernel's LDS struct) with gmul_h64 / gmul_t4 / ghash_wave_tables / ghash_wave_fold,
// seal_lds_init (the workgroup's tables), load_block / store_block, and for the tag kernels
// seal_tag_words (and tag_store / tag_diff in k_seal_tag).  launch_seal(st, SealMode, ...) and launch_reseal (bw_seal.h)
// are the entry points; piece_grid is the one grid formula.
//
// GF(2^128) elements are four big-endian words w0..w3 of the block (GCM bit order: the MSB of
// w0 is the coefficient of x^0); multiplication by x is a right shift by one with 0xE1 << 120
// folded in.
#include "bw_device.h"
#include "bw_internal.h"
#include "bw_seal.h"

#include <stdlib.h>
#include <string.h>

#include <type_traits>
#include <utility>

namespace bw {

// ------------------------------------------------------------------ SHA-256 (FIPS 180-4)
// the 64 round constants, once: for the kernels (k_seal_prep) and for the host (seal_pads)
#define BW_SHA256_K                                                                                     \
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,     \
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,     \
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,     \
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,     \
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,     \
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,     \
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,     \
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2
__constant__ uint32_t c_k256[64] = {BW_SHA256_K};
static const uint32_t h_k256[64] = {BW_SHA256_K};

__host__ __device__ __forceinline__ uint32_t ror32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

template <typename KT>
__host__ __device__ __forceinline__ void sha256_compress(uint32_t h[8], const uint32_t in[16], const KT& K) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = in[i];
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], k = h[7];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        uint32_t wi;
        if (i < 16) {
            wi = w[i];
        } else {
            const uint32_t x = w[(i - 15) & 15], y = w[(i - 2) & 15];
            const uint32_t s0 = ror32(x, 7) ^ ror32(x, 18) ^ (x >> 3);
            const uint32_t s1 = ror32(y, 17) ^ ror32(y, 19) ^ (y >> 10);
            wi = w[i & 15] = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
        }
        const uint32_t t1 = k + (ror32(e, 6) ^ ror32(e, 11) ^ ror32(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + wi;
        const uint32_t t2 = (ror32(a, 2) ^ ror32(a, 13) ^ ror32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        k = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += k;
}

// ------------------------------------------------------------------ GF(2^128), GCM bit order
struct G4 {
    uint32_t w0, w1, w2, w3;
};

__device__ __forceinline__ G4 gxor(G4 a, G4 b) { return {a.w0 ^ b.w0, a.w1 ^ b.w1, a.w2 ^ b.w2, a.w3 ^ b.w3}; }

__device__ __forceinline__ G4 gmulx(G4 v) {
    const uint32_t lsb = v.w3 & 1;
    G4 r;
    r.w3 = __builtin_amdgcn_alignbit(v.w2, v.w3, 1);
    r.w2 = __builtin_amdgcn_alignbit(v.w1, v.w2, 1);
    r.w1 = __builtin_amdgcn_alignbit(v.w0, v.w1, 1);
    r.w0 = (v.w0 >> 1) ^ (lsb ? 0xe1000000u : 0u);
    return r;
}

// bitwise X * Y (SP 800-38D Algorithm 1): setup and the tag fold only, never per data block
__device__ G4 gmul_slow(G4 x, G4 y) {
    G4 z = {0, 0, 0, 0}, v = y;
    const uint32_t xw[4] = {x.w0, x.w1, x.w2, x.w3};
#pragma unroll
    for (int k = 0; k < 4; k++)
        for (int b = 31; b >= 0; b--) {
            const uint32_t m = 0u - ((xw[k] >> b) & 1u);
            z.w0 ^= v.w0 & m; z.w1 ^= v.w1 & m; z.w2 ^= v.w2 & m; z.w3 ^= v.w3 & m;
            v = gmulx(v);
        }
    return z;
}

// ------------------------------------------------------------------ AES-256 helpers
__device__ __forceinline__ uint32_t gf8_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        r ^= (b & 1) ? a : 0;
        a = ((a << 1) ^ ((a & 0x80) ? 0x1b : 0)) & 0xff;
        b >>= 1;
    }
    return r;
}

// FIPS-197 S-box: affine map of the multiplicative inverse (x^254 in GF(2^8); 0 -> 0)
__device__ uint32_t aes_sbox(uint32_t x) {
    uint32_t x2 = gf8_mul(x, x), x3 = gf8_mul(x2, x), x6 = gf8_mul(x3, x3), x7 = gf8_mul(x6, x);
    uint32_t x14 = gf8_mul(x7, x7), x15 = gf8_mul(x14, x), x30 = gf8_mul(x15, x15), x31 = gf8_mul(x30, x);
    uint32_t x62 = gf8_mul(x31, x31), x63 = gf8_mul(x62, x), x126 = gf8_mul(x63, x63), x127 = gf8_mul(x126, x);
    const uint32_t inv = gf8_mul(x127, x127);  // x^254
    uint32_t s = inv, r = inv;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        r = ((r << 1) | (r >> 7)) & 0xff;
        s ^= r;
    }
    return s ^ 0x63;
}

// Te0[x] = (2s, s, s, 3s) big-endian, s = S[x]
__device__ __forceinline__ uint32_t aes_te0(uint32_t s) {
    const uint32_t s2 = ((s << 1) ^ ((s & 0x80) ? 0x1b : 0)) & 0xff;
    return (s2 << 24) | (s << 16) | (s << 8) | (s2 ^ s);
}

__device__ __forceinline__ void st4(uint32_t* d, G4 v) { d[0] = v.w0; d[1] = v.w1; d[2] = v.w2; d[3] = v.w3; }
__device__ __forceinline__ G4 ld4(const uint32_t* s) { return {s[0], s[1], s[2], s[3]}; }

// plain (unreplicated) T-table AES for the prep kernel
__device__ void aes_encrypt_plain(const uint32_t rk[60], const uint32_t* te, const uint32_t in[4], uint32_t out[4]) {
    uint32_t s0 = in[0] ^ rk[0], s1 = in[1] ^ rk[1], s2 = in[2] ^ rk[2], s3 = in[3] ^ rk[3];
#define TE(x, r) ror32(te[(x) & 0xff], (r))
    for (int r = 1; r < 14; r++) {
        const uint32_t t0 = TE(s0 >> 24, 0) ^ TE(s1 >> 16, 8) ^ TE(s2 >> 8, 16) ^ TE(s3, 24) ^ rk[4 * r];
        const uint32_t t1 = TE(s1 >> 24, 0) ^ TE(s2 >> 16, 8) ^ TE(s3 >> 8, 16) ^ TE(s0, 24) ^ rk[4 * r + 1];
        const uint32_t t2 = TE(s2 >> 24, 0) ^ TE(s3 >> 16, 8) ^ TE(s0 >> 8, 16) ^ TE(s1, 24) ^ rk[4 * r + 2];
        const uint32_t t3 = TE(s3 >> 24, 0) ^ TE(s0 >> 16, 8) ^ TE(s1 >> 8, 16) ^ TE(s2, 24) ^ rk[4 * r + 3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
#undef TE
#define SB(x) ((te[(x) & 0xff] >> 16) & 0xff)
    out[0] = ((SB(s0 >> 24) << 24) | (SB(s1 >> 16) << 16) | (SB(s2 >> 8) << 8) | SB(s3)) ^ rk[56];
    out[1] = ((SB(s1 >> 24) << 24) | (SB(s2 >> 16) << 16) | (SB(s3 >> 8) << 8) | SB(s0)) ^ rk[57];
    out[2] = ((SB(s2 >> 24) << 24) | (SB(s3 >> 16) << 16) | (SB(s0 >> 8) << 8) | SB(s1)) ^ rk[58];
    out[3] = ((SB(s3 >> 24) << 24) | (SB(s0 >> 16) << 16) | (SB(s1 >> 8) << 8) | SB(s2)) ^ rk[59];
#undef SB
}

// ------------------------------------------------------------------ k_seal_prep
__global__ __launch_bounds__(256) void k_seal_prep(const SealItem* __restrict__ items, uint64_t n, SealPads pads,
                                                   SealKey* __restrict__ keys) {
    __shared__ uint32_t s_te[256];
    s_te[threadIdx.x] = aes_te0(aes_sbox(threadIdx.x));
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SealItem& it = items[i];
    // HMAC inner: SHA-256(K ^ ipad || info || 0x01), the ipad block already compressed
    uint32_t m[16];
#pragma unroll
    for (int w = 0; w < 16; w++) m[w] = 0;
    const uint32_t il = it.info_len;
    for (uint32_t k = 0; k < il; k++) m[k >> 2] |= (uint32_t)it.info[k] << (24 - 8 * (k & 3));
    m[il >> 2] |= 0x01u << (24 - 8 * (il & 3));
    m[(il + 1) >> 2] |= 0x80u << (24 - 8 * ((il + 1) & 3));
    m[15] = (64 + il + 1) * 8;
    uint32_t h[8];
#pragma unroll
    for (int w = 0; w < 8; w++) h[w] = pads.istate[w];
    sha256_compress(h, m, c_k256);
    // HMAC outer: SHA-256(K ^ opad || inner)
#pragma unroll
    for (int w = 0; w < 8; w++) m[w] = h[w];
    m[8] = 0x80000000u;
#pragma unroll
    for (int w = 9; w < 15; w++) m[w] = 0;
    m[15] = (64 + 32) * 8;
#pragma unroll
    for (int w = 0; w < 8; w++) h[w] = pads.ostate[w];
    sha256_compress(h, m, c_k256);
    // AES-256 key schedule: the key bytes are the HMAC output, big-endian words
    uint32_t rk[60];
#pragma unroll
    for (int w = 0; w < 8; w++) rk[w] = h[w];
    uint32_t rcon = 1;
#pragma unroll
    for (int w = 8; w < 60; w++) {
        uint32_t t = rk[w - 1];
        if (w % 8 == 0 || w % 8 == 4) {
            if (w % 8 == 0) t = (t << 8) | (t >> 24);  // RotWord
            t = (((s_te[t >> 24] >> 16) & 0xff) << 24) | (((s_te[(t >> 16) & 0xff] >> 16) & 0xff) << 16) |
                (((s_te[(t >> 8) & 0xff] >> 16) & 0xff) << 8) | ((s_te[t & 0xff] >> 16) & 0xff);  // SubWord
            if (w % 8 == 0) {
                t ^= rcon << 24;
                rcon = ((rcon << 1) ^ ((rcon & 0x80) ? 0x1b : 0)) & 0xff;
            }
        }
        rk[w] = rk[w - 8] ^ t;
    }
    SealKey& K = keys[i];
#pragma unroll
    for (int w = 0; w < 60; w++) K.rk[w] = rk[w];
    const uint32_t zero[4] = {0, 0, 0, 0};
    const uint32_t j0[4] = {it.nonce[0], it.nonce[1], it.nonce[2], 1u};
    uint32_t hb[4], e0[4];
    {
        const uint32_t a0 = it.nonce[0] ^ rk[0], a1 = it.nonce[1] ^ rk[1], a2 = it.nonce[2] ^ rk[2];
#define TE(x, r) ror32(s_te[(x) & 0xff], (r))
        K.R1[0] = TE(a0 >> 24, 0) ^ TE(a1 >> 16, 8) ^ TE(a2 >> 8, 16) ^ rk[4];
        K.R1[1] = TE(a1 >> 24, 0) ^ TE(a2 >> 16, 8) ^ TE(a0, 24) ^ rk[5];
        K.R1[2] = TE(a2 >> 24, 0) ^ TE(a0 >> 8, 16) ^ TE(a1, 24) ^ rk[6];
        K.R1[3] = TE(a0 >> 16, 8) ^ TE(a1 >> 8, 16) ^ TE(a2, 24) ^ rk[7];
#undef TE
    }
    aes_encrypt_plain(rk, s_te, zero, hb);
    aes_encrypt_plain(rk, s_te, j0, e0);
    const G4 H = {hb[0], hb[1], hb[2], hb[3]};
    st4(K.H, H);
    st4(K.E0, {e0[0], e0[1], e0[2], e0[3]});
    G4 p = H;
    for (int k = 0; k < 6; k++) {
        st4(K.P[k], p);
        p = gmul_slow(p, p);
    }
    st4(K.H64, p);  // H^64
    for (uint32_t e = 64; e < PIECE_BLOCKS; e <<= 1) p = gmul_slow(p, p);
    st4(K.HP, p);
}

// ------------------------------------------------------------------ what the piece kernels share
// k_seal_ctr, k_seal_auth and k_reseal_ctr: the piece walk, the workgroup's LDS tables, block loads and
// stores, GHASH.  Their block loops stay their own.

// Piece p of the call: the item that owns it (wave-uniform), and the piece's 16-byte blocks
// [b0, b0 + q) of that item's len bytes.
struct Piece {
    uint64_t item, len, b0;
    uint32_t q;
};

__device__ __forceinline__ Piece piece_of(const SealItem* __restrict__ items, uint64_t n_items, uint64_t p) {
    // item owning piece p (items[].piece0 ascending)
    uint64_t lo = 0, hi = n_items;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (items[mid].piece0 <= p) lo = mid + 1;
        else hi = mid;
    }
    const uint64_t ii = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(lo - 1));
    const SealItem& it = items[ii];
    const uint64_t len = it.len, m = (len + 15) / 16;
    // pieces are cut from the end: the first takes the ragged remainder, so every later piece is
    // full and k_seal_tag folds them with the one multiplier H^PIECE_BLOCKS
    const uint64_t pi = p - it.piece0, np = (m + PIECE_BLOCKS - 1) / PIECE_BLOCKS;
    const uint64_t first = m - (np - 1) * PIECE_BLOCKS;
    return {ii, len, pi == 0 ? 0 : first + (pi - 1) * PIECE_BLOCKS, (uint32_t)(pi == 0 ? first : PIECE_BLOCKS)};
}

// The GHASH tables of a workgroup: SETS per-wave table sets (one per wave; two in k_reseal_ctr) and
// the reductions all of them share.
template <int SETS>
struct GhashLds {
    uint32_t gt[SETS][256][4];    // [set][byte] Shoup 8-bit table of H^64 (contiguous: random bytes spread the banks)
    uint32_t g4[SETS][6][16][4];  // [set][level][nibble] Shoup 4-bit tables of H^(2^k)
    uint32_t r8[256], r4[16];     // reduction of 8 / 4 shifted-out bits (xor into w0)
};

// The AES table of a workgroup: [byte][Te0 x 32 replicas | Te1 x 32 replicas].  It is the first member
// of the LDS struct that holds it, at LDS address 0 (te_at).
typedef uint32_t SealTe[256][64];

template <typename LT, typename = void>
struct lds_has_te : std::false_type {};
template <typename LT>
struct lds_has_te<LT, decltype((void)std::declval<LT&>().te)> : std::true_type {};

// The shared tables of a workgroup of THREADS >= 256 threads whose LDS is L (a GhashLds g, and a SealTe
// te where the kernel runs AES): r8 / r4, and the S-box -> Te0 / Te1 replicas; visible to the
// workgroup on return.
template <int THREADS, typename LT>
__device__ __forceinline__ void seal_lds_init(LT& L) {
    static_assert(THREADS >= 256, "te, r8 and r4 are filled by the first 256 lanes");
    const uint32_t tid = threadIdx.x;
    if (tid < 256) {
        if constexpr (lds_has_te<LT>::value) {
            const uint32_t t0 = aes_te0(aes_sbox(tid));
            L.te[tid][0] = t0;
            L.te[tid][32] = ror32(t0, 8);
        }
        G4 v = {0, 0, 0, tid};
        for (int k = 0; k < 8; k++) {
            v = gmulx(v);
            if (k == 3 && tid < 16) L.g.r4[tid] = v.w0;
        }
        L.g.r8[tid] = v.w0;
    }
    __syncthreads();
    if constexpr (lds_has_te<LT>::value) {
        for (uint32_t e = tid; e < 256 * 64; e += THREADS) {
            const uint32_t row = e >> 6, col = e & 63;
            if (col != 0 && col != 32) L.te[row][col] = L.te[row][col < 32 ? 0 : 32];
        }
        __syncthreads();
    }
}

#define SEAL_SEL(k) (0x0c0c0000u | ((4u + (k)) << 8))          // (byte k of w) << 8 | lane_off

template <int OFF>
__device__ __forceinline__ uint32_t te_at(const SealTe& te, uint32_t addr) {
    return *(const uint32_t*)((const uint8_t*)&te[0][0] + addr + OFF);
}

// Two AES-256 encryptions of counter blocks (n0, n1, n2, ctr), words big-endian, interleaved so
// one block's LDS lookups overlap the other's xors.  Round 1 starts from r1 (its nonce-word
// terms, precomputed per item): only the counter word's four lookups remain.  rk: 60 words, in
// registers (k_seal_ctr) or in LDS (k_reseal_ctr).
__device__ __forceinline__ void aes_ctr2(const SealTe& te, const uint32_t* rk, const uint32_t* r1, uint32_t lane_off,
                                         uint32_t ca, uint32_t cb, uint32_t oa[4], uint32_t ob[4]) {
#define A0(w, k) te_at<0>(te, __builtin_amdgcn_perm((w), lane_off, SEAL_SEL(k)))
#define A1(w, k) te_at<128>(te, __builtin_amdgcn_perm((w), lane_off, SEAL_SEL(k)))
#define R16(x) __builtin_amdgcn_alignbit((x), (x), 16)
    uint32_t a0, a1, a2, a3, b0, b1, b2, b3;
    {
        const uint32_t xa = ca ^ rk[3], xb = cb ^ rk[3];
        a0 = r1[0] ^ R16(A1(xa, 0)); b0 = r1[0] ^ R16(A1(xb, 0));
        a1 = r1[1] ^ R16(A0(xa, 1)); b1 = r1[1] ^ R16(A0(xb, 1));
        a2 = r1[2] ^ A1(xa, 2);      b2 = r1[2] ^ A1(xb, 2);
        a3 = r1[3] ^ A0(xa, 3);      b3 = r1[3] ^ A0(xb, 3);
    }
#define COL(s0, s1, s2, s3, r) (A0(s0, 3) ^ A1(s1, 2) ^ R16(A0(s2, 1) ^ A1(s3, 0)) ^ (r))
#pragma unroll
    for (int r = 2; r < 14; r++) {
        const uint32_t ta0 = COL(a0, a1, a2, a3, rk[4 * r]), tb0 = COL(b0, b1, b2, b3, rk[4 * r]);
        const uint32_t ta1 = COL(a1, a2, a3, a0, rk[4 * r + 1]), tb1 = COL(b1, b2, b3, b0, rk[4 * r + 1]);
        const uint32_t ta2 = COL(a2, a3, a0, a1, rk[4 * r + 2]), tb2 = COL(b2, b3, b0, b1, rk[4 * r + 2]);
        const uint32_t ta3 = COL(a3, a0, a1, a2, rk[4 * r + 3]), tb3 = COL(b3, b0, b1, b2, rk[4 * r + 3]);
        a0 = ta0; a1 = ta1; a2 = ta2; a3 = ta3;
        b0 = tb0; b1 = tb1; b2 = tb2; b3 = tb3;
    }
    // last round: S-box bytes (byte 2 of Te0 and byte 0 of Te1 are S[x]), assembled by v_perm
#define LAST(s0, s1, s2, s3, r) \
    ((__builtin_amdgcn_perm(A0(s0, 3), A0(s1, 2), 0x06020c0cu) | __builtin_amdgcn_perm(A1(s2, 1), A1(s3, 0), 0x0c0c0400u)) ^ (r))
    oa[0] = LAST(a0, a1, a2, a3, rk[56]); ob[0] = LAST(b0, b1, b2, b3, rk[56]);
    oa[1] = LAST(a1, a2, a3, a0, rk[57]); ob[1] = LAST(b1, b2, b3, b0, rk[57]);
    oa[2] = LAST(a2, a3, a0, a1, rk[58]); ob[2] = LAST(b2, b3, b0, b1, rk[58]);
    oa[3] = LAST(a3, a0, a1, a2, rk[59]); ob[3] = LAST(b3, b0, b1, b2, rk[59]);
#undef LAST
#undef COL
#undef R16
#undef A1
#undef A0
}

// Byte f of the zstd store frame of the raw_len bytes at s (FHD 0x00, window descriptor, raw
// blocks of <= 128 KiB behind 3-byte headers with the last-block bit).
__device__ __forceinline__ uint32_t frame_byte(const uint8_t* s, uint32_t raw_len, uint32_t wd, uint32_t f) {
    if (f == 0) return 0;  // Frame_Header_Descriptor: no content size, no checksum, no dictionary
    if (f == 1) return wd;
    const uint32_t nb = raw_len ? (raw_len + ZSTD_BLOCK - 1) / ZSTD_BLOCK : 1;
    const uint32_t k = (f - 2) / ZSTD_STRIDE, r = (f - 2) - k * ZSTD_STRIDE;
    if (r < 3) {
        const uint32_t bl = k == nb - 1 ? raw_len - k * ZSTD_BLOCK : ZSTD_BLOCK;
        return (((bl << 3) | (k == nb - 1 ? 1u : 0u)) >> (8 * r)) & 0xff;  // Raw_Block
    }
    return s[(uint64_t)k * ZSTD_BLOCK + r - 3];
}

// Block g of the len bytes at s as big-endian words, zero-padded past the item's end (as GHASH
// takes it); a full block is one 16-byte load at whatever byte s + 16 g is.
__device__ __forceinline__ G4 load_block(const uint8_t* s, uint64_t len, uint64_t g) {
    const uint64_t at = 16 * g;
    if (at + 16 <= len) {
        const uint4 v = *(const uint4*)(s + at);
        return {__builtin_bswap32(v.x), __builtin_bswap32(v.y), __builtin_bswap32(v.z), __builtin_bswap32(v.w)};
    }
    const uint32_t nb = (uint32_t)(len - at);
    uint32_t in[4];
#pragma unroll
    for (int w = 0; w < 4; w++) {
        uint32_t x = 0;
#pragma unroll
        for (int b = 0; b < 4; b++)
            if ((uint32_t)(4 * w + b) < nb) x |= (uint32_t)s[at + 4 * w + b] << (24 - 8 * b);
        in[w] = x;
    }
    return {in[0], in[1], in[2], in[3]};
}

// Block g of an item of len bytes at d from the words out: one 16-byte store, or the bytes of the
// ragged last block, after which out is masked to what was stored (the words GHASH will see).
__device__ __forceinline__ void store_block(uint8_t* d, uint64_t len, uint64_t g, uint32_t out[4]) {
    const uint64_t at = 16 * g;
    if (at + 16 <= len) {
        *(uint4*)(d + at) = make_uint4(__builtin_bswap32(out[0]), __builtin_bswap32(out[1]), __builtin_bswap32(out[2]),
                                       __builtin_bswap32(out[3]));
    } else {
        const uint32_t nb = (uint32_t)(len - at);
        for (uint32_t b = 0; b < nb; b++) d[at + b] = (uint8_t)(out[b >> 2] >> (24 - 8 * (b & 3)));
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int v = (int)nb - 4 * w;  // valid bytes of word w (big-endian)
            out[w] &= v >= 4 ? ~0u : (v <= 0 ? 0u : ~0u << (32 - 8 * v));
        }
    }
}

// CTR xor of block g of the item (keystream ks) from s to d; returns the GHASH input (the
// ciphertext, zero-padded past the end of the item).  FRAMED: the plaintext is the store frame
// of the raw bytes at s; a block inside one raw block's data is one (unaligned) 16-byte load.
template <bool DEC, bool FRAMED>
__device__ __forceinline__ G4 crypt_block(const uint8_t* s, uint8_t* d, uint64_t len, uint64_t g, const uint32_t ks[4],
                                          uint32_t raw_len, uint32_t wd) {
    const uint64_t at = 16 * g;
    uint32_t in[4];
    const bool full = at + 16 <= len;
    if (FRAMED) {
        const uint32_t f = (uint32_t)at;
        const uint32_t k0 = f >= 2 ? (f - 2) / ZSTD_STRIDE : 0, r0 = f >= 2 ? (f - 2) - k0 * ZSTD_STRIDE : 0;
        if (full && f >= 2 && r0 >= 3 && r0 + 16 <= ZSTD_STRIDE) {
            const uint4 v = *(const uint4*)(s + (uint64_t)k0 * ZSTD_BLOCK + r0 - 3);
            in[0] = __builtin_bswap32(v.x); in[1] = __builtin_bswap32(v.y);
            in[2] = __builtin_bswap32(v.z); in[3] = __builtin_bswap32(v.w);
        } else {
            const uint32_t nb = full ? 16 : (uint32_t)(len - at);
#pragma unroll
            for (int w = 0; w < 4; w++) {
                uint32_t x = 0;
#pragma unroll
                for (int b = 0; b < 4; b++)
                    if ((uint32_t)(4 * w + b) < nb) x |= frame_byte(s, raw_len, wd, f + 4 * w + b) << (24 - 8 * b);
                in[w] = x;
            }
        }
    } else {
        const G4 v = load_block(s, len, g);
        in[0] = v.w0; in[1] = v.w1; in[2] = v.w2; in[3] = v.w3;
    }
    uint32_t out[4];
#pragma unroll
    for (int w = 0; w < 4; w++) out[w] = in[w] ^ ks[w];
    store_block(d, len, g, out);
    const uint32_t* c = DEC ? in : out;  // GHASH runs over the ciphertext
    return {c[0], c[1], c[2], c[3]};
}

// Z = X * H^64 with table set `set`'s 8-bit table: Horner over the bytes of X from the last
template <int SETS>
__device__ __forceinline__ G4 gmul_h64(const GhashLds<SETS>& L, G4 x, uint32_t set) {
    const uint8_t* gbase = (const uint8_t*)&L.gt[set][0][0];
    const uint32_t xw[4] = {x.w0, x.w1, x.w2, x.w3};
    G4 z = {0, 0, 0, 0};
#pragma unroll
    for (int i = 15; i >= 0; i--) {
        if (i != 15) {
            const uint32_t rem = z.w3 & 0xff;
            z.w3 = __builtin_amdgcn_alignbyte(z.w2, z.w3, 1);
            z.w2 = __builtin_amdgcn_alignbyte(z.w1, z.w2, 1);
            z.w1 = __builtin_amdgcn_alignbyte(z.w0, z.w1, 1);
            z.w0 = (z.w0 >> 8) ^ L.r8[rem];
        }
        const uint32_t b = (xw[i >> 2] >> (8 * (3 - (i & 3)))) & 0xff;
        const uint4 m = *(const uint4*)(gbase + (b << 4));
        z.w0 ^= m.x; z.w1 ^= m.y; z.w2 ^= m.z; z.w3 ^= m.w;
    }
    return z;
}

// Z = X * T with a 4-bit table (16 entries)
template <int SETS>
__device__ __forceinline__ G4 gmul_t4(const GhashLds<SETS>& L, G4 x, const uint32_t (*t)[4]) {
    const uint32_t xw[4] = {x.w0, x.w1, x.w2, x.w3};
    G4 z = {0, 0, 0, 0};
#pragma unroll
    for (int i = 31; i >= 0; i--) {
        if (i != 31) {
            const uint32_t rem = z.w3 & 0xf;
            z.w3 = __builtin_amdgcn_alignbit(z.w2, z.w3, 4);
            z.w2 = __builtin_amdgcn_alignbit(z.w1, z.w2, 4);
            z.w1 = __builtin_amdgcn_alignbit(z.w0, z.w1, 4);
            z.w0 = (z.w0 >> 4) ^ L.r4[rem];
        }
        const uint32_t nib = (xw[i >> 3] >> (28 - 4 * (i & 7))) & 0xf;
        const uint4 m = *(const uint4*)t[nib];
        z.w0 ^= m.x; z.w1 ^= m.y; z.w2 ^= m.z; z.w3 ^= m.w;
    }
    return z;
}

__device__ __forceinline__ G4 shfl_down4(G4 v, int d) {
    return {(uint32_t)__shfl_down((int)v.w0, d, 64), (uint32_t)__shfl_down((int)v.w1, d, 64),
            (uint32_t)__shfl_down((int)v.w2, d, 64), (uint32_t)__shfl_down((int)v.w3, d, 64)};
}

// table set wid (this wave's own) for the item of K: 8-bit Shoup table of H^64 (4 entries per lane),
// 4-bit tables of H^(2^k); visible to the whole wave on return
template <int SETS>
__device__ __forceinline__ void ghash_wave_tables(GhashLds<SETS>& L, const SealKey& K, uint32_t wid, uint32_t lane) {
    G4 basis[8];
    basis[0] = ld4(K.H64);
#pragma unroll
    for (int j = 1; j < 8; j++) basis[j] = gmulx(basis[j - 1]);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t b = lane + 64 * r;
        G4 e = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (b & (0x80u >> j)) e = gxor(e, basis[j]);
        st4(L.gt[wid][b], e);
    }
    for (uint32_t pr = lane; pr < 96; pr += 64) {
        const uint32_t k = pr >> 4, nib = pr & 15;
        G4 v = ld4(K.P[k]), e = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (nib & (0x8u >> j)) e = gxor(e, v);
            v = gmulx(v);
        }
        st4(L.g4[wid][k][nib], e);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// fold the 64 lane partials: T = sum_l X_l * H^(63 - l), in lane 0
template <int SETS>
__device__ __forceinline__ G4 ghash_wave_fold(const GhashLds<SETS>& L, G4 X, uint32_t wid, uint32_t lane) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const G4 y = shfl_down4(X, 1 << k);
        const G4 t = gmul_t4(L, X, L.g4[wid][k]);
        if ((lane & ((2u << k) - 1)) == 0) X = gxor(t, y);
    }
    return X;
}

// ------------------------------------------------------------------ k_seal_ctr
struct SealLds {
    SealTe te;
    GhashLds<SEAL_THREADS / 64> g;  // a table set per wave
};
static_assert(offsetof(SealLds, te) == 0, "te_at: te at LDS address 0");
static_assert(sizeof(SealLds) == 156736, "k_seal_ctr's LDS");

template <bool DEC, bool FRAMED>
__global__ __launch_bounds__(SEAL_THREADS) void k_seal_ctr(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                           const SealItem* __restrict__ items, uint64_t n_items,
                                                           const SealKey* __restrict__ keys, uint64_t n_pieces,
                                                           uint32_t* __restrict__ parts) {
    __shared__ __attribute__((aligned(16))) SealLds L;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    seal_lds_init<SEAL_THREADS>(L);
    const uint32_t lane_off = (lane & 31) * 4;

    for (uint64_t p = (uint64_t)blockIdx.x * (SEAL_THREADS / 64) + wid; p < n_pieces;
         p += (uint64_t)gridDim.x * (SEAL_THREADS / 64)) {
        const Piece pc = piece_of(items, n_items, p);
        const SealItem& it = items[pc.item];
        const SealKey& K = keys[pc.item];
        const uint64_t len = pc.len, b0 = pc.b0;
        ghash_wave_tables(L.g, K, wid, lane);

        uint32_t rk[60];
#pragma unroll
        for (int w = 0; w < 60; w++) rk[w] = K.rk[w];
        const uint8_t* s = src + it.src_off;
        uint8_t* d = dst + it.dst_off;
        const uint32_t S = (pc.q + 63) / 64, pad = 64 * S - pc.q;
        G4 X = {0, 0, 0, 0};
        uint32_t r1[4];
#pragma unroll
        for (int w = 0; w < 4; w++) r1[w] = K.R1[w];
        // two blocks per lane per step (j, j + 1): their AES runs interleaved, GHASH stays in order
        for (uint32_t j = 0; j < S; j += 2) {
            const int32_t ra = (int32_t)(lane + 64 * j) - (int32_t)pad;  // >= -63; rb = ra + 64 >= 1
            const uint64_t ga = b0 + (uint32_t)(ra < 0 ? 0 : ra), gb = b0 + (uint32_t)(ra + 64);
            uint32_t ksa[4], ksb[4];
            aes_ctr2(L.te, rk, r1, lane_off, (uint32_t)(ga + 2), (uint32_t)(gb + 2), ksa, ksb);  // inc32 of J0 = nonce||1
            if (j) X = gmul_h64(L.g, X, wid);
            if (ra >= 0) X = gxor(X, crypt_block<DEC, FRAMED>(s, d, len, ga, ksa, it.raw_len, it.wd));
            if (j + 1 < S) {  // wave-uniform
                X = gmul_h64(L.g, X, wid);
                X = gxor(X, crypt_block<DEC, FRAMED>(s, d, len, gb, ksb, it.raw_len, it.wd));
            }
        }
        X = ghash_wave_fold(L.g, X, wid, lane);
        if (lane == 0) st4(parts + 4 * p, X);
        __builtin_amdgcn_wave_barrier();  // the tables are rebuilt for the next piece
    }
}

// ------------------------------------------------------------------ k_seal_auth
// The GHASH half of k_seal_ctr<true, false> alone: the same pieces, the same 64-lane Horner scheme
// and the same partials, so k_seal_prep and k_seal_tag<true> serve it unchanged -- but no AES, so no
// Te replicas in LDS, no round keys in registers, no keystream and no store but the piece's partial.
// The LDS holds the GHASH tables only (5.5 KiB per wave); WAVES per workgroup is the occupancy
// choice (launch_seal).
template <int WAVES>
struct AuthLds {
    GhashLds<WAVES> g;  // a table set per wave
};
static_assert(sizeof(AuthLds<8>) == 46144 && sizeof(AuthLds<16>) == 91200, "k_seal_auth's LDS");

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_seal_auth(const uint8_t* __restrict__ src,
                                                          const SealItem* __restrict__ items, uint64_t n_items,
                                                          const SealKey* __restrict__ keys, uint64_t n_pieces,
                                                          uint32_t* __restrict__ parts) {
    __shared__ __attribute__((aligned(16))) AuthLds<WAVES> L;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    seal_lds_init<64 * WAVES>(L);

    for (uint64_t p = (uint64_t)blockIdx.x * WAVES + wid; p < n_pieces; p += (uint64_t)gridDim.x * WAVES) {
        const Piece pc = piece_of(items, n_items, p);
        const SealItem& it = items[pc.item];
        const SealKey& K = keys[pc.item];
        const uint64_t len = pc.len, b0 = pc.b0;
        ghash_wave_tables(L.g, K, wid, lane);

        const uint8_t* s = src + it.src_off;
        const uint32_t S = (pc.q + 63) / 64, pad = 64 * S - pc.q;
        G4 X = {0, 0, 0, 0};
        // lane l takes blocks l - pad + 64 j: four loads in flight per lane, GHASH in order
        for (uint32_t j = 0; j < S; j += 4) {
            G4 c[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int32_t r = (int32_t)(lane + 64 * (j + u)) - (int32_t)pad;  // < 0 only for j + u == 0
                c[u] = {0, 0, 0, 0};
                if (j + u < S && r >= 0) c[u] = load_block(s, len, b0 + (uint32_t)r);
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (j + u < S) {  // wave-uniform
                    if (j + u) X = gmul_h64(L.g, X, wid);
                    X = gxor(X, c[u]);
                }
        }
        X = ghash_wave_fold(L.g, X, wid, lane);
        if (lane == 0) st4(parts + 4 * p, X);
        __builtin_amdgcn_wave_barrier();  // the tables are rebuilt for the next piece
    }
}

// ------------------------------------------------------------------ k_reseal_ctr
// One pass from the ciphertext under one key to the ciphertext under another: c' = c ^ ks_old ^ ks_new,
// where the two keystreams are xored before the ciphertext meets them, so no plaintext byte exists
// even in a register, and the GHASH of c (the old tag) and of c' (the new one) run side by side.  The
// pieces, the lanes' blocks and the partials are k_seal_ctr's; every source byte is loaded once and
// every output byte stored once.
//
// What does not fit k_seal_ctr's shape: a second GHASH table set per wave
// (SealLds at 16 waves is 153 KiB of 160) and a second key schedule (120 wave-uniform words are more
// than the scalar file holds).  So a workgroup has RESEAL_WAVES = 8 waves, each with two table sets
// (slot 2 wid: old, 2 wid + 1: new), and both schedules lie in LDS beside them: a round's four words
// are one 16-byte read at a wave-uniform address (a broadcast, no bank conflict) next to the round's
// 64 table lookups.  Four AES blocks (two blocks x two keys) are in flight per lane, which gives the
// two waves a SIMD holds the independent LDS reads that four waves give k_seal_ctr.
struct ResealLds {
    SealTe te;
    GhashLds<2 * RESEAL_WAVES> g;      // table set 2 wave + side
    uint32_t rk[RESEAL_WAVES][2][60];  // [wave][side] AES-256 round keys
};
static_assert(offsetof(ResealLds, te) == 0, "te_at: te at LDS address 0");
static_assert(sizeof(ResealLds) == 160576, "k_reseal_ctr's LDS: one workgroup per CU");

// block g of the item: cin = the ciphertext at s (what the old tag covers), cout = cin ^ kx, stored
// to d (what the new tag covers); both zero-padded past the item's end
__device__ __forceinline__ void reseal_block(const uint8_t* s, uint8_t* d, uint64_t len, uint64_t g, const uint32_t kx[4],
                                             G4& cin, G4& cout) {
    cin = load_block(s, len, g);
    uint32_t out[4] = {cin.w0 ^ kx[0], cin.w1 ^ kx[1], cin.w2 ^ kx[2], cin.w3 ^ kx[3]};
    store_block(d, len, g, out);
    cout = {out[0], out[1], out[2], out[3]};
}

// items: the geometry (src_off, len, dst_off, piece0; the old nonces); keys_o / keys_n: k_seal_prep's
// output under the old and the new PRK (and nonces); parts_o / parts_n: a partial per piece each
__global__ __launch_bounds__(64 * RESEAL_WAVES) void k_reseal_ctr(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                  const SealItem* __restrict__ items, uint64_t n_items,
                                                                  const SealKey* __restrict__ keys_o,
                                                                  const SealKey* __restrict__ keys_n, uint64_t n_pieces,
                                                                  uint32_t* __restrict__ parts_o,
                                                                  uint32_t* __restrict__ parts_n) {
    __shared__ __attribute__((aligned(16))) ResealLds L;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    seal_lds_init<64 * RESEAL_WAVES>(L);
    const uint32_t lane_off = (lane & 31) * 4;
    const uint32_t so = 2 * wid, sn = 2 * wid + 1;

    for (uint64_t p = (uint64_t)blockIdx.x * RESEAL_WAVES + wid; p < n_pieces; p += (uint64_t)gridDim.x * RESEAL_WAVES) {
        const Piece pc = piece_of(items, n_items, p);
        const SealItem& it = items[pc.item];
        const SealKey& Ko = keys_o[pc.item];
        const SealKey& Kn = keys_n[pc.item];
        const uint64_t len = pc.len, b0 = pc.b0;
        if (lane < 60) {
            L.rk[wid][0][lane] = Ko.rk[lane];
            L.rk[wid][1][lane] = Kn.rk[lane];
        }
        ghash_wave_tables(L.g, Ko, so, lane);
        ghash_wave_tables(L.g, Kn, sn, lane);  // its barrier publishes the round keys too

        const uint8_t* s = src + it.src_off;
        uint8_t* d = dst + it.dst_off;
        const uint32_t S = (pc.q + 63) / 64, pad = 64 * S - pc.q;
        G4 Xo = {0, 0, 0, 0}, Xn = {0, 0, 0, 0};
        uint32_t r1o[4], r1n[4];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            r1o[w] = Ko.R1[w];
            r1n[w] = Kn.R1[w];
        }
        for (uint32_t j = 0; j < S; j += 2) {
            const int32_t ra = (int32_t)(lane + 64 * j) - (int32_t)pad;  // >= -63; rb = ra + 64 >= 1
            const uint64_t ga = b0 + (uint32_t)(ra < 0 ? 0 : ra), gb = b0 + (uint32_t)(ra + 64);
            uint32_t ka[4], kb[4], na[4], nb[4];
            // an offset the compiler cannot see through, taken per step: the round keys are read from
            // LDS where a round uses them, not hoisted out of the loop into 120 registers
            uint32_t zo = 0;
            asm volatile("" : "+v"(zo));
            const uint32_t* rko = L.rk[wid][0] + zo;
            const uint32_t* rkn = L.rk[wid][1] + zo;
            aes_ctr2(L.te, rko, r1o, lane_off, (uint32_t)(ga + 2), (uint32_t)(gb + 2), ka, kb);
            aes_ctr2(L.te, rkn, r1n, lane_off, (uint32_t)(ga + 2), (uint32_t)(gb + 2), na, nb);
#pragma unroll
            for (int w = 0; w < 4; w++) {
                ka[w] ^= na[w];
                kb[w] ^= nb[w];
            }
            G4 ci, co;
            if (j) {
                Xo = gmul_h64(L.g, Xo, so);
                Xn = gmul_h64(L.g, Xn, sn);
            }
            if (ra >= 0) {
                reseal_block(s, d, len, ga, ka, ci, co);
                Xo = gxor(Xo, ci);
                Xn = gxor(Xn, co);
            }
            if (j + 1 < S) {  // wave-uniform
                Xo = gmul_h64(L.g, Xo, so);
                Xn = gmul_h64(L.g, Xn, sn);
                reseal_block(s, d, len, gb, kb, ci, co);
                Xo = gxor(Xo, ci);
                Xn = gxor(Xn, co);
            }
        }
        Xo = ghash_wave_fold(L.g, Xo, so, lane);
        Xn = ghash_wave_fold(L.g, Xn, sn, lane);
        if (lane == 0) {
            st4(parts_o + 4 * p, Xo);
            st4(parts_n + 4 * p, Xn);
        }
        __builtin_amdgcn_wave_barrier();  // the tables and the round keys are rebuilt for the next piece
    }
}

// ------------------------------------------------------------------ k_seal_tag
// the tag of one item from its pieces' partials: folded with H^PIECE_BLOCKS, the length block, E(J0)
__device__ __forceinline__ void seal_tag_words(const SealItem& it, const SealKey& K, const uint32_t* __restrict__ parts,
                                               uint32_t tw[4]) {
    const uint64_t len = it.len, m = (len + 15) / 16;
    const uint64_t np = (m + PIECE_BLOCKS - 1) / PIECE_BLOCKS;
    const G4 H = ld4(K.H);
    G4 acc = {0, 0, 0, 0};
    const G4 HP = ld4(K.HP);
    for (uint64_t pi = 0; pi < np; pi++) {
        const G4 T = ld4(parts + 4 * (it.piece0 + pi));
        acc = pi == 0 ? T : gxor(gmul_slow(acc, HP), T);  // every piece after the first is full
    }
    const uint64_t bits = len * 8;
    const G4 Lb = {0, 0, (uint32_t)(bits >> 32), (uint32_t)bits};
    G4 y = gmul_slow(gxor(gmul_slow(acc, H), Lb), H);
    y = gxor(y, ld4(K.E0));
    tw[0] = y.w0; tw[1] = y.w1; tw[2] = y.w2; tw[3] = y.w3;
}

// the 16 tag bytes at t from the words tw, each xored with flip
__device__ __forceinline__ void tag_store(uint8_t* t, const uint32_t tw[4], uint8_t flip) {
    for (int b = 0; b < 16; b++) t[b] = (uint8_t)(tw[b >> 2] >> (24 - 8 * (b & 3))) ^ flip;
}

// nonzero when the 16 tag bytes at t are not the words tw (every byte is compared)
__device__ __forceinline__ uint32_t tag_diff(const uint8_t* t, const uint32_t tw[4]) {
    uint32_t diff = 0;
    for (int b = 0; b < 16; b++) diff |= t[b] ^ (uint8_t)(tw[b >> 2] >> (24 - 8 * (b & 3)));
    return diff;
}

// k_seal_tag<true> and k_seal_tag<false> in one lane: the old tag is compared, and the new tag is
// stored behind the new ciphertext where it matched and complemented where it did not, so an item
// that was not authentic under the old key is not authentic under the new one either
__global__ __launch_bounds__(256) void k_reseal_tag(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                    const SealItem* __restrict__ items, uint64_t n,
                                                    const SealKey* __restrict__ keys_o, const SealKey* __restrict__ keys_n,
                                                    const uint32_t* __restrict__ parts_o, const uint32_t* __restrict__ parts_n,
                                                    uint8_t* __restrict__ ok) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SealItem& it = items[i];
    uint32_t to[4], tn[4];
    seal_tag_words(it, keys_o[i], parts_o, to);
    seal_tag_words(it, keys_n[i], parts_n, tn);
    // tag_diff and tag_store, written out: through the helpers this kernel's scalar register count changes
    const uint8_t* t = src + it.src_off + it.len;
    uint32_t diff = 0;
    for (int b = 0; b < 16; b++) diff |= t[b] ^ (uint8_t)(to[b >> 2] >> (24 - 8 * (b & 3)));
    const uint8_t flip = diff ? 0xff : 0;
    uint8_t* u = dst + it.dst_off + it.len;
    for (int b = 0; b < 16; b++) u[b] = (uint8_t)(tn[b >> 2] >> (24 - 8 * (b & 3))) ^ flip;
    ok[i] = diff == 0;
}

template <bool DEC>
__global__ __launch_bounds__(256) void k_seal_tag(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                  const SealItem* __restrict__ items, uint64_t n,
                                                  const SealKey* __restrict__ keys, const uint32_t* __restrict__ parts,
                                                  uint8_t* __restrict__ ok) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SealItem& it = items[i];
    uint32_t tw[4];
    seal_tag_words(it, keys[i], parts, tw);
    if (!DEC) tag_store(dst + it.dst_off + it.len, tw, 0);
    else ok[i] = tag_diff(src + it.src_off + it.len, tw) == 0;
}

// ------------------------------------------------------------------ host side
void seal_pads(const uint8_t prk[32], SealPads* pads) {
    uint32_t blk[16];
    for (int pass = 0; pass < 2; pass++) {
        const uint8_t x = pass ? 0x5c : 0x36;
        for (int w = 0; w < 16; w++) {
            uint32_t v = 0;
            for (int b = 0; b < 4; b++) {
                const int k = 4 * w + b;
                v |= (uint32_t)((k < 32 ? prk[k] : 0) ^ x) << (24 - 8 * b);
            }
            blk[w] = v;
        }
        uint32_t* st = pass ? pads->ostate : pads->istate;
        const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                                0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
        for (int w = 0; w < 8; w++) st[w] = iv[w];
        sha256_compress(st, blk, h_k256);
    }
}

uint64_t seal_pieces(uint64_t len) {
    const uint64_t m = (len + 15) / 16;
    return (m + PIECE_BLOCKS - 1) / PIECE_BLOCKS;
}

void seal_fill_item(SealItem* it, uint64_t src_off, uint64_t len, uint64_t dst_off, uint64_t piece0,
                    const uint8_t nonce[12], const uint8_t* info, uint32_t info_len) {
    memset(it, 0, sizeof(SealItem));
    it->src_off = src_off;
    it->len = len;
    it->dst_off = dst_off;
    it->piece0 = piece0;
    for (int w = 0; w < 3; w++)
        it->nonce[w] = (uint32_t)nonce[4 * w] << 24 | (uint32_t)nonce[4 * w + 1] << 16 |
                       (uint32_t)nonce[4 * w + 2] << 8 | nonce[4 * w + 3];
    it->info_len = info_len;
    memcpy(it->info, info, info_len);
}

uint32_t zstd_window_descriptor(uint64_t raw_len) {
    uint32_t wlog = raw_len > 1 ? 64 - __builtin_clzll(raw_len - 1) : 0;  // ceil(log2(raw_len))
    wlog = wlog < 10 ? 10 : (wlog > 21 ? 21 : wlog);  // level 3's windowLog, cut to the source size
    return (wlog - 10) << 3;
}

// The piece kernels' grid for workgroups of `waves` waves (a piece per wave and pass): a pass over
// the grid covers at most 16,384 pieces, whatever the workgroup's size.
static dim3 piece_grid(uint64_t n_pieces, uint64_t waves) {
    const uint64_t need = (n_pieces + waves - 1) / waves, cap = 16384 / waves;
    return dim3((unsigned)(need < cap ? need : cap));
}
static_assert(16384 % (SEAL_THREADS / 64) == 0 && 16384 % SEAL_AUTH_WAVES == 0 && 16384 % RESEAL_WAVES == 0,
              "a pass is a whole number of workgroups");

static dim3 item_grid(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }  // k_seal_prep, k_seal_tag: a lane per item

// k_seal_auth's workgroup: SEAL_AUTH_WAVES = 8 waves (44.6 KiB of LDS; at 109 VGPRs two of them are
// resident per CU, the 16 waves one 16-wave workgroup gives).  BW_SEAL_AUTH_WAVES=16 selects the
// one-workgroup-per-CU shape of k_seal_ctr for A/B runs (tools/check_bench.py; measured slower,
// DESIGN.md section 5).
static bool auth_wide() {
    static const bool wide = [] {
        const char* e = getenv("BW_SEAL_AUTH_WAVES");
        return e && atoi(e) == 16;
    }();
    return wide;
}

void launch_seal(hipStream_t st, SealMode mode, const uint8_t* src, uint8_t* dst, const SealItem* it, uint64_t n,
                 const SealPads& pads, SealKey* k, uint64_t n_pieces, uint32_t* parts, uint8_t* ok) {
    if (!n) return;
    hipLaunchKernelGGL(k_seal_prep, item_grid(n), dim3(256), 0, st, it, n, pads, k);
    const dim3 grid = piece_grid(n_pieces, SEAL_THREADS / 64), block(SEAL_THREADS);
    if (n_pieces) switch (mode) {
        case SealMode::Seal:
            hipLaunchKernelGGL((k_seal_ctr<false, false>), grid, block, 0, st, src, dst, it, n, k, n_pieces, parts);
            break;
        case SealMode::SealFramed:
            hipLaunchKernelGGL((k_seal_ctr<false, true>), grid, block, 0, st, src, dst, it, n, k, n_pieces, parts);
            break;
        case SealMode::Open:
            hipLaunchKernelGGL((k_seal_ctr<true, false>), grid, block, 0, st, src, dst, it, n, k, n_pieces, parts);
            break;
        case SealMode::Auth:
            if (auth_wide())
                hipLaunchKernelGGL(k_seal_auth<16>, piece_grid(n_pieces, 16), dim3(64 * 16), 0, st, src, it, n, k, n_pieces,
                                   parts);
            else
                hipLaunchKernelGGL(k_seal_auth<SEAL_AUTH_WAVES>, piece_grid(n_pieces, SEAL_AUTH_WAVES),
                                   dim3(64 * SEAL_AUTH_WAVES), 0, st, src, it, n, k, n_pieces, parts);
            break;
    }
    if (mode == SealMode::Seal || mode == SealMode::SealFramed)
        hipLaunchKernelGGL(k_seal_tag<false>, item_grid(n), dim3(256), 0, st, src, dst, it, n, k, parts, ok);
    else
        hipLaunchKernelGGL(k_seal_tag<true>, item_grid(n), dim3(256), 0, st, src, dst, it, n, k, parts, ok);
}

// The entry point bw_internal.h declares, which no code calls any more: that header is part of the
// profiled hot path's source digest (backuwup_amd/build.py), so the declaration stays as it is until a
// change that re-stamps the PMC evidence removes it together with this forwarder.
void launch_seal(hipStream_t st, bool dec, bool framed, const uint8_t* src, uint8_t* dst, const SealItem* it,
                 uint64_t n, const SealPads& pads, SealKey* k, uint64_t n_pieces, uint32_t* parts, uint8_t* ok) {
    launch_seal(st, dec ? SealMode::Open : (framed ? SealMode::SealFramed : SealMode::Seal), src, dst, it, n, pads, k, n_pieces, parts, ok);
}

void launch_reseal(hipStream_t st, const uint8_t* src, uint8_t* dst, const SealItem* it_o, const SealItem* it_n, uint64_t n,
                   const SealPads& pads_o, const SealPads& pads_n, SealKey* k_o, SealKey* k_n, uint64_t n_pieces,
                   uint32_t* parts_o, uint32_t* parts_n, uint8_t* ok) {
    if (!n) return;
    hipLaunchKernelGGL(k_seal_prep, item_grid(n), dim3(256), 0, st, it_o, n, pads_o, k_o);
    hipLaunchKernelGGL(k_seal_prep, item_grid(n), dim3(256), 0, st, it_n, n, pads_n, k_n);
    if (n_pieces)
        hipLaunchKernelGGL(k_reseal_ctr, piece_grid(n_pieces, RESEAL_WAVES), dim3(64 * RESEAL_WAVES), 0, st, src, dst, it_o, n,
                           k_o, k_n, n_pieces, parts_o, parts_n);
    hipLaunchKernelGGL(k_reseal_tag, item_grid(n), dim3(256), 0, st, src, dst, it_o, n, k_o, k_n, parts_o, parts_n, ok);
}

}  // namespace bw
