// bw_seal.h -- the launchers of bw_seal.hip: seal, open and authenticate through one launch_seal, and
// reseal.  Declared apart from bw_internal.h, whose code is part of the profiled hot path's source
// digest (backuwup_amd/build.py OFF_PATH); the item, key and pad types stay there.
#pragma once
#include "bw_internal.h"

namespace bw {

// What launch_seal does with the items (k_seal_prep first, k_seal_tag last, in every mode):
enum class SealMode {
    Seal,        // dst = ciphertext || tag (k_seal_ctr<false, false>)
    SealFramed,  // Seal, the plaintext being the zstd store frame of the item's raw_len source bytes, built
                 // while it is encrypted (k_seal_ctr<false, true>)
    Open,        // src = ciphertext || tag, dst = plaintext, ok[i] = tag verified (k_seal_ctr<true, false>)
    Auth,        // Open's ok without its plaintext: GHASH only (k_seal_auth); dst is not used
};

constexpr int SEAL_AUTH_WAVES = 8;  // k_seal_auth: waves per workgroup (5.5 KiB of GHASH tables each)

// items[i].len is the plaintext's length in every mode; n_pieces the sum of seal_pieces over them;
// parts holds 16 bytes per piece; ok (n bytes) is written by Open and Auth only.
void launch_seal(hipStream_t st, SealMode mode, const uint8_t* src, uint8_t* dst, const SealItem* items, uint64_t n,
                 const SealPads& pads, SealKey* keys, uint64_t n_pieces, uint32_t* parts, uint8_t* ok);

constexpr int RESEAL_WAVES = 8;  // k_reseal_ctr: waves per workgroup (two GHASH table sets and two key schedules each)

// Reseal (bw_reseal_device): items under the old PRK become the same plaintexts under the new one in
// one pass, c' = c ^ keystream_old ^ keystream_new; no plaintext is stored.  it_o and it_n are the
// same items with the old and the new nonces (one array serves both when the nonces are kept);
// k_seal_prep runs once per side, k_reseal_ctr writes the new ciphertexts and both sides' piece
// partials, k_reseal_tag compares the old tag (ok[i]) and stores the new one, complemented where
// the old one did not verify.
void launch_reseal(hipStream_t st, const uint8_t* src, uint8_t* dst, const SealItem* it_o, const SealItem* it_n, uint64_t n,
                   const SealPads& pads_o, const SealPads& pads_n, SealKey* k_o, SealKey* k_n, uint64_t n_pieces,
                   uint32_t* parts_o, uint32_t* parts_n, uint8_t* ok);

}  // namespace bw

// bw_reseal_device with a HKDF info length per item (info_lens, n x u32; NULL: info_len for all), so
// that packfile headers and blobs go through one launch sequence (bw_rekey.hip).  info holds n rows of
// info_len bytes.
int bw_reseal_items(bw_ctx* ctx, const uint8_t old_prk[32], const uint8_t new_prk[32], const uint8_t* d_src,
                    const uint64_t* src_off, const uint64_t* src_len, uint64_t n, const uint8_t* info, uint32_t info_len,
                    const uint32_t* info_lens, const uint8_t* nonces, const uint8_t* new_nonces, uint8_t* d_dst,
                    const uint64_t* dst_off, uint8_t* ok);
