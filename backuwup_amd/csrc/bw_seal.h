// bw_seal.h -- the authenticate-only mode of sealing and reseal (bw_seal.hip), declared apart from
// bw_internal.h: they serve check and rekey, which are off the chunk -> hash -> dedup path
// (backuwup_amd/build.py OFF_PATH).
#pragma once
#include "bw_internal.h"

namespace bw {

constexpr int SEAL_AUTH_WAVES = 8;  // k_seal_auth: waves per workgroup (5.5 KiB of GHASH tables each)

// launch_seal with its third mode.  auth (with dec): the tags are checked and nothing else is
// written: k_seal_prep, then k_seal_auth (GHASH only) in place of k_seal_ctr<true, false>, then
// k_seal_tag<true>; dst is not used.  auth = false is launch_seal as bw_internal.h declares it.
void launch_seal(hipStream_t st, bool dec, bool framed, const uint8_t* src, uint8_t* dst, const SealItem* items,
                 uint64_t n, const SealPads& pads, SealKey* keys, uint64_t n_pieces, uint32_t* parts, uint8_t* ok, bool auth);

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
