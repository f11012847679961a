// bw_seal.h -- the authenticate-only mode of sealing (bw_seal.hip), declared apart from bw_internal.h:
// it serves check, which is off the chunk -> hash -> dedup path (backuwup_amd/build.py OFF_PATH).
#pragma once
#include "bw_internal.h"

namespace bw {

constexpr int SEAL_AUTH_WAVES = 8;  // k_seal_auth: waves per workgroup (5.5 KiB of GHASH tables each)

// launch_seal with its third mode.  auth (with dec): the tags are checked and nothing else is
// written: k_seal_prep, then k_seal_auth (GHASH only) in place of k_seal_ctr<true, false>, then
// k_seal_tag<true>; dst is not used.  auth = false is launch_seal as bw_internal.h declares it.
void launch_seal(hipStream_t st, bool dec, bool framed, const uint8_t* src, uint8_t* dst, const SealItem* items,
                 uint64_t n, const SealPads& pads, SealKey* keys, uint64_t n_pieces, uint32_t* parts, uint8_t* ok, bool auth);

}  // namespace bw
