// bw_unpack.h -- host-side declarations of the read side (bw_zstd_dec.hip, used by
// bw_capi_pack.hip): zstd frame decoding and packfile header parsing.  A header of its own, off the
// chunk -> hash -> dedup path (backuwup_amd/build.py OFF_PATH), like the sources it serves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/backuwup_gpu.h"

namespace bw {

struct ZdItem {
    uint64_t src_off, src_len, dst_off, dst_cap;
};
constexpr uint64_t ZD_LIT_STRIDE = 131072 + 64;  // a wave's literals buffer (zd::BLOCK_MAX + slack)
constexpr uint32_t ZD_MAX_WAVES = 2048;          // k_zd_frame's grid: 8 waves per CU on 256 CUs
// frames items[0 .. n) of src decoded into dst by `waves` waves; lit holds waves x ZD_LIT_STRIDE
// bytes; out_len[i] = regenerated size, status[i] = zd::Err (0 = decoded)
void launch_zd_frames(hipStream_t st, const uint8_t* src, uint8_t* dst, const ZdItem* items, uint64_t n, uint32_t waves,
                      uint8_t* lit, uint64_t* out_len, uint32_t* status);
// out[12 k ..] = src[off[k] .. + 12) for k < n (off: device)
void launch_gather12(hipStream_t st, const uint8_t* src, const uint64_t* off, uint64_t n, uint8_t* out);
// opened packfile headers: out null -> parsed[f] = entry count (~0: malformed); else the entries
// of file f at out[rec0[f] ..]
void launch_unpack_parse(hipStream_t st, const uint8_t* pt, const uint64_t* pt_off, const uint64_t* pt_len,
                         uint64_t n_files, const uint64_t* rec0, uint64_t* parsed, bw_unpack_entry* out);

}  // namespace bw
