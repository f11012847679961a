/* backuwup_gpu_pack.h -- the C ABI of the write side after the hot path (SURVEY.md §8f rows 2-4:
 * blob sealing, per-blob zstd level 3, packfiles and index files) and of the read side (row 5: zstd
 * decoding, packfile headers and blobs), implemented by libbackuwup_amd.so
 * (backuwup_amd/csrc/bw_capi_pack.hip).  Included by backuwup_gpu.h, whose types it uses; kept in a
 * file of its own so the hot path's header (and the source digest the committed profiles carry,
 * backuwup_amd/build.py) does not change when this side does. */
#ifndef BACKUWUP_GPU_PACK_H
#define BACKUWUP_GPU_PACK_H
#include "backuwup_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- blob sealing ----
 * The encryption half of Manager::compress_encrypt_blob (pack.rs:70-80) for already compressed
 * payloads, and the packfile header / index keys (pack.rs:212-217, blob_index.rs:185-191,205-213):
 *   key_i = KeyManager::derive_backup_key(info_i)  (key_manager.rs:80-86:
 *           Hkdf::<Sha256>::from_prk(prk).expand(info_i, 32 bytes); prk = backup_secret_key)
 *   out_i = Aes256Gcm::new(key_i).encrypt_in_place(nonce_i, b"", src_i)  = ciphertext || 16-byte tag
 * Item i: src_i = src[src_off[i] .. + src_len[i]), info_i = info[i*info_len .. + info_len)
 * (info_len <= BW_SEAL_MAX_INFO: 32 for a blob hash, 6 for "header", 5 for "index"),
 * nonce_i = nonces[12*i .. + 12]; the output goes to dst + dst_off[i] (src_len[i] + 16 bytes).
 * Output ranges must not overlap each other or the inputs.  Tables are host arrays. */
#define BW_SEAL_MAX_INFO 54u
#define BW_SEAL_TAG_BYTES 16u
/* Device buffers; asynchronous on the context stream. */
int bw_seal_device(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* d_src, const uint64_t* src_off,
                   const uint64_t* src_len, uint64_t n, const uint8_t* info, uint32_t info_len,
                   const uint8_t* nonces, uint8_t* d_dst, const uint64_t* dst_off);
/* decrypt_in_place: src_len[i] includes the tag (>= 16, else BW_EINVAL); plaintext (src_len[i] - 16
 * bytes) to dst + dst_off[i]; ok[i] (host) = 1 if the tag verified, 0 where the reference returns
 * Err(aes_gcm::Error) -- the plaintext of such an item must be discarded.  Synchronous. */
int bw_open_device(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* d_src, const uint64_t* src_off,
                   const uint64_t* src_len, uint64_t n, const uint8_t* info, uint32_t info_len,
                   const uint8_t* nonces, uint8_t* d_dst, const uint64_t* dst_off, uint8_t* ok);
/* Same over host buffers (synchronous; only the output ranges are written). */
int bw_seal(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* src, const uint64_t* src_off,
            const uint64_t* src_len, uint64_t n, const uint8_t* info, uint32_t info_len,
            const uint8_t* nonces, uint8_t* dst, const uint64_t* dst_off);
int bw_open(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* src, const uint64_t* src_off,
            const uint64_t* src_len, uint64_t n, const uint8_t* info, uint32_t info_len,
            const uint8_t* nonces, uint8_t* dst, const uint64_t* dst_off, uint8_t* ok);
/* Reseal: item i, sealed under old_prk with nonces[i], comes out sealed under new_prk with
 * new_nonces[i] (NULL: the nonces are kept).  The tables are bw_open_device's: src_len[i] includes the
 * tag (>= 16, else BW_EINVAL), and output i is src_len[i] bytes at d_dst + dst_off[i].  Where item i is
 * authentic, output i is, byte for byte,
 *   Aes256Gcm(HKDF(new_prk, info_i)).encrypt(new_nonce_i, open(old_prk, item_i)),
 * and ok[i] (host) equals bw_open_device's ok[i] under old_prk for every input.
 * An item whose old tag does not verify does not come out with a valid new tag (that would launder
 * damage into an authentic blob): its ok[i] is 0, its ciphertext bytes are whatever the xor gives, and
 * its 16 tag bytes are the bitwise complement of the tag that would verify, so it is rejected under
 * the new key.
 * The new ciphertext is c ^ keystream_old ^ keystream_new, the two keystreams xored first: no
 * plaintext byte is stored to device or host memory.  Every source byte is read once and never
 * written; nothing outside the output ranges and the context's scratch is written.  Output ranges
 * must not overlap each other or a source range (BW_EINVAL, before anything is written).
 * Synchronous. */
int bw_reseal_device(bw_ctx* ctx, const uint8_t old_prk[32], const uint8_t new_prk[32], const uint8_t* d_src,
                     const uint64_t* src_off, const uint64_t* src_len, uint64_t n, const uint8_t* info,
                     uint32_t info_len, const uint8_t* nonces, const uint8_t* new_nonces, uint8_t* d_dst,
                     const uint64_t* dst_off, uint8_t* ok);
/* Same over host buffers (only the output ranges are written; the plaintext exists on neither side). */
int bw_reseal(bw_ctx* ctx, const uint8_t old_prk[32], const uint8_t new_prk[32], const uint8_t* src,
              const uint64_t* src_off, const uint64_t* src_len, uint64_t n, const uint8_t* info, uint32_t info_len,
              const uint8_t* nonces, const uint8_t* new_nonces, uint8_t* dst, const uint64_t* dst_off, uint8_t* ok);

/* ---- packfiles and index files ----
 * Manager::write_packfiles + serialize_packfile (pack.rs:115-227): the queue of unique blobs
 * (already gated by the index, so write_packfiles' re-check at :131 finds nothing) becomes
 * packfiles laid out back to back in one buffer:
 *   u64 LE header_len || AES-GCM(key "header", nonce = packfile id)(bincode varint
 *   Vec<PackfileHeaderBlob{hash, kind, compression = Zstd, length, offset}>) || (nonce || sealed)*
 * where sealed = AES-GCM(derive_backup_key(hash), nonce)(zstd payload) (pack.rs:58-80).  A
 * packfile closes when its blob section reaches BW_PACKFILE_TARGET_SIZE or it holds
 * BW_PACKFILE_MAX_BLOBS blobs (pack.rs:147).  Packfile ids and blob nonces come from the
 * caller (the reference draws them from getrandom, pack.rs:74-76, :207-208). */
#define BW_PACKFILE_TARGET_SIZE 3145728u /* packfile/mod.rs:25 */
#define BW_PACKFILE_MAX_SIZE 16777216u   /* packfile/mod.rs:27 */
#define BW_PACKFILE_MAX_BLOBS 100000u    /* packfile/mod.rs:29 */
#define BW_BLOB_NONCE_SIZE 12u
#define BW_INDEX_MAX_FILE_ENTRIES 50000u /* blob_index.rs:16 */
#define BW_INDEX_ENTRY_BYTES 44u         /* (BlobHash, PackfileId) */
enum { BW_BLOB_FILE_CHUNK = 0, BW_BLOB_TREE = 1 }; /* BlobKind, filesystem/mod.rs:13-17 */

/* payload_len[i] is the raw blob length: each blob is framed on the GPU as the magicless zstd
 * frame of raw blocks that zstd level 3 emits for incompressible input (2-byte frame header,
 * 3-byte header per 128 KiB block).  Without this flag payloads are caller-made zstd frames. */
#define BW_PACK_ZSTD_STORE 1u

typedef struct bw_packfile {
    uint64_t first_blob; /* queue position of its first blob                         */
    uint64_t n_blobs;
    uint64_t offset;     /* start of the packfile in the output buffer               */
    uint64_t size;       /* 8 + header_len + blob section                            */
    uint64_t header_len; /* encrypted header bytes (the u64 LE prefix)                */
} bw_packfile;

/* ---- per-blob zstd level 3 ----
 * Manager::compress_encrypt_blob's compression (pack.rs:58-64): for every blob, the frame
 * zstd::bulk::Compressor::new(3) writes with include_checksum(false), include_contentsize(false),
 * include_magicbytes(false) -- byte for byte the level-3 output of libzstd's dfast compressor
 * (pinned against the system libzstd 1.4.8; the reference links 1.5.5).
 * Blob i: src + src_off[i] (src_len[i] <= 3 MiB, else BW_EINVAL like add_blob's BlobTooLarge,
 * pack.rs:32-34); its frame goes to dst + dst_off[i], which must hold bw_zstd_store_size(src_len[i])
 * bytes (level 3 never writes more); frame_len[i] (host) = the frame's size.  Synchronous. */
int bw_zstd_compress_device(bw_ctx* ctx, const uint8_t* d_src, const uint64_t* src_off, const uint64_t* src_len,
                            uint64_t n, uint8_t* d_dst, const uint64_t* dst_off, uint64_t* frame_len);
/* Same over host buffers (staged through the device). */
int bw_zstd_compress(bw_ctx* ctx, const uint8_t* src, const uint64_t* src_off, const uint64_t* src_len, uint64_t n,
                     uint8_t* dst, const uint64_t* dst_off, uint64_t* frame_len);
/* Asynchronous form: one call lasts as long as its largest blob's serial parse, so a packer keeps
 * several batches in flight.  bw_zstd_submit_device copies the offset tables, starts the batch on
 * one of the context's BW_ZSTD_LANES lanes (each its own hash tables and a stream of its own,
 * ordered after the work already on the context's stream: lanes 0-3 high-priority streams, which
 * the runtime serves from a hardware-queue pool of their own, lanes 4-5 normal ones; 1 GiB text
 * batches from one host thread, HIP's default 4 queues per pool: 4 lanes 3.5 GB/s, 6 lanes 4.4-4.6)
 * and returns at once with *ticket; BW_ESTATE when every lane holds
 * a batch (wait for one first).  Hash tables: per lane, 768 KiB per blob for sub-batches of more
 * than 2,048 blobs and 2.5 MiB per blob for smaller ones (two pools, each grown to the largest
 * sub-batch of its layout seen: at most BW_OPT_ZSTD_SLOTS x 768 KiB + 2,048 x 2.5 MiB).  d_src and d_dst stay untouched by the caller until
 * bw_zstd_wait(ticket), which blocks for the batch and writes its n frame sizes to frame_len. */
#define BW_ZSTD_LANES 6
int bw_zstd_submit_device(bw_ctx* ctx, const uint8_t* d_src, const uint64_t* src_off, const uint64_t* src_len,
                          uint64_t n, uint8_t* d_dst, const uint64_t* dst_off, uint64_t* ticket);
int bw_zstd_wait(bw_ctx* ctx, uint64_t ticket, uint64_t* frame_len);

/* compress_encrypt_blob + write_packfiles end to end (pack.rs:58-80, 115-227) for a queue of
 * unique blobs in device memory, in two calls around the caller's plan:
 *   1. bw_pack_compress_device: zstd level 3 of blob i (d_src + src_off[i], src_len[i] <= 3 MiB,
 *      else BW_EINVAL) into a staging area the context owns; frame_len[i] (host) = its frame's
 *      size (synchronous);
 *   2. the caller plans over those sizes -- bw_pack_plan(frame_len, n, 0, ...) or
 *      bw_pack_plan_session(..., frame_len, ..., 0, ...) -- and draws one id per packfile;
 *   3. bw_pack_build_compressed: the staged frames sealed (derive_backup_key(hashes[i]), nonces[i])
 *      and laid out as bw_pack_build_device does with flags 0 (asynchronous on the context stream).
 * The staged frames stay valid until the next bw_pack_compress_device on the same context. */
int bw_pack_compress_device(bw_ctx* ctx, const uint8_t* d_src, const uint64_t* src_off, const uint64_t* src_len,
                            uint64_t n, uint64_t* frame_len);
int bw_pack_build_compressed(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* hashes, const uint8_t* kinds,
                             const uint8_t* nonces, const bw_packfile* plan, uint64_t npf, const uint8_t* ids,
                             uint8_t* d_out);
/* Host-buffer forms (synchronous): the blobs are staged through the device; the packfiles land
 * in out (plan[npf-1].offset + plan[npf-1].size bytes). */
int bw_pack_compress(bw_ctx* ctx, const uint8_t* src, const uint64_t* src_off, const uint64_t* src_len, uint64_t n,
                     uint64_t* frame_len);
int bw_pack_build_compressed_host(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* hashes, const uint8_t* kinds,
                                  const uint8_t* nonces, const bw_packfile* plan, uint64_t npf, const uint8_t* ids,
                                  uint8_t* out);
/* Size of the zstd store frame of a len-byte blob. */
uint64_t bw_zstd_store_size(uint64_t len);
/* Grouping and sizes (host only).  out may be NULL with cap 0 to query *n_out; BW_ENOSPC when
 * cap is too small; *total_bytes = the output buffer size. */
int bw_pack_plan(const uint64_t* payload_len, uint64_t n, uint32_t flags, bw_packfile* out, uint64_t cap,
                 uint64_t* n_out, uint64_t* total_bytes);
/* The reference's write cadence over one session (Manager::add_blob -> trigger_write_if_desired ->
 * write_packfiles, then Manager::flush; pack.rs:31-55, 82-162): n blobs in canonical (add) order
 * with their gate verdicts (bw_blob.is_dup) and payload lengths.  The packfiles hold the blobs with
 * is_dup == 0 in that order (*n_unique of them; first_blob counts among them), cut where the
 * reference cuts: a drain starts when the pending queue -- including copies of still-pending blobs,
 * which add_blob does not catch -- reaches BW_PACKFILE_TARGET_SIZE sealed bytes or
 * BW_PACKFILE_MAX_BLOBS blobs, and drains everything queued (its last packfile is a remainder);
 * the final flush drains the rest.  Host only. */
int bw_pack_plan_session(const uint8_t* digests, const uint8_t* is_dup, const uint64_t* payload_len, uint64_t n,
                         uint32_t flags, bw_packfile* out, uint64_t cap, uint64_t* n_out, uint64_t* total_bytes,
                         uint64_t* n_unique);
/* Build the planned packfiles.  Blob i: payload d_src + src_off[i] (src_len[i] bytes), hashes
 * 32 B, kinds 1 B (BW_BLOB_*), nonces 12 B; packfile_ids 12 B per packfile (host arrays).
 * d_out (device, plan's total_bytes) receives the packfiles.  Asynchronous on the context
 * stream; plan = bw_pack_plan's or bw_pack_plan_session's; BW_EINVAL when the plan does not match the blobs or a packfile exceeds
 * BW_PACKFILE_MAX_SIZE (the reference's assert, pack.rs:152-156). */
int bw_pack_build_device(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* d_src, const uint64_t* src_off,
                         const uint64_t* src_len, uint64_t n, const uint8_t* hashes, const uint8_t* kinds,
                         const uint8_t* nonces, uint32_t flags, const bw_packfile* plan, uint64_t n_packfiles,
                         const uint8_t* packfile_ids, uint8_t* d_out);
/* Same over host buffers (synchronous). */
int bw_pack_build(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* src, const uint64_t* src_off,
                  const uint64_t* src_len, uint64_t n, const uint8_t* hashes, const uint8_t* kinds,
                  const uint8_t* nonces, uint32_t flags, const bw_packfile* plan, uint64_t n_packfiles,
                  const uint8_t* packfile_ids, uint8_t* out);

/* Index files: BlobIndex::push/flush (blob_index.rs:151-164, 202-226).  file =
 * AES-GCM(key "index", nonce = u32 LE file number || 0^8)(bincode varint Vec<(BlobHash,
 * PackfileId)>). */
typedef struct bw_index_file {
    uint32_t file_num; /* the file name, "{file_num:0>10}"               */
    uint32_t pad;
    uint64_t offset;   /* start of the file in the buffer                  */
    uint64_t size;     /* bytes (plaintext + 16)                           */
    uint64_t n_entries;
} bw_index_file;
/* entries (host, n x 44 B) pushed in order from last_file_num: one file per
 * BW_INDEX_MAX_FILE_ENTRIES entries plus the final unconditional flush (Manager::flush,
 * pack.rs:84-90), so n = 0 still writes one empty file.  out (host) receives the files back to
 * back; files[] their table.  out = NULL or a small cap: BW_ENOSPC with *n_files and
 * *total_bytes set.  Sealed on the GPU; synchronous. */
int bw_index_files_build(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* entries, uint64_t n,
                         uint32_t last_file_num, uint8_t* out, uint64_t cap, bw_index_file* files, uint64_t files_cap,
                         uint64_t* n_files, uint64_t* total_bytes);
/* BlobIndex::load (blob_index.rs:167-200) fused with the device seed: n_files index files (host
 * buffer `data`, table files[] with file_num/offset/size) are decrypted and parsed on the GPU
 * and every digest is seeded into the context's index (as bw_index_seed).  entries (optional,
 * host, cap x 44 B) receives the records in file order (the reference sorts its `items` by hash
 * afterwards).  A file whose tag fails -> BW_ECRYPTO, one that is not exactly one varint Vec ->
 * BW_EFORMAT; *bad_file = its position and nothing is seeded.  Synchronous. */
int bw_index_load_files(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* data, const bw_index_file* files,
                        uint64_t n_files, uint8_t* entries, uint64_t cap, uint64_t* n_entries, uint64_t* bad_file);

/* ---- the read side ----
 * Manager::get_blob's data path (unpack.rs:23-83): packfile header opened and parsed, blob opened,
 * frame decoded.  The decoder is written from RFC 8878 (backuwup_amd/csrc/bw_zstd_dec_core.h): it
 * reads every frame a zstd encoder at any level writes for one blob without a dictionary, not only
 * what bw_zstd_compress emits.  Refused, with a per-blob error: a non-zero dictionary id, the
 * checksum flag (the reference's Compressor never sets it, pack.rs:58-64), a reserved block type,
 * bytes after the last block, and every malformed or truncated section.  All calls are synchronous. */

/* Decompressor::new() + include_magicbytes(false) + decompress(buf, BLOB_MAX_UNCOMPRESSED_SIZE)
 * (unpack.rs:65-67) for n magicless frames.  Frame i: d_src + src_off[i], src_len[i] bytes; its
 * bytes go to d_dst + dst_off[i], at most dst_cap[i] (<= 3 MiB, else BW_EINVAL); out_len[i] (host)
 * = the regenerated size; ok[i] (host) = 1, or 0 where the reference returns Err (out_len[i] = 0;
 * the blob's output range then holds garbage).  Nothing outside [dst_off[i], dst_off[i] +
 * dst_cap[i]) is written, whatever the frame says.  Output ranges must not overlap each other or
 * the input.  A frame of 0 bytes decodes to 0 bytes, as ZSTD_decompressDCtx does. */
int bw_zstd_decompress_device(bw_ctx* ctx, const uint8_t* d_src, const uint64_t* src_off, const uint64_t* src_len,
                              uint64_t n, uint8_t* d_dst, const uint64_t* dst_off, const uint64_t* dst_cap,
                              uint64_t* out_len, uint8_t* ok);
/* Same over host buffers (staged through the device, which holds the frames and sum(dst_cap) bytes;
 * only out_len[i] bytes per blob are copied back). */
int bw_zstd_decompress(bw_ctx* ctx, const uint8_t* src, const uint64_t* src_off, const uint64_t* src_len, uint64_t n,
                       uint8_t* dst, const uint64_t* dst_off, const uint64_t* dst_cap, uint64_t* out_len, uint8_t* ok);

/* One PackfileHeaderBlob (filesystem/mod.rs:36-43) as stored, with the packfile it came from. */
typedef struct bw_unpack_entry {
    uint8_t hash[32];
    uint32_t packfile;   /* position in the packfiles[] table of the call              */
    uint8_t kind;        /* BW_BLOB_*                                                  */
    uint8_t compression; /* CompressionKind tag as stored (0 = None, 1 = Zstd)         */
    uint8_t pad[2];
    uint64_t length;     /* sealed bytes (frame + 16-byte tag)                         */
    uint64_t offset;     /* of the blob's nonce, relative to the blob section          */
} bw_unpack_entry;

/* The header half of get_blob (unpack.rs:27-48) for n_pf packfiles lying in the host buffer
 * `data`: packfiles[p].offset / .size locate packfile p (the other fields are ignored), ids holds
 * its 12-byte id.  Size and header_len checks on the host; headers opened (key "header", nonce =
 * id) and parsed on the GPU, as bw_index_load_files does for index files.  entries (host, cap
 * records) receives every header's entries in packfile order; *n_entries their number.
 *   size > BW_PACKFILE_MAX_SIZE (PackfileTooLarge, :28), header_len == 0 or > size
 *   (InvalidHeaderSize, :36) or past the packfile's bytes           -> BW_EFORMAT
 *   tag mismatch (:45)                                               -> BW_ECRYPTO
 *   not exactly one varint Vec<PackfileHeaderBlob>, enum tag above 1 -> BW_EFORMAT
 * each with *bad_file = the packfile's position (else ~0); cap too small -> BW_ENOSPC with
 * *n_entries set. */
int bw_unpack_headers(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* data, const bw_packfile* packfiles,
                      const uint8_t* ids, uint64_t n_pf, bw_unpack_entry* entries, uint64_t cap, uint64_t* n_entries,
                      uint64_t* bad_file);

/* The blob half of get_blob (unpack.rs:52-73) for n chosen entries over packfiles in device
 * memory (d_packfiles + packfiles[p].offset, .size; .header_len must be the u64 prefix's value,
 * as bw_pack_plan wrote it or as read from the packfile): the nonce is read at 8 + header_len +
 * entry.offset, the blob opened with derive_backup_key(entry.hash) into a staging area the context
 * owns (shared with bw_pack_compress_device: frames staged there are dropped), and its frame
 * decoded to d_dst + dst_off[i] (at most BLOB_MAX_UNCOMPRESSED_SIZE = 3 MiB each; out_len[i] =
 * the regenerated size).  entry.compression is ignored and the payload always decoded, as the
 * reference does (unpack.rs:65-67).  With BW_UNPACK_VERIFY the regenerated bytes are hashed on the
 * device and compared with entry.hash, which the reference never does (this runs a batch through
 * the context's pipeline, like bw_process_files_device: wait for outstanding tickets first).
 * status[i] (host) is one of BW_UNPACK_*; a blob failure is reported there and the call still
 * returns BW_OK. */
#define BW_UNPACK_VERIFY 1u
enum {
    BW_UNPACK_OK = 0,
    BW_UNPACK_ETAG = 1,    /* aes_gcm::Error (unpack.rs:63)                            */
    BW_UNPACK_EZSTD = 2,   /* the Decompressor's error (unpack.rs:67)                  */
    BW_UNPACK_EDIGEST = 3, /* BW_UNPACK_VERIFY: BLAKE3 of the bytes != entry.hash      */
    BW_UNPACK_ERANGE = 4   /* nonce + length outside the packfile (read_exact fails, :58-59), or length < 16 */
};
int bw_unpack_blobs_device(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* d_packfiles, const bw_packfile* packfiles,
                           uint64_t n_pf, const bw_unpack_entry* entries, uint64_t n, uint32_t flags, uint8_t* d_dst,
                           const uint64_t* dst_off, uint64_t* out_len, uint8_t* status);
/* Same over host buffers (packfiles uploaded, blobs copied back).  A frame does not say how much it
 * regenerates, so the call reserves 3 MiB of device memory per entry: pass a few hundred entries at a time. */
int bw_unpack_blobs(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* packfiles_data, const bw_packfile* packfiles,
                    uint64_t n_pf, const bw_unpack_entry* entries, uint64_t n, uint32_t flags, uint8_t* dst,
                    const uint64_t* dst_off, uint64_t* out_len, uint8_t* status);

/* ---- restore: the data path of dir_unpacker.rs:14-130 ----
 * A session over a set of packfiles in device memory does what unpack() does with data: find a
 * blob by hash (BlobIndex::find_packfile, blob_index.rs:143-148, then the header scan of
 * unpack.rs:50-51), walk the trees (fetch_tree, fetch_full_tree, the breadth-first queue of unpack)
 * and assemble files from their chunks (restore_file).  Creating directories, writing files and
 * setting mtimes stays with the caller (backuwup_amd/restore.py does it).  All calls are synchronous
 * and use the context the session was opened on; the session owns every buffer it needs. */
typedef struct bw_restore bw_restore;

/* Per-hash and per-file statuses of a session, beside BW_UNPACK_* (which they never collide with). */
enum {
    BW_RESTORE_OK = 0,
    BW_RESTORE_ENOTFOUND = 16,   /* the index lacks the hash: get_blob returns Ok(None), unpack.rs:24-26 */
    BW_RESTORE_EMISMATCH = 17,   /* the packfile's header lacks it: IndexHeaderMismatch, unpack.rs:77    */
    BW_RESTORE_ENOPACKFILE = 18, /* the index names a packfile id that is not among ids: File::open fails */
    BW_RESTORE_ENOTTREE = 19,    /* a tree hash names a FileChunk blob, dir_unpacker.rs:124              */
    BW_RESTORE_EFORMAT = 20      /* bincode::deserialize::<Tree> fails, or a chain or directory cycle    */
};
/* Test hook for bw_restore_files(_device): the k-th distinct blob of a call is decoded k mod 16 bytes
 * past a 16-byte boundary, so that the gather's unaligned-source path runs (sources are 16-byte
 * aligned otherwise). */
#define BW_RESTORE_SKEW_SLOTS 0x100u

/* packfiles / entries: as bw_unpack_headers took and returned them (d_packfiles + packfiles[p].offset,
 * .size, .header_len; ids 12 B each); index_items: n_items x BW_INDEX_ENTRY_BYTES (BlobHash,
 * PackfileId) records as bw_index_load_files returns them (BlobIndex.items).  slots = how many
 * 3 MiB decode slots the session owns (0 = 1,024).  Two device tables are built, one kernel launch
 * each: hash -> packfile position (a hash the index holds more than once resolves to any of its
 * items, as the reference's binary search may), and (packfile position, hash) -> the lowest entry
 * index (the header scan's first match).  Both compare whole 32-byte keys.  d_packfiles must stay
 * valid and unchanged until bw_restore_close; the host tables are copied. */
int bw_restore_open(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* d_packfiles, const bw_packfile* packfiles,
                    const uint8_t* ids, uint64_t n_pf, const bw_unpack_entry* entries, uint64_t n_entries,
                    const uint8_t* index_items, uint64_t n_items, uint32_t slots, bw_restore** out);
/* Same over packfiles in a host buffer: the session uploads them and keeps the copy. */
int bw_restore_open_host(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* packfiles_data, const bw_packfile* packfiles,
                         const uint8_t* ids, uint64_t n_pf, const bw_unpack_entry* entries, uint64_t n_entries,
                         const uint8_t* index_items, uint64_t n_items, uint32_t slots, bw_restore** out);
int bw_restore_close(bw_restore* session);
/* The lookup alone: entry_idx[i] = the entry of hashes[32 i ..] and status[i] = BW_RESTORE_OK, or
 * entry_idx[i] = ~0 and status[i] = BW_RESTORE_ENOTFOUND / _EMISMATCH / _ENOPACKFILE. */
int bw_restore_locate(bw_restore* session, const uint8_t* hashes, uint64_t n, uint64_t* entry_idx, uint8_t* status);

/* One node of the walk.  Node 0 is the root; the children of a Dir node are the nodes
 * [child_first, child_first + n_children) in child order, parents taken in node order (the order in
 * which unpack() visits them); the children of a File node are the rows [child_first, child_first +
 * n_children) of `chunks` (32 B each). */
typedef struct bw_restore_node {
    uint32_t kind;  /* BW_TREE_FILE or BW_TREE_DIR      */
    uint32_t flags; /* BW_TREE_HAS_*                    */
    uint64_t size, mtime, ctime;
    uint64_t parent; /* ~0 for the root                 */
    uint64_t child_first, n_children;
    uint64_t name_off, name_len; /* into `names`        */
} bw_restore_node;
typedef struct bw_restore_counts {
    uint64_t n_nodes, name_bytes, n_chunks;
} bw_restore_counts;
typedef struct bw_restore_error {
    uint8_t hash[32]; /* the offending tree blob        */
    uint32_t reason;  /* BW_RESTORE_* or BW_UNPACK_*    */
    uint32_t pad;
} bw_restore_error;

/* unpack()'s walk, level by level: every level's tree blobs are located, opened and decoded through
 * the unpack chain, parsed on the device (bincode 1.3.3 legacy deserialize: fixint little endian,
 * u32 enum tag, u64 lengths, one-byte Option tags, trailing bytes allowed), their next_sibling
 * chains followed one round at a time and each chain's children concatenated in chain order.
 * flags: BW_UNPACK_VERIFY or 0.  *counts always receives what the walk needs; the arrays are filled
 * when all three caps suffice, else BW_ENOSPC.  A tree error is fatal to the walk, as
 * fetch_full_tree(..).await? is: BW_EFORMAT is returned and *err names the blob and the reason (a
 * locate status, BW_UNPACK_ETAG / _EZSTD / _ERANGE / _EDIGEST, BW_RESTORE_ENOTTREE, or
 * BW_RESTORE_EFORMAT: an enum or Option tag above 1, a name that String::from_utf8 refuses, a
 * length that runs past the blob).
 * Differences from the reference: it creates directories as it goes, so on an error deep in the
 * tree it has already written the levels above; this call reports before anything is written.  It
 * loops forever on a next_sibling cycle or a directory that contains itself; here a chain of more
 * pieces than the store has entries, and a tree whose hash is one of its own ancestors', are
 * BW_RESTORE_EFORMAT.  A root of kind File yields one node and its chunk rows; the reference
 * restores nothing from it. */
int bw_restore_trees(bw_restore* session, const uint8_t root_hash[32], uint32_t flags, bw_restore_node* nodes,
                     uint64_t node_cap, uint8_t* names, uint64_t names_cap, uint8_t* chunks, uint64_t chunks_cap,
                     bw_restore_counts* counts, bw_restore_error* err);

/* restore_file (dir_unpacker.rs:75-92) for n_files files: file f is the concatenation of the blobs
 * named by rows file_first[f] .. file_first[f + 1] of chunks (host, 32 B each); the files land back
 * to back in d_dst, file_off[f] / file_len[f] (host) say where.  The children go through in file
 * order in sub-batches of at most `slots` distinct blobs, each located, opened and decoded once per
 * sub-batch however often it is named; the instances' places come from a scan of the regenerated
 * sizes on the device, and one gather kernel copies them.  flags: BW_UNPACK_VERIFY,
 * BW_RESTORE_SKEW_SLOTS.
 * Failures are per file, as the reference prints them and carries on (dir_unpacker.rs:58-63):
 * file_status[f] = the first failing child's status (a locate status or BW_UNPACK_*),
 * file_bad_child[f] = its position in the file (~0 when none), file_len[f] = the bytes of the
 * children before it, which is the partial file the reference leaves behind.
 * dst_cap is a window: when a file does not fit behind the ones before it, the call returns
 * BW_ENOSPC with *n_done = the whole files written (the caller drains them and calls again with
 * the rest) and file_len[*n_done] = that file's size as far as the sub-batch showed it.  Nothing
 * outside [d_dst, d_dst + dst_cap) is written.  Otherwise *n_done = n_files. */
int bw_restore_files_device(bw_restore* session, const uint8_t* chunks, const uint64_t* file_first, uint64_t n_files,
                            uint32_t flags, uint8_t* d_dst, uint64_t dst_cap, uint64_t* file_off, uint64_t* file_len,
                            uint8_t* file_status, uint64_t* file_bad_child, uint64_t* n_done);
/* Same into a host buffer (the files are copied back from a window the session owns). */
int bw_restore_files(bw_restore* session, const uint8_t* chunks, const uint64_t* file_first, uint64_t n_files,
                     uint32_t flags, uint8_t* dst, uint64_t dst_cap, uint64_t* file_off, uint64_t* file_len,
                     uint8_t* file_status, uint64_t* file_bad_child, uint64_t* n_done);

/* ---- prune: which header entries a set of roots reaches, and packfiles of the live ones ----
 * The reference has no prune; this goes past it as BW_UNPACK_VERIFY does.  Three steps over an open
 * restore session: bw_prune_mark (device), bw_prune_plan (host), bw_prune_repack (device).  A sealed
 * blob is nonce || AES-GCM(derive_backup_key(hash), nonce)(frame): neither depends on the packfile,
 * so a repack copies blobs verbatim and seals only new headers.  All calls are synchronous. */
typedef struct bw_prune_packfile_stat {
    uint64_t live_blobs, live_bytes, total_blobs, total_bytes; /* bytes: 12 + length per entry */
} bw_prune_packfile_stat;
typedef struct bw_prune_counts {
    uint64_t live_blobs, live_bytes, total_blobs, total_bytes; /* the sums of the per-packfile stats   */
    uint64_t n_trees_expanded; /* tree blobs opened, parsed and expanded                                */
    uint64_t n_levels;         /* rounds of the walk (a next_sibling is one step, like a child)         */
    uint64_t n_errors;         /* always the full number                                                */
} bw_prune_counts;
/* A reference error names the reference: hash = the hash referred to, parent = the piece that holds
 * it (all zero for a root), child_pos = the child's position (~0 for next_sibling, the root's index
 * for a root).  An entry error names an entry: hash = the entry's, parent zero, child_pos = ~0. */
typedef struct bw_prune_error {
    uint8_t hash[32];
    uint8_t parent[32];
    uint64_t child_pos;
    uint32_t reason; /* BW_RESTORE_* or BW_UNPACK_* */
    uint32_t pad;
} bw_prune_error;

/* Reachability from n_roots root hashes (host, 32 B each; 0 roots: everything is dead) over the
 * session's entries.  live[e] (host, one byte per session entry) = 1 when a kept root reaches entry
 * e.  The walk is level-synchronous: a frontier of tree entries not yet expanded (a device list)
 * goes through the unpack chain `slots` blobs at a time, is parsed in the slots, and one kernel
 * resolves every children row and next_sibling with the session's tables (the answer
 * bw_restore_locate gives), sets the entry's live bit and, for a tree reference (a child of a Dir
 * piece, a next_sibling, a root), its queued bit; the lane that sets the queued bit appends the
 * entry to the next frontier.  Each distinct tree blob is expanded once whatever the number of
 * roots and paths that reach it; cycles end by themselves and are no error.  The children of a File
 * piece are marked whatever their kind and never opened.  A hash held by several entries marks only
 * the entry bw_restore_locate resolves it to.  flags: BW_UNPACK_VERIFY (tree blobs are re-hashed;
 * chunk payloads are never read) or 0.
 * Errors never stop the walk.  Reference errors: a failed locate (BW_RESTORE_ENOTFOUND, _EMISMATCH,
 * _ENOPACKFILE), or a tree reference that resolves to a FileChunk entry (BW_RESTORE_ENOTTREE; the
 * entry is marked live all the same).  Entry errors: a tree blob the chain or the parser refuses
 * (BW_UNPACK_ETAG, _EZSTD, _EDIGEST, _ERANGE, BW_RESTORE_EFORMAT; it is live but not expanded), and a
 * live FileChunk entry whose nonce + length leaves its packfile or whose length < 16
 * (BW_UNPACK_ERANGE), each reported once.  errs is filled in no particular order;
 * counts->n_errors > err_cap -> BW_ENOSPC with live, stats (n_pf records) and counts still filled. */
int bw_prune_mark(bw_restore* session, const uint8_t* roots, uint64_t n_roots, uint32_t flags, uint8_t* live,
                  bw_prune_packfile_stat* stats, bw_prune_counts* counts, bw_prune_error* errs, uint64_t err_cap);

/* Host only.  order = the live entries of the packfiles with rewrite[p] != 0, ascending by packfile
 * position, then by entry index; plan = write_packfiles' grouping over their sealed lengths (the
 * rule of bw_pack_plan with flags 0: first_blob counts positions of order, sizes include the exact
 * header).  Packfiles with rewrite[p] == 0 are left alone, dead blobs and all; a rewritten packfile
 * without a live blob contributes nothing.  A live entry of a rewritten packfile whose range leaves
 * its packfile or whose length < 16 -> BW_EINVAL with *bad_entry = its index (else ~0); a new
 * packfile above BW_PACKFILE_MAX_SIZE -> BW_EINVAL.  A cap too small -> BW_ENOSPC with *n_moved,
 * *n_new and *total_bytes set. */
int bw_prune_plan(const bw_unpack_entry* entries, uint64_t n_entries, const bw_packfile* packfiles, uint64_t n_pf,
                  const uint8_t* live, const uint8_t* rewrite, uint64_t* order, uint64_t order_cap, uint64_t* n_moved,
                  bw_packfile* plan, uint64_t plan_cap, uint64_t* n_new, uint64_t* total_bytes, uint64_t* bad_entry);

/* The planned packfiles into d_out (device, plan's total_bytes): each moved blob's nonce || sealed
 * bytes copied from the session's packfiles by one kernel (no blob is opened), each header built
 * from the moved entries (hash, kind, length and the compression tag exactly as stored; offset = the
 * running 12 + length sum) and sealed with key "header" and nonce new_ids[12 p ..].  order and plan
 * are checked again against the session's entries: BW_EINVAL when they do not match.  Nothing
 * outside [d_out, d_out + total_bytes) is written and no packfile byte outside the moved blobs is
 * read.  d_out must not overlap the session's packfiles. */
int bw_prune_repack_device(bw_restore* session, const uint64_t* order, uint64_t n_moved, const bw_packfile* plan,
                           uint64_t n_new, const uint8_t* new_ids, uint8_t* d_out);
/* Same into a host buffer. */
int bw_prune_repack(bw_restore* session, const uint64_t* order, uint64_t n_moved, const bw_packfile* plan,
                    uint64_t n_new, const uint8_t* new_ids, uint8_t* out);

/* ---- diff: what changed between two snapshots, opening only the tree blobs on changed paths ----
 * The reference has no diff.  A Tree blob holds its own name, kind and metadata and names its children
 * and its next_sibling by hash (filesystem/mod.rs:63-77), so equal hashes mean equal subtrees.  An
 * item is a pair (A hash or none, B hash or none); the walk starts with the root pair and goes down
 * level by level over an open restore session. */
enum { BW_DIFF_ADDED = 1, BW_DIFF_REMOVED = 2, BW_DIFF_MODIFIED = 3, BW_DIFF_TYPE_CHANGED = 4 };
#define BW_DIFF_UNREADABLE 1u /* a side's first piece could not be read: that side has its hash only  */
#define BW_DIFF_TRUNCATED 2u  /* a later piece of a side's chain could not be read: its list ends there */
typedef struct bw_diff_side {
    uint8_t hash[32];
    uint32_t kind;  /* BW_TREE_FILE or BW_TREE_DIR */
    uint32_t flags; /* BW_TREE_HAS_*               */
    uint64_t size, mtime, ctime;
    uint64_t n_children; /* the rows of its whole next_sibling chain */
} bw_diff_side;
typedef struct bw_diff_record {
    uint32_t change; /* BW_DIFF_ADDED .. BW_DIFF_TYPE_CHANGED */
    uint32_t flags;  /* BW_DIFF_UNREADABLE, BW_DIFF_TRUNCATED  */
    uint64_t parent; /* the record of the item above, ~0 for a root item; always lower than the record's own index */
    uint64_t name_off, name_len; /* into `names`: the B side's name, A's for REMOVED; empty for an unreadable node */
    bw_diff_side a, b;           /* an absent side is all zero */
    uint64_t common_prefix, common_suffix, n_new; /* BW_DIFF_MODIFIED: over the two children lists */
} bw_diff_record;
typedef struct bw_diff_counts {
    uint64_t n_records, name_bytes;
    uint64_t n_read;   /* entries opened: the ones of read[]                      */
    uint64_t n_levels; /* levels of the walk that hold a record                   */
    uint64_t n_errors; /* always the full number                                  */
} bw_diff_counts;

/* root_a / root_b: 32 bytes each (host), or NULL for an empty snapshot; both NULL or equal bytes: no
 * record, no error, nothing read, n_levels = 0.  flags: BW_UNPACK_VERIFY or 0.  Synchronous.
 *   Equal hashes give no record and are not opened.  Otherwise one record per item: one side present
 * is ADDED or REMOVED; both of one kind MODIFIED; File against Dir TYPE_CHANGED, whose sides are
 * expanded apart.  The roots pair whatever their names.  A side's list is the children rows of its
 * next_sibling chain in chain order.  MODIFIED: common_prefix = the equal leading rows, common_suffix
 * = the equal trailing rows capped at min(n_a, n_b) - common_prefix, n_new = the B rows whose hash is
 * nowhere in A's list.  A File's rows are chunk hashes and are never opened.  A child of a Dir item
 * is unmatched when its hash does not occur in the other side's list; every unmatched child's first
 * piece is read; per side the unmatched child at the lowest position represents its name,
 * representatives with byte-equal names pair, every other one is one-sided, and one-sided Dirs are
 * expanded all the way down.  Every comparison of hashes and names runs on the device.
 *   read[e] (host, one byte per session entry) = 1 exactly for the Tree entries opened: first pieces
 * of unmatched children (and of the roots) and later chain pieces of expanded items.
 *   Errors never stop the walk and use prune's record: hash = the hash referred to, parent = the
 * piece that names it (zero for a root), child_pos = its position there (~0 for a next_sibling, 0 / 1
 * for root A / B), reason = a locate status, BW_RESTORE_ENOTTREE, BW_UNPACK_ERANGE / _ETAG / _EZSTD /
 * _EDIGEST, or BW_RESTORE_EFORMAT (the parser, a chain of more pieces than the store has entries, a
 * child whose hash is one of its ancestors' on its side: its first piece is read for the name and its
 * list counts as empty).  A first piece that cannot be read gives a one-sided record with
 * BW_DIFF_UNREADABLE; a later piece that cannot be read ends the list and sets BW_DIFF_TRUNCATED.
 * counts->n_errors > err_cap -> BW_ENOSPC with everything else filled; errs is in no particular order.
 *   Capacity: the walk stops at the first level whose records or names do not fit and returns
 * BW_ENOSPC with counts holding the totals up to and including that level; the levels before it are
 * filled in, and nothing is written past a cap.  A parent's record comes before its children's; the
 * order inside a level is free.
 *   Hard limit: the walk indexes a level in 32 bits.  A level of more than 2^30 nodes, or whose lists
 * hold more than 2^30 children rows (a forged chain that names itself can grow one that far), ends
 * the call with BW_ENOMEM, as does a device allocation that fails; nothing is filled in then. */
int bw_diff_trees(bw_restore* session, const uint8_t* root_a, const uint8_t* root_b, uint32_t flags,
                  bw_diff_record* records, uint64_t record_cap, uint8_t* names, uint64_t names_cap, uint8_t* read,
                  bw_diff_counts* counts, bw_prune_error* errs, uint64_t err_cap);

/* ---- parent match: which files a new backup need not read ----
 * The reference reads, chunks and hashes every file on every run (dir_packer.rs:231-282) and lets dedup
 * discard the result; this goes past it, as restic's parent snapshot and git's index do.  A Tree blob
 * holds its own name, kind and metadata and names its children by hash (filesystem/mod.rs:63-77), so a
 * File's tree blob in the parent snapshot is the new snapshot's as it stands when name, kind, size,
 * mtime and ctime are equal and the chunk list is assumed equal: the parent's child hash is the new
 * child hash, no file byte is read and no tree blob is rebuilt.  That assumption is the heuristic. */
enum {
    BW_PARENT_NEW = 0,          /* no readable child of that name under the matched parent Dir, or the node above is not DIR */
    BW_PARENT_UNCHANGED = 1,    /* File against File, equal flags with HAS_SIZE and HAS_MTIME, equal size, mtime and (where
                                   flagged) ctime, mtime < trust_before */
    BW_PARENT_CHANGED = 2,      /* File against File, anything else */
    BW_PARENT_RACY = 3,         /* would be UNCHANGED, but mtime >= trust_before */
    BW_PARENT_DIR = 4,          /* Dir against Dir: descended */
    BW_PARENT_TYPE_CHANGED = 5  /* File against Dir or Dir against File: nothing below is matched */
};
typedef struct bw_parent_result {
    uint8_t hash[32]; /* the parent snapshot's child hash; zero for BW_PARENT_NEW */
    uint32_t status;  /* BW_PARENT_* */
    uint32_t pad;
} bw_parent_result;
typedef struct bw_parent_counts {
    uint64_t n_read;          /* entries opened: the ones of read[]                         */
    uint64_t n_levels;        /* levels of the walk that hold an item; level 0 is the roots */
    uint64_t n_errors;        /* always the full number                                     */
    uint64_t n_unchanged;     /* scan nodes that are BW_PARENT_UNCHANGED                    */
    uint64_t unchanged_bytes; /* the sum of their sizes: what the backup will not read      */
} bw_parent_counts;

/* The scan (host) is what a stat-only directory walk yields, in the layout of a bw_restore_trees
 * listing: node 0 is the root; a Dir's children are the nodes [child_first, child_first + n_children);
 * a File has n_children = 0; name_off / name_len point into names; parent is not looked at.  A listing
 * of bw_restore_trees is a valid scan once its File nodes' n_children are zeroed.  It is checked in
 * O(n) before anything is read: kind in {File, Dir}, name ranges inside names, a File without
 * children, a Dir's children after itself, inside the scan, and no node the child of two; otherwise
 * BW_EINVAL, with read all zero.  parent_root: 32 bytes (host), or NULL: every node is NEW, nothing
 * is read, n_levels = 0.  flags: BW_UNPACK_VERIFY or 0.  Synchronous.
 *   The walk is level by level.  Level 0 is the item (scan node 0, parent_root); the roots pair whatever
 * their names.  For an item (scan Dir, hash) the hash's whole next_sibling chain is read and its
 * children rows concatenated in chain order; of every row the first piece only is read, for its name,
 * kind and metadata (a File's later pieces are never opened); the readable rows of one item are keyed
 * by their whole name bytes, the lowest position winning among equal names; every scan child of the
 * Dir probes that table (scan children with equal names get one answer) and gets its status from the
 * table above.  trust_before is there because mtimes are whole seconds: the caller passes the parent
 * snapshot's start time, ~0 trusts every mtime.  A Dir against Dir pair is an item of the next level;
 * parent children no scan node names are not descended, so nothing under a removed directory is read.
 * Every comparison of hashes and names, the verdict and the sums run on the device.
 *   results[i] (host, one per scan node); read[e] (host, one byte per session entry) = 1 exactly for
 * the Tree entries opened.  Errors never stop the walk and use prune's record with the diff walk's
 * meaning: hash = the hash referred to, parent = the piece that names it (zero for the root),
 * child_pos = its position there (~0 for a next_sibling, 0 for the root), reason = a locate status,
 * BW_RESTORE_ENOTTREE, BW_UNPACK_ERANGE / _ETAG / _EZSTD / _EDIGEST, or BW_RESTORE_EFORMAT (the
 * parser, or a chain of more pieces than the store has entries).  A row whose first piece cannot be
 * read takes no part in the join, so the scan node of its name is NEW; a later piece of an item's
 * chain that cannot be read ends the list there; an unreadable root makes scan node 0 NEW.
 * counts->n_errors > err_cap -> BW_ENOSPC with everything else filled; errs is in no particular order.
 *   Hard limit: a level is indexed in 32 bits.  A scan of more than 2^30 nodes, or a level whose lists
 * hold more than 2^30 rows, ends the call with BW_ENOMEM, as does a device allocation that fails;
 * nothing but read (zeros) is filled in then. */
int bw_parent_match(bw_restore* session, const uint8_t* parent_root, uint64_t trust_before, uint32_t flags,
                    const bw_restore_node* nodes, uint64_t n_nodes, const uint8_t* names, uint64_t names_len,
                    bw_parent_result* results, uint8_t* read, bw_parent_counts* counts, bw_prune_error* errs,
                    uint64_t err_cap);

/* ---- impact: which files of which snapshots a set of lost blobs takes down ----
 * The reference cannot ask this; restic answers it with find --blob / --pack.  Two steps over an open
 * restore session, both synchronous: bw_impact_mark gives every reached entry its taint (each distinct
 * tree blob is opened once, as in bw_prune_mark), bw_impact_paths goes down from the roots and opens
 * only affected paths (as bw_diff_trees opens only changed ones). */
#define BW_IMPACT_SELF 1u  /* the entry's own bytes are lost or refused               */
#define BW_IMPACT_BELOW 2u /* an expanded Tree entry with an affected reference       */
typedef struct bw_impact_counts {
    uint64_t n_trees_expanded; /* tree blobs opened, parsed and expanded (bw_prune_mark's figure without bad[]) */
    uint64_t n_levels;         /* rounds of the walk                                                            */
    uint64_t n_edges;          /* references of expanded pieces that resolve to a Tree entry                    */
    uint64_t n_sweeps;         /* sweeps over the edge list, the one that changed nothing included (>= 1)       */
    uint64_t n_tainted;        /* entries with any taint bit                                                    */
    uint64_t n_errors;         /* always the full number                                                        */
    uint64_t n_roots_affected;
} bw_impact_counts;

/* bad (host, one byte per session entry, or NULL: none): nonzero = treat this entry's bytes as lost.
 * A Tree entry with bad[e] set is never opened, so a what-if question corrupts and reads nothing.
 * flags: BW_UNPACK_VERIFY or 0; chunk payloads are never read, so a damaged chunk that bad[] does not
 * name is not found here (bw_check_data finds it, and its status feeds bad[]).
 *   The walk is bw_prune_mark's, with its rules: level-synchronous from the roots; a frontier of Tree
 * entries not yet expanded goes through the unpack chain `slots` at a time; each distinct Tree entry
 * is expanded once; a hash held by several entries means the entry bw_restore_locate resolves it to;
 * cycles end by themselves.
 *   taint[e] (host, one byte per session entry) is 0 for an entry no root reaches, else the OR of:
 * BW_IMPACT_SELF, set when the entry is reached and bad[e] is nonzero, or it is a Tree entry reached
 * by a tree reference that the unpack chain or the parser refuses (BW_UNPACK_ERANGE / _ETAG / _EZSTD /
 * _EDIGEST, BW_RESTORE_EFORMAT), or it is a FileChunk entry whose range fails prune's range rule;
 * BW_IMPACT_BELOW, set on an expanded Tree entry that has an affected reference among its children
 * rows and its next_sibling.  A reference is affected when locate fails; or it is a tree reference (a
 * Dir row, a next_sibling, a root) that resolves to a FileChunk entry; or it is a tree reference and
 * the entry it resolves to has any taint bit; or it is a row of a File piece and the entry it resolves
 * to has SELF.  File rows look only at SELF because they are never opened; this is conservative in
 * one case: a tree-kind blob that the parser refuses (SELF) but that a File also names as a chunk,
 * which a restore would still read.  BELOW is the least fixed point of that rule over the graph of
 * expanded blobs: the expand kernel settles rows that resolve to FileChunk entries at once and appends
 * an 8-byte (parent entry, child entry) edge for every reference that resolves to a Tree entry; a
 * propagate kernel sweeps the edge list, latest level first, and the sweep is repeated until one
 * changes nothing.
 *   root_affected[r] (host, one byte per root) = 1 when root r's reference is affected.  Errors are
 * bw_prune_mark's records with its meaning and never stop the walk; bad[] itself produces no error
 * record.  counts->n_errors > err_cap -> BW_ENOSPC with everything else filled.  An edge names an
 * entry in 31 bits: a session of 2^31 entries or more -> BW_ENOMEM. */
int bw_impact_mark(bw_restore* session, const uint8_t* roots, uint64_t n_roots, const uint8_t* bad, uint32_t flags,
                   uint8_t* taint, uint8_t* root_affected, bw_impact_counts* counts, bw_prune_error* errs,
                   uint64_t err_cap);

#define BW_IMPACT_UNREADABLE 1u /* the first piece is SELF, unlocatable or not a tree: hash only, empty name, not descended */
#define BW_IMPACT_TRUNCATED 2u  /* a later piece of the chain is lost: the list ends there                                  */
#define BW_IMPACT_CYCLIC 4u     /* the hash is one of its own ancestors' on this path: its list counts as empty             */
typedef struct bw_impact_record {
    uint8_t hash[32];
    uint64_t root;   /* the index of the root it lies under                                              */
    uint64_t parent; /* the record of the item above, ~0 for a root; always lower than the record's own */
    uint64_t name_off, name_len; /* into `names`; empty for an unreadable item                          */
    uint32_t kind;       /* BW_TREE_FILE or BW_TREE_DIR */
    uint32_t meta_flags; /* BW_TREE_HAS_*               */
    uint64_t size, mtime, ctime;
    uint64_t n_children;     /* the rows read: its whole next_sibling chain, as far as it could be read */
    uint64_t n_affected;     /* the affected ones among them                                            */
    uint64_t first_affected; /* the position of the first in the list, ~0 when none                     */
    uint32_t flags;          /* BW_IMPACT_UNREADABLE / _TRUNCATED / _CYCLIC                             */
    uint32_t pad;
} bw_impact_record;
typedef struct bw_impact_root {
    uint64_t n_records, n_files, n_unreadable; /* records under the root; the File ones; the UNREADABLE ones */
    uint64_t lost_chunk_refs;                  /* the sum of the File records' n_affected                     */
} bw_impact_root;
typedef struct bw_impact_paths_counts {
    uint64_t n_records, name_bytes;
    uint64_t n_levels; /* levels of the walk that hold a record */
    uint64_t n_errors; /* always the full number                */
} bw_impact_paths_counts;

/* taint: host, one byte per session entry, as bw_impact_mark returned it (any other bit -> BW_EINVAL);
 * it is uploaded once.  flags: BW_UNPACK_VERIFY or 0.  The walk is a third policy over the tree-chain
 * fetch that the diff walk and the parent match share.
 *   An item is (root index, parent record, tree reference); level 0 holds the affected roots in root
 * order (a root is affected by the rule above).  Per item the first piece is read for its header and
 * name, the whole next_sibling chain is fetched and the rows are concatenated in chain order.  An
 * entry with SELF is never opened.  For a Dir the affected rows become the next level's items;
 * unaffected rows are not opened, so an intact subtree costs nothing.  For a File the affected rows
 * are counted.  Each item gives one record; a level's records follow its items' order.
 *   The same subtree under two roots, or twice under one root, gives records under each: paths belong
 * to snapshots.  per_root[r] (host, one per root) sums the records returned.
 *   Errors never stop the walk and use prune's record with the diff walk's meaning; they are what
 * opening the items meets: a locate status or BW_RESTORE_ENOTTREE for an item's reference, a chain or
 * parser refusal of a piece that taint does not name, and BW_RESTORE_EFORMAT for a CYCLIC item or a
 * chain of more pieces than the store has entries.  A piece that is not opened because of SELF gives
 * no error here: bw_impact_mark reported it, or bad[] named it.
 *   Capacity and hard limit are bw_diff_trees' word for word: the walk stops at the first level whose
 * records or names do not fit and returns BW_ENOSPC with counts holding the totals up to and including
 * that level; the levels before it are filled in, and nothing is written past a cap; per_root is
 * partial then: it sums the levels that were filled in, not the level counts stops at.  counts->n_errors
 * > err_cap -> BW_ENOSPC with everything else filled.  A level is indexed in 32 bits: more than 2^30
 * items or rows in a level ends the call with BW_ENOMEM. */
int bw_impact_paths(bw_restore* session, const uint8_t* roots, uint64_t n_roots, const uint8_t* taint, uint32_t flags,
                    bw_impact_record* records, uint64_t record_cap, uint8_t* names, uint64_t names_cap,
                    bw_impact_root* per_root, bw_impact_paths_counts* counts, bw_prune_error* errs, uint64_t err_cap);

/* ---- retain: which snapshots keep each blob alive, what forgetting a set of them frees ----
 * The reference cannot ask this; restic answers it with stats and forget --dry-run, borg with its
 * "deduplicated size" column.  Two steps over an open restore session, both synchronous: bw_retain_mark
 * walks all roots at once (each distinct tree blob is opened once, as in bw_prune_mark) and gives every
 * entry the set of roots that reach it; bw_retain_drop answers "what if these roots are forgotten" from
 * those sets alone, with no tree read, in the form bw_prune_plan takes. */
#define BW_RETAIN_MAX_ROOTS 4096u
typedef struct bw_retain_root {
    uint64_t reached_blobs, reached_bytes;   /* bytes: 12 + length per entry, prune's convention */
    uint64_t unique_blobs, unique_bytes;     /* entries whose mask is this root's bit alone      */
    uint64_t n_damaged;                      /* damaged entries with this root in their mask     */
    uint32_t status, pad;                    /* 0, or why the root itself could not be walked    */
} bw_retain_root;
typedef struct bw_retain_counts {
    uint64_t n_trees_expanded, n_levels, n_edges, n_sweeps, n_errors;
    uint64_t reached_blobs, reached_bytes, orphan_blobs, orphan_bytes; /* mask != 0 / mask == 0 */
} bw_retain_counts;
typedef struct bw_retain_freed {
    uint64_t freed_blobs, freed_bytes;   /* mask != 0 and every root of it dropped */
    uint64_t live_blobs, live_bytes;     /* some root of the mask kept             */
} bw_retain_freed;

/* W = max(1, ceil(n_roots / 64)).  masks (host, n_entries * W words, entry-major): bit r % 64 of
 * masks[e * W + r / 64] says that root r reaches entry e, which is: bw_prune_mark over the single root r
 * sets live[e].  Bits at or past n_roots are zero.  Two equal roots each have their own bit.
 *   The walk is bw_prune_mark's with its rules.  A Tree entry is opened for root r only when r reaches
 * it through a tree reference (a root, a Dir's child row, a next_sibling); a File row that names a Tree
 * entry reaches it and does not open it.  So two sets are kept per entry, reach and open: root i seeds
 * bit i into both sets of the entry it locates to (into reach alone when that is a FileChunk entry);
 * for every reference of an expanded entry p that locates to c, reach(c) |= open(p), and when it is a
 * tree reference and c a Tree entry also open(c) |= open(p); the sets are the least fixed point of that
 * rule.  The expand kernel appends an 8-byte edge per located reference, a propagate kernel sweeps the
 * edges between Tree entries earliest level first until a sweep changes nothing (n_sweeps, >= 1), and
 * the other edges are settled in one pass after that.  n_edges counts both kinds.
 *   damaged[e] (host, one byte per entry) is nonzero when e is a reached FileChunk entry whose range
 * fails prune's range rule, or a queued Tree entry that could not be expanded (BW_UNPACK_ERANGE / _ETAG
 * / _EZSTD / _EDIGEST, BW_RESTORE_EFORMAT), or an expanded Tree entry that holds a reference that does
 * not locate or a tree reference to a FileChunk entry.  per_root[r].status is the locate status of root
 * r's own reference, or BW_RESTORE_ENOTTREE, else 0.  A snapshot is complete when status == 0 and
 * n_damaged == 0; otherwise what lies below the damage was not seen and its figures are lower bounds.
 *   Errors are bw_prune_mark's records, the same multiset as bw_prune_mark over the same roots, and
 * never stop the walk; counts->n_errors > err_cap -> BW_ENOSPC with everything else filled.  flags:
 * BW_UNPACK_VERIFY or 0.  n_roots > BW_RETAIN_MAX_ROOTS, or a session of 2^31 entries or more ->
 * BW_ENOMEM.  With no roots every mask is zero and every entry an orphan. */
int bw_retain_mark(bw_restore* session, const uint8_t* roots, uint64_t n_roots, uint32_t flags,
                   uint64_t* masks, uint8_t* damaged, bw_retain_root* per_root, bw_retain_counts* counts,
                   bw_prune_error* errs, uint64_t err_cap);

/* masks: as bw_retain_mark returned them for n_roots roots.  drop (host, n_sets * W words): one root set
 * per question.  live (host, n_sets * n_entries bytes, or NULL): live[q * n_entries + e] = 1 when
 * masks[e] & ~drop[q] is nonzero.  stats (host, n_sets * n_packfiles records, or NULL): bw_prune_mark's
 * per-packfile sums for that live vector.  freed: n_sets records.  For a sound store live and stats are
 * what bw_prune_mark over the kept roots returns, and go straight into bw_prune_plan.  A mask or drop
 * word with a bit at or past n_roots -> BW_EINVAL; n_roots > BW_RETAIN_MAX_ROOTS -> BW_ENOMEM. */
int bw_retain_drop(bw_restore* session, const uint64_t* masks, uint64_t n_roots, const uint64_t* drop,
                   uint64_t n_sets, uint8_t* live, bw_prune_packfile_stat* stats, bw_retain_freed* freed);

/* ---- find: which paths of which snapshots match a set of patterns ----
 * The reference cannot ask this; restic answers it with find and restore --include.  One synchronous
 * call over an open restore session: a fourth policy over the tree-chain fetch that the diff walk, the
 * parent match and impact's report walk share, and a bit-parallel glob automaton whose state is carried
 * down the path, so that a directory no pattern can match below is never opened.
 *   A pattern is a valid UTF-8 byte string matched against an item's path: its names from the root's
 * child down, joined by '/'.  The root itself has the path "" and never matches.  Within a component
 * '*' matches zero or more bytes other than '/', '?' one code point other than '/', [abc] [a-z] [!a-z]
 * [^a-z] are classes of ASCII members (a negated class matches one code point that is not in it and is
 * not '/'), \x is a literal x, any other byte is a literal.  A component that is exactly ** stands for
 * zero or more whole components.  A leading '/' anchors the pattern at the root's children; without one
 * it floats, as if it began with a ** component.  A trailing '/' means directories only.  BW_EINVAL with
 * the reason in bw_last_error: an empty pattern or component (a//b), an unterminated class, a dangling
 * backslash, invalid UTF-8, a class member that is not ASCII, a '/' inside a class or behind a
 * backslash, a class range that runs backwards, a pattern that needs more than 64 automaton states (a
 * state per literal byte, '?', class and run of '*', one per component end, one per run of ** components,
 * one for floating).  BW_FIND_ICASE folds ASCII letters only. */
#define BW_FIND_MAX_PATTERNS 32u
#define BW_FIND_ICASE   2u  /* ASCII case folding */
#define BW_FIND_SUBTREE 4u  /* everything below a Dir that a pattern matches is matched by that pattern too */
#define BW_FIND_CHUNKS  8u  /* fetch the chunk rows of the File records that are hits */
/* BW_UNPACK_VERIFY (1) may be OR-ed in as for the other walks */

#define BW_FIND_HIT        1u
#define BW_FIND_UNREADABLE 2u  /* first piece unlocatable, not a tree, or refused: hash only, empty name, not matched, not descended */
#define BW_FIND_TRUNCATED  4u  /* a later piece of its chain is lost: the list ends there */
#define BW_FIND_CYCLIC     8u  /* its hash is one of its ancestors' on this path: not descended */
#define BW_FIND_PRUNED    16u  /* a Dir no pattern can match below: its rows were never fetched */

typedef struct bw_find_query {
    const uint8_t* patterns;     /* the patterns' bytes back to back */
    const uint64_t* pattern_off; /* n_patterns + 1 offsets */
    uint32_t n_patterns, kinds;  /* kinds: bit BW_TREE_FILE, bit BW_TREE_DIR (1u << kind); 0 = both */
    uint64_t size_min, size_max, mtime_min, mtime_max; /* inclusive; 0 .. ~0 = no filter */
} bw_find_query;
typedef struct bw_find_record {
    uint8_t hash[32];
    uint64_t root, parent;           /* parent: the record of the item above, ~0 for a root; always lower than its own */
    uint64_t name_off, name_len;     /* into `names`; empty for an unreadable item */
    uint32_t kind, meta_flags;       /* BW_TREE_FILE / _DIR; BW_TREE_HAS_* */
    uint64_t size, mtime, ctime;
    uint64_t child_first, n_children; /* Dir: its rows read and the record of the first (they are consecutive records; 0, 0
                                         when PRUNED, CYCLIC or empty); File with BW_FIND_CHUNKS and HIT: its rows in `chunks` */
    uint32_t patterns;                /* the patterns that match its path, inherited ones included */
    uint32_t flags;                   /* BW_FIND_HIT / _UNREADABLE / _TRUNCATED / _CYCLIC / _PRUNED */
} bw_find_record;
typedef struct bw_find_root   { uint64_t n_records, n_hits, n_hit_files, hit_bytes, n_unreadable; } bw_find_root;
typedef struct bw_find_counts { uint64_t n_records, name_bytes, n_chunks, n_levels, n_opened, n_pruned, n_errors; } bw_find_counts;

/* roots: host, 32 bytes each.  flags: BW_FIND_* and BW_UNPACK_VERIFY.  records, names, chunks (32 bytes a
 * row), per_root (one per root) and errs are host arrays.
 *   Levels.  An item is (root index, parent record, tree reference, carried states: one 64-bit state set
 * per pattern).  Level 0 is every root in root order; a root's record is never a hit and carries no
 * pattern bit, and its children start from the patterns' initial states.
 *   Per level only the first piece of every item is opened, for its header and name (the parent match's
 * second fetch).  The match kernel runs each item's name through every pattern from its parent's carried
 * states: a pattern bit is set when the state after the name accepts (a trailing '/' requires kind Dir),
 * and with BW_FIND_SUBTREE also when the parent has it.  HIT is set when patterns != 0 and the kind, size
 * and mtime filters hold; an item without BW_TREE_HAS_SIZE or BW_TREE_HAS_MTIME fails a filter on that
 * field that is narrower than 0 .. ~0.  A Dir's carried states are the states after a further '/'.  A
 * Dir is PRUNED when every carried state is empty and it hands no pattern bit down.  Then the rows of
 * every Dir item that is not PRUNED, CYCLIC or UNREADABLE are fetched, the whole next_sibling chain in
 * chain order, and every row becomes an item of the next level, in row order.
 *   Records.  Every item gives one record, hits, misses and unreadable items alike, in level order and
 * item order within the level, so every hit's ancestors are records and a path is the parent chain.  A
 * Dir's children are the records child_first .. child_first + n_children.  The same subtree under two
 * roots, or twice under one root, gives records under each.
 *   Chunk rows.  With BW_FIND_CHUNKS the chains of the File records with HIT are fetched after their
 * level and their rows land in `chunks` in record order; without it no File's rows are read.
 * chunks_cap > 0 without the flag is allowed and unused.
 *   Counts.  n_opened counts the tree blobs handed to the unpack chain: one per located first piece,
 * one per located piece of a chain that is fetched (the first piece again: a fetch decodes what it
 * opens once, and keeps nothing between fetches).  n_pruned counts the PRUNED records.  per_root sums the
 * records returned; hit_bytes sums the sizes of hit Files.
 *   Errors never stop the walk and use prune's record with the diff walk's meaning: a locate status or
 * BW_RESTORE_ENOTTREE for an item's reference, a chain or parser refusal of a piece, and
 * BW_RESTORE_EFORMAT for a CYCLIC item or a chain of more pieces than the store has entries.
 *   Capacity and hard limit are bw_impact_paths' word for word: the walk stops at the first level whose
 * records, names or chunk rows do not fit and returns BW_ENOSPC with counts holding the totals up to and
 * including that level; the levels before it are filled in, and nothing is written past a cap; per_root
 * is partial then.  counts->n_errors > err_cap -> BW_ENOSPC with everything else filled.  A level is
 * indexed in 32 bits: more than 2^30 items or rows in a level ends the call with BW_ENOMEM.
 * n_patterns == 0 or > BW_FIND_MAX_PATTERNS, a kinds bit other than the two, or a refused pattern ->
 * BW_EINVAL. */
int bw_find_paths(bw_restore* session, const uint8_t* roots, uint64_t n_roots, const bw_find_query* query, uint32_t flags,
                  bw_find_record* records, uint64_t record_cap, uint8_t* names, uint64_t names_cap,
                  uint8_t* chunks, uint64_t chunks_cap, bw_find_root* per_root, bw_find_counts* counts,
                  bw_prune_error* errs, uint64_t err_cap);

/* ---- check: is this store sound, are these bytes still the bytes that were sealed ----
 * The reference never verifies what it has written; this goes past it as prune does.  Three layers,
 * all synchronous: bw_auth(_device) recomputes AES-GCM tags without decrypting, bw_check_structure
 * cross-checks headers and index items without reading a blob byte, bw_check_data reads every
 * selected entry's bytes.  The last two work over an open restore session and change nothing in it. */

/* bw_open_device's verdicts without its plaintext: the same tables minus d_dst and dst_off.
 * src_len[i] includes the tag (>= 16, else BW_EINVAL); ok[i] (host) = 1 exactly where bw_open_device
 * sets ok[i] = 1, for every input.  The tag is recomputed from the ciphertext alone (GHASH, plus two
 * AES blocks per item for H and E(J0)); the key comes from prk, so only its owner can make a tag
 * verify.  The source ranges are read once and no byte of device memory outside the context's own
 * scratch is written. */
int bw_auth_device(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* d_src, const uint64_t* src_off,
                   const uint64_t* src_len, uint64_t n, const uint8_t* info, uint32_t info_len,
                   const uint8_t* nonces, uint8_t* ok);
/* Same over a host buffer: the source is uploaded and nothing but ok comes back. */
int bw_auth(bw_ctx* ctx, const uint8_t prk[32], const uint8_t* src, const uint64_t* src_off,
            const uint64_t* src_len, uint64_t n, const uint8_t* info, uint32_t info_len,
            const uint8_t* nonces, uint8_t* ok);

/* Per-entry bits of bw_check_structure. */
#define BW_CHECK_E_RANGE 1u     /* 12 + length leaves the packfile's blob section, or length < 16: BW_UNPACK_ERANGE's rule */
#define BW_CHECK_E_ORDER 2u     /* offset != the sum of 12 + length over the earlier entries of the packfile */
#define BW_CHECK_E_UNINDEXED 4u /* no index item is (this hash, this packfile's id): restore never finds it   */
#define BW_CHECK_E_SHADOWED 8u  /* an earlier entry of the packfile has the hash: the header scan stops there */
/* Statuses beside BW_UNPACK_* and BW_RESTORE_* (which they never collide with). */
enum {
    BW_CHECK_SKIPPED = 32,   /* bw_check_data: the entry was not selected                               */
    BW_CHECK_IDUPLICATE = 33 /* bw_check_structure: the item equals, in both fields, an item before it  */
};
typedef struct bw_check_packfile_stat {
    uint64_t n_entries;
    uint64_t n_range, n_order, n_unindexed, n_shadowed; /* entries with the flag                       */
    uint64_t claimed_bytes; /* the sum of 12 + length over the packfile's entries                       */
    uint64_t section_bytes; /* size - 8 - header_len (0 when the header alone exceeds the size)         */
    int64_t tail;           /* section_bytes - claimed_bytes: < 0 truncated, > 0 trailing bytes         */
} bw_check_packfile_stat;
typedef struct bw_check_counts {
    uint64_t n_entries, n_range, n_order, n_unindexed, n_shadowed, claimed_bytes, section_bytes; /* sums */
    uint64_t n_items_ok, n_items_nopackfile, n_items_mismatch, n_items_duplicate;
    uint64_t n_packfiles_clean; /* packfiles without a flagged entry and with tail == 0                 */
} bw_check_counts;

/* Everything that needs no blob byte, from the session's device copies of the entries, the index
 * items, the ids and its two locator tables.  The session's entries must come in packfile order, as
 * bw_unpack_headers returns them (else BW_EINVAL).  All outputs are host arrays.
 *   entry_flags[e] (one byte per session entry): BW_CHECK_E_* bits.  A shadowed entry is not also
 *     reported unindexed.  The expected offsets come from one segmented exclusive sum over all entries
 *     (segments = packfiles), so a packfile of 100,000 entries and 1,000 packfiles of one entry cost the same.
 *   item_status[i] (one byte per index item): BW_RESTORE_OK; BW_RESTORE_ENOPACKFILE, the id is not
 *     among the session's ids; BW_RESTORE_EMISMATCH, that packfile's header lacks the hash;
 *     BW_CHECK_IDUPLICATE, an item with a lower index has the same hash and id (the lowest of such a
 *     group is OK; which one wins does not depend on scheduling).  An item that does not resolve
 *     keeps its own status however often it is repeated.
 *   stats[p]: one record per packfile; *counts: their sums, the four item statuses, the clean packfiles.
 * A session without entries, items or packfiles is fine: BW_OK and zeros. */
int bw_check_structure(bw_restore* session, uint8_t* entry_flags, uint8_t* item_status, bw_check_packfile_stat* stats,
                       bw_check_counts* counts);

/* Every selected entry's bytes.  select: one byte per session entry, NULL = all; status[e] (host,
 * one byte per session entry): BW_CHECK_SKIPPED for an entry not selected, BW_UNPACK_ERANGE for one
 * with BW_CHECK_E_RANGE (it is never read), else by mode:
 *   BW_CHECK_AUTH: the blob is authenticated where it lies in the session's packfiles (bw_auth_device's
 *     path: nonce at 8 + header_len + offset, key info = the entry's hash): BW_UNPACK_OK or _ETAG.  No
 *     decode slot is used and nothing is decrypted; the selection goes in one launch sequence.
 *   BW_CHECK_FULL: the unpack chain with BW_UNPACK_VERIFY, `slots` entries at a time as
 *     bw_restore_files_device drives it: BW_UNPACK_OK, _ETAG, _EZSTD or _EDIGEST; an entry of kind
 *     Tree that passes is parsed in its slot, and BW_RESTORE_EFORMAT is what the parser refuses.  No
 *     regenerated byte leaves the device.
 * For every selected entry, the AUTH status is BW_UNPACK_OK exactly when the FULL status is neither
 * BW_UNPACK_ETAG nor BW_UNPACK_ERANGE. */
#define BW_CHECK_AUTH 1u
#define BW_CHECK_FULL 2u
int bw_check_data(bw_restore* session, uint32_t mode, const uint8_t* select, uint8_t* status);

/* ---- rekey: the store of an open restore session under a new secret ----
 * The session holds the old PRK, the packfiles on the device, the entries and the ids.  d_out (device)
 * receives the same packfile table -- the same offsets, sizes and ids -- with packfile p laid out as
 *   u64 header_len || header resealed (info "header", nonce = id) || per entry: nonce copied || blob
 *   resealed (info = the entry's hash)
 * through bw_reseal_device's path, headers and blobs in one launch sequence: no plaintext is stored.
 *   entry_status[e] (host, one byte per session entry): BW_UNPACK_OK or BW_UNPACK_ETAG (the output's
 *     tag is then the complement of the valid one); BW_UNPACK_ERANGE for an entry that leaves its
 *     packfile's blob section (it is never read).
 *   packfile_status[p] (host): the header's verdict, BW_UNPACK_OK or BW_UNPACK_ETAG; BW_UNPACK_ERANGE
 *     where 8 + header_len exceeds the packfile or header_len < 16 (the header is copied as it is).
 * Every byte of a packfile that no in-range entry and no header covers (the length prefix, the nonces,
 * trailing bytes of a blob section) is copied as it is.  Two in-range entries of one packfile whose
 * ranges (nonce and sealed bytes) overlap: BW_EINVAL before anything is written.  d_out must not overlap
 * the session's packfiles.  An empty session returns BW_OK.  Synchronous. */
int bw_rekey_store_device(bw_restore* session, const uint8_t new_prk[32], uint8_t* d_out, uint8_t* entry_status,
                          uint8_t* packfile_status);
/* Same into a host buffer of the packfile table's extent: only the packfiles' ranges are written. */
int bw_rekey_store(bw_restore* session, const uint8_t new_prk[32], uint8_t* out, uint8_t* entry_status,
                   uint8_t* packfile_status);

/* ---- parity: Reed-Solomon shards over packfiles, and repair from them ----
 * The reference has no redundancy: one lost packfile loses every file with a chunk in it.  A parity
 * group is k data shards (packfiles, byte for byte as stored, zero-extended to the group's shard_len)
 * and m parity shards over GF(2^8) with the polynomial 0x11d and the generator 2:
 *   P_i[b] = XOR_j mul(C[i][j], D_j[b]),  C[i][j] = inv(i ^ (m + j)),  0 <= i < m, 0 <= j < k, b < shard_len
 * (a Cauchy matrix: any k of the k + m shards rebuild the rest; C[i][j] does not depend on k, so a
 * short last group uses the leading columns).  1 <= k, 1 <= m, k + m <= 256. */

/* The primitive: dst_r[b] = XOR_c mul(matrix[r * cols + c], src_c[b]) for b < len, r < rows (k_gf_matmul,
 * one launch).  Source c is d_src[src_off[c] ..] at any alignment and reads as zero at and beyond
 * src_len[c]; destination r is d_dst[dst_off[r] .. dst_off[r] + len).  d_dst and every dst_off must be
 * 16-byte aligned, rows >= 1 and 1 <= cols <= 255, else BW_EINVAL.  Every byte of every destination
 * range is written (a zero row writes zeros), nothing else is, and no source byte at or beyond its
 * src_len is read.  Destinations must not overlap each other or a source.  matrix and the tables are
 * host arrays.  Synchronous. */
int bw_gf_matmul_device(bw_ctx* ctx, const uint8_t* matrix, uint32_t rows, uint32_t cols, const uint8_t* d_src,
                        const uint64_t* src_off, const uint64_t* src_len, uint8_t* d_dst, const uint64_t* dst_off,
                        uint64_t len);
/* Same over host buffers: the sources are uploaded and only the destination ranges come back. */
int bw_gf_matmul(bw_ctx* ctx, const uint8_t* matrix, uint32_t rows, uint32_t cols, const uint8_t* src,
                 const uint64_t* src_off, const uint64_t* src_len, uint8_t* dst, const uint64_t* dst_off, uint64_t len);

typedef struct bw_parity_group {
    uint64_t first_packfile; /* position in the packfile table of the group's first data shard        */
    uint32_t k, m;           /* data shards (consecutive packfiles), parity shards                      */
    uint64_t shard_len;      /* the largest member's size rounded up to 16                              */
    uint64_t out_offset;     /* parity shard i lies at out_offset + i * shard_len of the parity buffer  */
} bw_parity_group;

/* Host only.  Groups take consecutive packfiles in table order, k per group, the last one the
 * remainder; offsets are 16-aligned and back to back, *out_bytes their end.  A size of 0, k or m of 0
 * or k + m > 256 -> BW_EINVAL; cap too small -> BW_ENOSPC with *n_groups and *out_bytes set. */
int bw_parity_plan(const uint64_t* sizes, uint64_t n_pf, uint32_t k, uint32_t m, bw_parity_group* out, uint64_t cap,
                   uint64_t* n_groups, uint64_t* out_bytes);

/* Every parity shard of every group into d_out (device, 16-byte aligned, out_cap bytes), all groups in
 * one k_gf_matmul launch over d_packfiles (device; packfile p at packfiles[p].offset, .size bytes).
 * digests (host): the BLAKE3 of every shard, 32 bytes each, group by group, data shards then parity
 * shards (32 * (n_pf + sum of m) bytes for a plan that covers the table); data shards are hashed at
 * their true size, parity shards at shard_len, through the device hashing of the verified unpack chain.
 * A group that leaves the table or the output, a shard_len below a member's size or no multiple of 16,
 * a misaligned out_offset -> BW_EINVAL before anything is written.  Synchronous. */
int bw_parity_build_device(bw_ctx* ctx, const uint8_t* d_packfiles, const bw_packfile* packfiles, uint64_t n_pf,
                           const bw_parity_group* groups, uint64_t n_groups, uint8_t* d_out, uint64_t out_cap,
                           uint8_t* digests);
/* Same over host buffers (data of the packfile table's extent, out of out_cap bytes). */
int bw_parity_build(bw_ctx* ctx, const uint8_t* data, const bw_packfile* packfiles, uint64_t n_pf,
                    const bw_parity_group* groups, uint64_t n_groups, uint8_t* out, uint64_t out_cap, uint8_t* digests);

/* Host only.  present[s] != 0: shard s of the k + m (data shards first) is at hand.  used[0 .. k): the
 * inputs, every present data shard and then the lowest-numbered present parity shards; missing[0 ..
 * *n_missing): the absent shards, ascending (room for k + m entries); matrix (*n_missing x k, row-major,
 * room for (k + m) * k bytes): row r times the inputs in the order of `used` is shard missing[r], data
 * and parity alike (Gauss-Jordan inverse over GF(2^8), times the Cauchy rows for missing parity).
 * Fewer than k present -> BW_ETOOFEW with missing and *n_missing set. */
int bw_parity_solve(uint32_t k, uint32_t m, const uint8_t* present, uint32_t* used, uint32_t* missing,
                    uint32_t* n_missing, uint8_t* matrix);

/* Per-shard status of bw_parity_repair. */
enum {
    BW_PARITY_OK = 0,          /* present (and, with digests, authentic); nothing written               */
    BW_PARITY_DAMAGED = 1,     /* present, its digest differs: not used as an input, rebuilt, and good   */
    BW_PARITY_REBUILT = 2,     /* missing, rebuilt (with digests: and its digest agrees)                 */
    BW_PARITY_REBUILT_BAD = 3, /* rebuilt, but its digest differs or bytes beyond its size are not zero  */
    BW_PARITY_LOST = 4         /* more than m shards missing or damaged: nothing was written             */
};

/* One group.  Shard s (data shards 0 .. k, then parity) lies, where present[s] != 0, at
 * d_shards[shard_off[s] ..] with shard_size[s] bytes: a packfile's true size (<= shard_len) or shard_len
 * for a parity shard, else BW_EINVAL.  digests (host, (k + m) x 32 as bw_parity_build returned them, may
 * be NULL): present shards are hashed first and one whose digest differs is demoted to missing, so a
 * damaged survivor is never an input; rebuilt shards are hashed at shard_size.  Every missing or demoted
 * shard s is written at d_out[out_off[s] ..], shard_len bytes (16-byte aligned; the caller keeps
 * shard_size[s] of them), by one k_gf_matmul launch; a rebuilt data shard whose bytes beyond shard_size
 * are not zero is BW_PARITY_REBUILT_BAD even without digests.  status[s] (host): BW_PARITY_*.  With more
 * than m shards gone the call returns BW_OK, every gone shard is BW_PARITY_LOST and nothing is written.
 * Synchronous. */
int bw_parity_repair_device(bw_ctx* ctx, const bw_parity_group* group, const uint8_t* present, const uint8_t* d_shards,
                            const uint64_t* shard_off, const uint64_t* shard_size, const uint8_t* digests, uint8_t* d_out,
                            const uint64_t* out_off, uint8_t* status);
/* Same over host buffers: only the rebuilt shards' ranges of out are written (shard_len bytes each). */
int bw_parity_repair(bw_ctx* ctx, const bw_parity_group* group, const uint8_t* present, const uint8_t* shards,
                     const uint64_t* shard_off, const uint64_t* shard_size, const uint8_t* digests, uint8_t* out,
                     const uint64_t* out_off, uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* BACKUWUP_GPU_PACK_H */
