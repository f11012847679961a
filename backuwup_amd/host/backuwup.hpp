// backuwup.hpp -- C++ host-side mirror of the reference's call sites, over the C ABI.
//
// The reference is Rust; there is no Rust toolchain in this image, so the host side of the
// boundary is written in C++ (the reference is compiled code) with the reference's names,
// argument meaning and error behaviour.  A Rust maintainer binds the same C ABI instead
// (INTEGRATION.md).  Header-only; link with -lbackuwup_amd.
//
//   fastcdc::v2020::FastCDC / Chunk    client/src/backup/filesystem/dir_packer.rs:254-266
//   blake3::hash                       dir_packer.rs:286
//   packfile::BlobIndex                packfile/blob_index.rs:44-148
//   packfile::Manager::add_blob gate   packfile/pack.rs:31-39
//   dir_packer::process_file           dir_packer.rs:231-282 (batched over many files)
//   Tree / split_serialize_tree / add_tree_to_blobs   filesystem/mod.rs:63-77, dir_packer.rs:314-390
//   Manager::write_packfiles / serialize_packfile      packfile/pack.rs:115-227
//   compress_encrypt_blob (zstd level 3) + write_packfiles   packfile/pack.rs:58-80
//   BlobIndex::flush / load (index files)              packfile/blob_index.rs:151-240
//   Pool (the drop-ins over every GPU of the node)     client/src/main.rs:43, dir_packer.rs:166
//   NodeSession (N ranks in one process)               client/src/backup/mod.rs:64, blob_index.rs:130-148
#pragma once

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdint>
#include <exception>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/backuwup_gpu.h"

namespace backuwup {

using BlobHash = std::array<uint8_t, 32>;  // shared/src/types.rs:31

struct Error : std::runtime_error {
    int rc;
    Error(int r, const std::string& m) : std::runtime_error(m), rc(r) {}
};

inline void check(int rc, bw_ctx* ctx = nullptr) {
    if (rc != BW_OK) {
        std::string m = bw_strerror(rc);
        if (ctx) m += std::string(": ") + bw_last_error(ctx);
        throw Error(rc, m);
    }
}

// One GPU context: stream, workspaces, the in-HBM index.  Not thread-safe (the reference
// serialises index access under the packer mutex, packfile/mod.rs:77).
class Context {
public:
    explicit Context(int device = 0) { check(bw_create(device, &h_)); }
    ~Context() { bw_destroy(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    bw_ctx* get() const { return h_; }

private:
    bw_ctx* h_ = nullptr;
};

namespace fastcdc {
namespace v2020 {

constexpr uint32_t MINIMUM_MIN = BW_MINIMUM_MIN, MINIMUM_MAX = BW_MINIMUM_MAX;
constexpr uint32_t AVERAGE_MIN = BW_AVERAGE_MIN, AVERAGE_MAX = BW_AVERAGE_MAX;
constexpr uint32_t MAXIMUM_MIN = BW_MAXIMUM_MIN, MAXIMUM_MAX = BW_MAXIMUM_MAX;

struct Chunk {
    uint64_t hash;
    size_t offset;
    size_t length;
};

// FastCDC::new(source, min_size, avg_size, max_size): the crate panics on out-of-range sizes;
// here the constructor throws Error(BW_EINVAL).  Iterating yields the chunks in order.
class FastCDC {
public:
    FastCDC(Context& ctx, const uint8_t* source, size_t len, uint32_t min_size, uint32_t avg_size,
            uint32_t max_size) {
        const uint32_t s0 = 2 * (min_size / 2);
        const uint32_t mc = s0 < max_size ? s0 : max_size;
        std::vector<bw_chunk> out(len / (mc ? mc : 1) + 2);
        uint64_t n = 0;
        check(bw_fastcdc_chunks(ctx.get(), source, len, min_size, avg_size, max_size, out.data(), out.size(), &n),
              ctx.get());
        chunks_.reserve(n);
        for (uint64_t i = 0; i < n; i++) chunks_.push_back({out[i].hash, out[i].offset, out[i].length});
    }
    // The Rust drop-in's form (rust/backuwup-gpu FastCDC::new): chunks AND hashes the source in one
    // submit on a context of `pool` (any type with with_context, i.e. backuwup::Pool) and keeps the
    // digests until destruction, so Pool::hash of one of these chunk slices is answered without a
    // second trip (bw_fastcdc_chunks_hashed); the source must stay unchanged meanwhile.
    template <class P, class = decltype(std::declval<P&>().home_device())>
    FastCDC(P& pool, const uint8_t* source, size_t len, uint32_t min_size, uint32_t avg_size, uint32_t max_size) {
        const uint32_t s0 = 2 * (min_size / 2);
        const uint32_t mc = s0 < max_size ? s0 : max_size;
        std::vector<bw_chunk> out(len / (mc ? mc : 1) + 2);
        uint64_t n = 0;
        pool.with_context([&](Context& ctx) {
            check(bw_fastcdc_chunks_hashed(ctx.get(), source, len, min_size, avg_size, max_size, out.data(), out.size(),
                                           &n, &kept_),
                  ctx.get());
            return 0;
        });
        chunks_.reserve(n);
        for (uint64_t i = 0; i < n; i++) chunks_.push_back({out[i].hash, out[i].offset, out[i].length});
    }
    ~FastCDC() { bw_fastcdc_release(kept_); }
    FastCDC(const FastCDC&) = delete;
    FastCDC& operator=(const FastCDC&) = delete;
    std::vector<Chunk>::const_iterator begin() const { return chunks_.begin(); }
    std::vector<Chunk>::const_iterator end() const { return chunks_.end(); }
    size_t size() const { return chunks_.size(); }

private:
    std::vector<Chunk> chunks_;
    uint64_t kept_ = 0;  // bw_fastcdc_release(0) is a no-op
};

}  // namespace v2020
}  // namespace fastcdc

namespace blake3 {
inline BlobHash hash(Context& ctx, const uint8_t* data, size_t len) {
    BlobHash h{};
    check(bw_blake3_hash(ctx.get(), data, len, h.data()), ctx.get());
    return h;
}
}  // namespace blake3

// packfile::blob_index::BlobIndex -- lives in HBM; `load` seeds it with the prior backups'
// sorted items (blob_index.rs:167-200); `is_blob_duplicate` answers in canonical order and
// inserts a new blob (the blobs_queued insert of blob_index.rs:109).
class BlobIndex {
public:
    explicit BlobIndex(Context& ctx, uint64_t capacity_hint = 0) : ctx_(ctx) {
        check(bw_index_reset(ctx.get(), capacity_hint), ctx.get());
    }
    void load(const std::vector<BlobHash>& sorted_items) {
        check(bw_index_seed(ctx_.get(), sorted_items.empty() ? nullptr : sorted_items[0].data(), sorted_items.size()),
              ctx_.get());
    }
    bool is_blob_duplicate(const BlobHash& h) {
        uint8_t dup = 0;
        check(bw_index_check_insert(ctx_.get(), h.data(), 1, &dup), ctx_.get());
        return dup != 0;
    }
    std::vector<uint8_t> is_blob_duplicate_many(const std::vector<BlobHash>& hs) {
        std::vector<uint8_t> dup(hs.size());
        if (!hs.empty()) check(bw_index_check_insert(ctx_.get(), hs[0].data(), hs.size(), dup.data()), ctx_.get());
        return dup;
    }
    uint64_t size() {
        uint64_t n = 0;
        check(bw_index_size(ctx_.get(), &n), ctx_.get());
        return n;
    }

private:
    Context& ctx_;
};

struct BlobTooLarge : Error {
    BlobTooLarge() : Error(BW_EINVAL, "Blob too large") {}
};

// The dedup gate of packfile::Manager::add_blob (pack.rs:31-39): BlobTooLarge above 3 MiB,
// nullopt-like `false` for a duplicate (Ok(None)), `true` when the blob goes on to be packed.
inline bool add_blob_gate(BlobIndex& index, const BlobHash& h, size_t len) {
    if (len > BW_BLOB_MAX_UNCOMPRESSED_SIZE) throw BlobTooLarge();
    return !index.is_blob_duplicate(h);
}

// process_file for a batch of files laid out back to back: CDC for files > 1 MiB, one blob per
// smaller (or empty) file, blake3 per blob, dedup verdict per blob -- canonical order.
inline std::vector<bw_blob> process_files(Context& ctx, const uint8_t* data, size_t data_len,
                                          const std::vector<uint64_t>& file_off,
                                          const std::vector<uint64_t>& file_len, const bw_params* params = nullptr) {
    bw_params p;
    if (params) p = *params;
    else bw_params_default(&p);
    const uint32_t s0 = 2 * (p.min_size / 2);
    const uint64_t mc = s0 < p.max_size ? s0 : p.max_size;
    uint64_t cap = 1;
    for (uint64_t l : file_len) cap += l / (mc ? mc : 1) + 2;
    std::vector<bw_blob> out(cap);
    uint64_t n = 0;
    check(bw_process_files(ctx.get(), data, data_len, file_off.data(), file_len.data(), file_off.size(), &p,
                           out.data(), cap, &n),
          ctx.get());
    out.resize(n);
    return out;
}

enum class TreeKind : uint32_t { File = BW_TREE_FILE, Dir = BW_TREE_DIR };

struct TreeMetadata {  // filesystem/mod.rs:63-68
    std::optional<uint64_t> size, mtime, ctime;
};

struct Tree {  // filesystem/mod.rs:70-77 (next_sibling is set by the split, not by callers)
    TreeKind kind = TreeKind::File;
    std::string name;
    TreeMetadata metadata;
    std::vector<BlobHash> children;
};

inline bw_tree to_c(const Tree& t) {
    bw_tree c{};
    c.kind = (uint32_t)t.kind;
    c.flags = (t.metadata.size ? BW_TREE_HAS_SIZE : 0) | (t.metadata.mtime ? BW_TREE_HAS_MTIME : 0) |
              (t.metadata.ctime ? BW_TREE_HAS_CTIME : 0);
    c.size = t.metadata.size.value_or(0);
    c.mtime = t.metadata.mtime.value_or(0);
    c.ctime = t.metadata.ctime.value_or(0);
    c.name = (const uint8_t*)t.name.data();
    c.name_len = t.name.size();
    c.children = t.children.empty() ? nullptr : t.children[0].data();
    c.n_children = t.children.size();
    return c;
}

// bincode::serialize(&tree) of one piece (dir_packer.rs:318)
inline std::vector<uint8_t> serialize(const Tree& t, const BlobHash* next_sibling = nullptr) {
    const bw_tree c = to_c(t);
    uint64_t n = 0;
    const int rc = bw_tree_serialize(&c, next_sibling ? next_sibling->data() : nullptr, nullptr, 0, &n);
    if (rc != BW_ENOSPC) check(rc);
    std::vector<uint8_t> out(n);
    check(bw_tree_serialize(&c, next_sibling ? next_sibling->data() : nullptr, out.data(), n, &n));
    return out;
}

// add_tree_to_blobs for many trees: every piece through the dedup gate in canonical order;
// returns the hash each tree contributes to its parent (its first piece's hash).
inline std::vector<BlobHash> add_trees_to_blobs(Context& ctx, const std::vector<Tree>& trees,
                                                std::vector<bw_tree_blob>* pieces = nullptr) {
    std::vector<bw_tree> c;
    c.reserve(trees.size());
    uint64_t cap = 0;
    for (const Tree& t : trees) {
        c.push_back(to_c(t));
        cap += t.children.size() <= BW_TREE_BLOB_MAX_CHILDREN
                   ? 1
                   : (t.children.size() + BW_TREE_BLOB_MAX_CHILDREN - 1) / BW_TREE_BLOB_MAX_CHILDREN;
    }
    std::vector<BlobHash> hashes(trees.size());
    std::vector<bw_tree_blob> out(pieces ? cap : 0);
    uint64_t n = 0;
    check(bw_tree_blobs(ctx.get(), c.data(), c.size(), 0, hashes.empty() ? nullptr : hashes[0].data(),
                        pieces ? out.data() : nullptr, cap, &n),
          ctx.get());
    if (pieces) *pieces = std::move(out);
    return hashes;
}

// ------------------------------------------------------------------ packfiles (pack.rs:115-227)
using PackfileId = std::array<uint8_t, 12>;  // shared/src/types.rs
using BlobNonce = std::array<uint8_t, 12>;
enum class BlobKind : uint8_t { FileChunk = BW_BLOB_FILE_CHUNK, Tree = BW_BLOB_TREE };  // filesystem/mod.rs:13-17

struct Blob {  // filesystem/mod.rs:46-51 (data = the raw bytes; framed as zstd store on the GPU)
    BlobHash hash;
    BlobKind kind;
    std::vector<uint8_t> data;
};

// Manager::write_packfiles over a queue of unique blobs: nonces[i] and the packfile ids are the
// caller's random draws (the reference's getrandom, pack.rs:74-76, :207-208); ids must hold at
// least as many entries as packfiles result (packfile_count()).  Returns (id, bytes) per packfile.
inline size_t packfile_count(const std::vector<Blob>& blobs) {
    std::vector<uint64_t> lens;
    for (const Blob& b : blobs) lens.push_back(b.data.size());
    uint64_t n = 0, total = 0;
    const int rc = bw_pack_plan(lens.data(), lens.size(), BW_PACK_ZSTD_STORE, nullptr, 0, &n, &total);
    if (rc != BW_ENOSPC && rc != BW_OK) check(rc);
    return n;
}

inline std::vector<std::pair<PackfileId, std::vector<uint8_t>>> write_packfiles(
    Context& ctx, const std::array<uint8_t, 32>& prk, const std::vector<Blob>& blobs,
    const std::vector<BlobNonce>& nonces, const std::vector<PackfileId>& ids) {
    std::vector<uint64_t> lens, offs;
    std::vector<uint8_t> data, hashes, kinds, nb;
    for (size_t i = 0; i < blobs.size(); i++) {
        offs.push_back(data.size());
        lens.push_back(blobs[i].data.size());
        data.insert(data.end(), blobs[i].data.begin(), blobs[i].data.end());
        hashes.insert(hashes.end(), blobs[i].hash.begin(), blobs[i].hash.end());
        kinds.push_back((uint8_t)blobs[i].kind);
        nb.insert(nb.end(), nonces.at(i).begin(), nonces.at(i).end());
    }
    uint64_t np = 0, total = 0;
    std::vector<bw_packfile> plan(packfile_count(blobs));
    check(bw_pack_plan(lens.data(), lens.size(), BW_PACK_ZSTD_STORE, plan.data(), plan.size(), &np, &total));
    if (ids.size() < np) throw Error(BW_EINVAL, "not enough packfile ids");
    std::vector<uint8_t> idb, out(total);
    for (size_t k = 0; k < np; k++) idb.insert(idb.end(), ids[k].begin(), ids[k].end());
    check(bw_pack_build(ctx.get(), prk.data(), data.data(), offs.data(), lens.data(), lens.size(), hashes.data(),
                        kinds.data(), nb.data(), BW_PACK_ZSTD_STORE, plan.data(), np, idb.data(), out.data()),
          ctx.get());
    std::vector<std::pair<PackfileId, std::vector<uint8_t>>> res;
    for (size_t k = 0; k < np; k++)
        res.emplace_back(ids[k], std::vector<uint8_t>(out.begin() + plan[k].offset,
                                                      out.begin() + plan[k].offset + plan[k].size));
    return res;
}

// compress_encrypt_blob + write_packfiles with the reference's level-3 zstd (pack.rs:58-80,
// 115-227): the frames are made and staged on the GPU, the grouping runs over their sizes, and the
// packfiles are sealed from the staging.  ids must hold at least the resulting packfile count
// (8 per blob is always enough).  Returns (id, bytes) per packfile.
inline std::vector<std::pair<PackfileId, std::vector<uint8_t>>> write_packfiles_zstd(
    Context& ctx, const std::array<uint8_t, 32>& prk, const std::vector<Blob>& blobs,
    const std::vector<BlobNonce>& nonces, const std::vector<PackfileId>& ids) {
    std::vector<uint64_t> lens, offs, frame(blobs.size());
    std::vector<uint8_t> data, hashes, kinds, nb;
    for (size_t i = 0; i < blobs.size(); i++) {
        offs.push_back(data.size());
        lens.push_back(blobs[i].data.size());
        data.insert(data.end(), blobs[i].data.begin(), blobs[i].data.end());
        hashes.insert(hashes.end(), blobs[i].hash.begin(), blobs[i].hash.end());
        kinds.push_back((uint8_t)blobs[i].kind);
        nb.insert(nb.end(), nonces.at(i).begin(), nonces.at(i).end());
    }
    // all-empty queues (e.g. one empty file) leave `data` empty: hand the library a real pointer anyway
    static const uint8_t none[1] = {0};
    check(bw_pack_compress(ctx.get(), data.empty() ? none : data.data(), offs.data(), lens.data(), lens.size(),
                           frame.data()),
          ctx.get());
    uint64_t np = 0, total = 0;
    const int rc = bw_pack_plan(frame.data(), frame.size(), 0, nullptr, 0, &np, &total);
    if (rc != BW_ENOSPC && rc != BW_OK) check(rc);
    std::vector<bw_packfile> plan(np);
    check(bw_pack_plan(frame.data(), frame.size(), 0, plan.data(), plan.size(), &np, &total));
    if (ids.size() < np) throw Error(BW_EINVAL, "not enough packfile ids");
    std::vector<uint8_t> idb, out(total);
    for (size_t k = 0; k < np; k++) idb.insert(idb.end(), ids[k].begin(), ids[k].end());
    check(bw_pack_build_compressed_host(ctx.get(), prk.data(), hashes.data(), kinds.data(), nb.data(), plan.data(), np,
                                        idb.data(), out.data()),
          ctx.get());
    std::vector<std::pair<PackfileId, std::vector<uint8_t>>> res;
    for (size_t k = 0; k < np; k++)
        res.emplace_back(ids[k], std::vector<uint8_t>(out.begin() + plan[k].offset,
                                                      out.begin() + plan[k].offset + plan[k].size));
    return res;
}

// ------------------------------------------------------------------ the read side (unpack.rs:23-83)
// Decompressor::decompress(frame, BLOB_MAX_UNCOMPRESSED_SIZE) with include_magicbytes(false)
// (unpack.rs:65-67) for every frame, on the GPU: ok[i] false where the reference returns Err.
// A frame does not say how much it regenerates: 3 MiB of host and device room per frame, so pass
// a few hundred frames at a time.
inline std::vector<std::vector<uint8_t>> zstd_decompress(Context& ctx, const std::vector<std::vector<uint8_t>>& frames,
                                                         std::vector<bool>* ok_out = nullptr) {
    const uint64_t cap = BW_BLOB_MAX_UNCOMPRESSED_SIZE;
    std::vector<uint64_t> so, sl, dof, dc(frames.size(), cap), ol(frames.size());
    std::vector<uint8_t> src, ok(frames.size()), dst(frames.size() * cap + 1);
    for (size_t i = 0; i < frames.size(); i++) {
        so.push_back(src.size());
        sl.push_back(frames[i].size());
        dof.push_back(i * cap);
        src.insert(src.end(), frames[i].begin(), frames[i].end());
    }
    static const uint8_t none[1] = {0};
    check(bw_zstd_decompress(ctx.get(), src.empty() ? none : src.data(), so.data(), sl.data(), frames.size(), dst.data(),
                             dof.data(), dc.data(), ol.data(), ok.data()),
          ctx.get());
    std::vector<std::vector<uint8_t>> out(frames.size());
    if (ok_out) ok_out->assign(frames.size(), false);
    for (size_t i = 0; i < frames.size(); i++) {
        if (!ok[i]) continue;
        out[i].assign(dst.begin() + dof[i], dst.begin() + dof[i] + ol[i]);
        if (ok_out) (*ok_out)[i] = true;
    }
    return out;
}

struct PackfileTable {  // packfiles laid out back to back, as the bw_unpack_* calls take them
    std::vector<uint8_t> data, ids;
    std::vector<bw_packfile> tab;
};

inline PackfileTable packfile_table(const std::vector<std::pair<PackfileId, std::vector<uint8_t>>>& packfiles) {
    PackfileTable t;
    for (const auto& p : packfiles) {
        bw_packfile f{};
        f.offset = t.data.size();
        f.size = p.second.size();
        for (int k = 0; k < 8 && (size_t)k < p.second.size(); k++) f.header_len |= (uint64_t)p.second[k] << (8 * k);
        t.tab.push_back(f);
        t.data.insert(t.data.end(), p.second.begin(), p.second.end());
        t.ids.insert(t.ids.end(), p.first.begin(), p.first.end());
    }
    return t;
}

// The header half of Manager::get_blob (unpack.rs:27-48): every packfile's entries, in order.
inline std::vector<bw_unpack_entry> unpack_headers(Context& ctx, const std::array<uint8_t, 32>& prk, const PackfileTable& t) {
    uint64_t n = 0, bad = 0;
    const int rc = bw_unpack_headers(ctx.get(), prk.data(), t.data.data(), t.tab.data(), t.ids.data(), t.tab.size(), nullptr,
                                     0, &n, &bad);
    if (rc != BW_ENOSPC) check(rc, ctx.get());
    std::vector<bw_unpack_entry> out(n);
    if (n)
        check(bw_unpack_headers(ctx.get(), prk.data(), t.data.data(), t.tab.data(), t.ids.data(), t.tab.size(), out.data(), n,
                                &n, &bad),
              ctx.get());
    return out;
}

// The blob half (unpack.rs:52-73) for the chosen entries: blob i and status[i] (BW_UNPACK_*);
// verify re-hashes every blob on the GPU against its entry's hash.  3 MiB of host and device room per
// entry: pass a few hundred entries at a time.
inline std::vector<Blob> unpack_blobs(Context& ctx, const std::array<uint8_t, 32>& prk, const PackfileTable& t,
                                      const std::vector<bw_unpack_entry>& entries, bool verify,
                                      std::vector<uint8_t>* status_out = nullptr) {
    const uint64_t cap = BW_BLOB_MAX_UNCOMPRESSED_SIZE;
    std::vector<uint64_t> dof, ol(entries.size());
    std::vector<uint8_t> st(entries.size()), dst(entries.size() * cap + 1);
    for (size_t i = 0; i < entries.size(); i++) dof.push_back(i * cap);
    check(bw_unpack_blobs(ctx.get(), prk.data(), t.data.data(), t.tab.data(), t.tab.size(), entries.data(), entries.size(),
                          verify ? BW_UNPACK_VERIFY : 0, dst.data(), dof.data(), ol.data(), st.data()),
          ctx.get());
    std::vector<Blob> out(entries.size());
    for (size_t i = 0; i < entries.size(); i++) {
        std::copy(entries[i].hash, entries[i].hash + 32, out[i].hash.begin());
        out[i].kind = (BlobKind)entries[i].kind;
        if (st[i] == BW_UNPACK_OK) out[i].data.assign(dst.begin() + dof[i], dst.begin() + dof[i] + ol[i]);
    }
    if (status_out) *status_out = st;
    return out;
}

// ------------------------------------------------------------------ restore (dir_unpacker.rs:14-130)
// A session over packfiles (uploaded once) and the index items bw_index_load_files returned:
// trees() is unpack()'s walk, files() restore_file for many files, unpack() both.
struct RestoredFile {
    std::string path;  // relative, components joined with '/'
    std::vector<uint8_t> data;
    bool has_mtime = false;
    uint64_t mtime = 0;
    uint8_t status = BW_RESTORE_OK;  // the first failing child's status; data is then the partial file
    uint64_t bad_child = ~0ull;
};

struct TreeError : Error {
    bw_restore_error what;
    TreeError(int rc, const std::string& m, const bw_restore_error& e) : Error(rc, m), what(e) {}
};

class Restore {
public:
    struct Walk {
        std::vector<bw_restore_node> nodes;
        std::vector<uint8_t> names, chunks;
        std::string name(size_t i) const {
            return std::string(names.begin() + nodes[i].name_off, names.begin() + nodes[i].name_off + nodes[i].name_len);
        }
    };

    Restore(Context& ctx, const std::array<uint8_t, 32>& prk, const PackfileTable& t,
            const std::vector<bw_unpack_entry>& entries, const std::vector<uint8_t>& index_items, uint32_t slots = 0)
        : ctx_(ctx) {
        check(bw_restore_open_host(ctx.get(), prk.data(), t.data.data(), t.tab.data(), t.ids.data(), t.tab.size(),
                                   entries.data(), entries.size(), index_items.data(),
                                   index_items.size() / BW_INDEX_ENTRY_BYTES, slots, &s_),
              ctx.get());
    }
    ~Restore() { bw_restore_close(s_); }
    Restore(const Restore&) = delete;
    Restore& operator=(const Restore&) = delete;
    bw_restore* get() const { return s_; }

    // entry index and status (BW_RESTORE_*) per hash
    std::vector<uint8_t> locate(const std::vector<BlobHash>& hashes, std::vector<uint64_t>* entry_idx = nullptr) {
        std::vector<uint8_t> h, st(hashes.size());
        std::vector<uint64_t> idx(hashes.size());
        for (const auto& x : hashes) h.insert(h.end(), x.begin(), x.end());
        check(bw_restore_locate(s_, h.data(), hashes.size(), idx.data(), st.data()), ctx_.get());
        if (entry_idx) *entry_idx = idx;
        return st;
    }

    Walk trees(const BlobHash& root, bool verify = false) {
        Walk w;
        bw_restore_counts n{};
        bw_restore_error e{};
        const uint32_t flags = verify ? BW_UNPACK_VERIFY : 0;
        int rc = bw_restore_trees(s_, root.data(), flags, nullptr, 0, nullptr, 0, nullptr, 0, &n, &e);
        if (rc == BW_EFORMAT) throw TreeError(rc, "tree blob refused", e);
        if (rc != BW_ENOSPC) check(rc, ctx_.get());
        w.nodes.resize(n.n_nodes);
        w.names.resize(n.name_bytes + 1);
        w.chunks.resize(32 * (n.n_chunks + 1));
        rc = bw_restore_trees(s_, root.data(), flags, w.nodes.data(), n.n_nodes, w.names.data(), n.name_bytes + 1,
                              w.chunks.data(), n.n_chunks + 1, &n, &e);
        if (rc == BW_EFORMAT) throw TreeError(rc, "tree blob refused", e);
        check(rc, ctx_.get());
        return w;
    }

    // dir_unpacker::unpack without the file system: every File node below the root's directories,
    // in node order, through a window of `window` bytes (grown when one file needs more)
    std::vector<RestoredFile> unpack(const BlobHash& root, uint64_t window = 64ull << 20, bool verify = false) {
        const Walk w = trees(root, verify);
        std::vector<RestoredFile> out;
        if (w.nodes.empty() || w.nodes[0].kind != BW_TREE_DIR) return out;
        std::vector<std::string> path(w.nodes.size());
        std::vector<uint64_t> first{0};
        std::vector<uint8_t> rows;
        for (size_t i = 1; i < w.nodes.size(); i++) {
            const bw_restore_node& nd = w.nodes[i];
            path[i] = (nd.parent ? path[nd.parent] + "/" : std::string()) + w.name(i);
            if (nd.kind != BW_TREE_FILE) continue;
            RestoredFile f;
            f.path = path[i];
            f.has_mtime = nd.flags & BW_TREE_HAS_MTIME;
            f.mtime = nd.mtime;
            out.push_back(f);
            rows.insert(rows.end(), w.chunks.begin() + 32 * nd.child_first, w.chunks.begin() + 32 * (nd.child_first + nd.n_children));
            first.push_back(rows.size() / 32);
        }
        std::vector<uint8_t> buf(window);
        size_t done = 0;
        while (done < out.size()) {
            const uint64_t n = out.size() - done;
            std::vector<uint64_t> off(n), len(n), bad(n);
            std::vector<uint8_t> st(n);
            uint64_t got = 0;
            const int rc = bw_restore_files(s_, rows.data(), first.data() + done, n, verify ? BW_UNPACK_VERIFY : 0, buf.data(),
                                            buf.size(), off.data(), len.data(), st.data(), bad.data(), &got);
            if (rc != BW_ENOSPC) check(rc, ctx_.get());
            for (uint64_t k = 0; k < got; k++) {
                RestoredFile& f = out[done + k];
                f.data.assign(buf.begin() + off[k], buf.begin() + off[k] + len[k]);
                f.status = st[k];
                f.bad_child = bad[k];
            }
            done += got;
            if (rc == BW_ENOSPC && !got) buf.resize(std::max<uint64_t>(2 * buf.size(), len[0]));
        }
        return out;
    }

private:
    Context& ctx_;
    bw_restore* s_ = nullptr;
};

// ------------------------------------------------------------------ prune (no counterpart in the reference)
// Over an open Restore: mark() = which header entries the kept roots reach, plan() = the live entries
// of the packfiles worth rewriting and their new grouping, repack() = the new packfiles, the moved
// blobs copied sealed as they are.
class Prune {
public:
    struct Mark {
        std::vector<uint8_t> live;                  // one byte per header entry
        std::vector<bw_prune_packfile_stat> stats;  // per packfile
        bw_prune_counts counts{};
        std::vector<bw_prune_error> errors;         // in no particular order
    };
    struct Plan {
        std::vector<uint64_t> order;    // the moved entries
        std::vector<bw_packfile> plan;  // the new packfiles over them
        uint64_t total_bytes = 0;
    };

    Prune(Context& ctx, Restore& session, const PackfileTable& t, const std::vector<bw_unpack_entry>& entries)
        : ctx_(ctx), s_(session), t_(t), entries_(entries) {}

    Mark mark(const std::vector<BlobHash>& roots, bool verify = false) {
        Mark m;
        m.live.resize(entries_.size() + 1);
        m.stats.resize(t_.tab.size() + 1);
        std::vector<uint8_t> r;
        for (const auto& x : roots) r.insert(r.end(), x.begin(), x.end());
        uint64_t cap = 64;
        for (;;) {
            m.errors.resize(cap + 1);
            const int rc = bw_prune_mark(s_.get(), r.data(), roots.size(), verify ? BW_UNPACK_VERIFY : 0, m.live.data(),
                                         m.stats.data(), &m.counts, m.errors.data(), cap);
            if (rc != BW_ENOSPC) {
                check(rc, ctx_.get());
                break;
            }
            cap = m.counts.n_errors;
        }
        m.live.resize(entries_.size());
        m.stats.resize(t_.tab.size());
        m.errors.resize(m.counts.n_errors);
        return m;
    }

    // a packfile is rewritten when dead_bytes / total_bytes exceeds the threshold
    static std::vector<uint8_t> choose_rewrite(const std::vector<bw_prune_packfile_stat>& stats, double max_dead_fraction = 0.0) {
        std::vector<uint8_t> rw(stats.size());
        for (size_t p = 0; p < stats.size(); p++)
            rw[p] = stats[p].total_bytes && (double)(stats[p].total_bytes - stats[p].live_bytes) > max_dead_fraction * (double)stats[p].total_bytes;
        return rw;
    }

    Plan plan(const std::vector<uint8_t>& live, const std::vector<uint8_t>& rewrite) {
        Plan p;
        uint64_t nm = 0, nn = 0, bad = 0;
        int rc = bw_prune_plan(entries_.data(), entries_.size(), t_.tab.data(), t_.tab.size(), live.data(), rewrite.data(),
                               nullptr, 0, &nm, nullptr, 0, &nn, &p.total_bytes, &bad);
        if (rc != BW_ENOSPC) check(rc, ctx_.get());
        p.order.resize(nm + 1);
        p.plan.resize(nn + 1);
        check(bw_prune_plan(entries_.data(), entries_.size(), t_.tab.data(), t_.tab.size(), live.data(), rewrite.data(),
                            p.order.data(), nm, &nm, p.plan.data(), nn, &nn, &p.total_bytes, &bad),
              ctx_.get());
        p.order.resize(nm);
        p.plan.resize(nn);
        return p;
    }

    // (id, bytes) per new packfile; new_ids: at least one per planned packfile
    std::vector<std::pair<PackfileId, std::vector<uint8_t>>> repack(const Plan& p, const std::vector<PackfileId>& new_ids) {
        if (new_ids.size() < p.plan.size()) throw Error(BW_EINVAL, "prune: too few new packfile ids");
        std::vector<uint8_t> ids, out(p.total_bytes + 1);
        for (size_t g = 0; g < p.plan.size(); g++) ids.insert(ids.end(), new_ids[g].begin(), new_ids[g].end());
        check(bw_prune_repack(s_.get(), p.order.data(), p.order.size(), p.plan.data(), p.plan.size(), ids.data(), out.data()),
              ctx_.get());
        std::vector<std::pair<PackfileId, std::vector<uint8_t>>> res;
        for (size_t g = 0; g < p.plan.size(); g++)
            res.emplace_back(new_ids[g], std::vector<uint8_t>(out.begin() + p.plan[g].offset,
                                                              out.begin() + p.plan[g].offset + p.plan[g].size));
        return res;
    }

private:
    Context& ctx_;
    Restore& s_;
    const PackfileTable& t_;
    const std::vector<bw_unpack_entry>& entries_;
};

// ------------------------------------------------------------------ diff (no counterpart in the reference)
// Over an open Restore: trees() = what changed from root a to root b (nullptr: an empty snapshot), by
// the walk that opens only the tree blobs on changed paths.  Errors are collected and never end the call.
class Diff {
public:
    struct Result {
        std::vector<bw_diff_record> records;  // a parent before its children
        std::vector<uint8_t> names;
        std::vector<uint8_t> read;            // one byte per header entry: the tree blobs opened
        bw_diff_counts counts{};
        std::vector<bw_prune_error> errors;   // in no particular order

        std::string name(size_t i) const {
            const bw_diff_record& r = records[i];
            return std::string(names.begin() + r.name_off, names.begin() + r.name_off + r.name_len);
        }
        // the names joined through parent; the root's path is empty
        std::string path(size_t i) const {
            const bw_diff_record& r = records[i];
            if (r.parent == ~0ull) return "";
            const std::string up = path(r.parent);
            return up.empty() ? name(i) : up + "/" + name(i);
        }
    };

    Diff(Context& ctx, Restore& session, const std::vector<bw_unpack_entry>& entries)
        : ctx_(ctx), s_(session), entries_(entries) {}

    Result trees(const BlobHash* a, const BlobHash* b, bool verify = false) {
        Result d;
        d.read.resize(entries_.size() + 1);
        uint64_t rcap = 1024, ncap = 1 << 16, ecap = 64;
        for (;;) {
            d.records.resize(rcap + 1);
            d.names.resize(ncap + 1);
            d.errors.resize(ecap + 1);
            const int rc = bw_diff_trees(s_.get(), a ? a->data() : nullptr, b ? b->data() : nullptr, verify ? BW_UNPACK_VERIFY : 0,
                                         d.records.data(), rcap, d.names.data(), ncap, d.read.data(), &d.counts,
                                         d.errors.data(), ecap);
            if (rc != BW_ENOSPC) {
                check(rc, ctx_.get());
                break;
            }
            // the counts are the totals up to the level that did not fit
            if (d.counts.n_records > rcap) rcap = std::max<uint64_t>(2 * rcap, d.counts.n_records);
            if (d.counts.name_bytes > ncap) ncap = std::max<uint64_t>(2 * ncap, d.counts.name_bytes);
            if (d.counts.n_errors > ecap) ecap = d.counts.n_errors;
        }
        d.records.resize(d.counts.n_records);
        d.names.resize(d.counts.name_bytes);
        d.errors.resize(d.counts.n_errors);
        d.read.resize(entries_.size());
        return d;
    }

private:
    Context& ctx_;
    Restore& s_;
    const std::vector<bw_unpack_entry>& entries_;
};

// ------------------------------------------------------------------ parent match (no counterpart in the reference)
// Over an open Restore: match() = which nodes of a stat-only scan are the parent snapshot's as they
// stand, so that a backup need not read them.  The scan has the layout of Restore::Walk (scan_of()
// makes one from a walk); errors are collected and never end the call.
class ParentMatch {
public:
    struct Result {
        std::vector<bw_parent_result> results;  // one per scan node: BW_PARENT_* and the parent's child hash
        std::vector<uint8_t> read;              // one byte per header entry: the tree blobs opened
        bw_parent_counts counts{};
        std::vector<bw_prune_error> errors;     // in no particular order
    };

    ParentMatch(Context& ctx, Restore& session, const std::vector<bw_unpack_entry>& entries)
        : ctx_(ctx), s_(session), entries_(entries) {}

    // a listing as a scan: the File nodes name no chunks
    static Restore::Walk scan_of(Restore::Walk w) {
        for (auto& n : w.nodes)
            if (n.kind == BW_TREE_FILE) n.child_first = n.n_children = 0;
        w.chunks.clear();
        return w;
    }

    // parent_root nullptr: no parent, every node is BW_PARENT_NEW; trust_before ~0 trusts every mtime
    Result match(const BlobHash* parent_root, const std::vector<bw_restore_node>& nodes, const std::vector<uint8_t>& names,
                 uint64_t trust_before = ~0ull, bool verify = false) {
        Result m;
        m.results.resize(nodes.size() + 1);
        m.read.resize(entries_.size() + 1);
        uint64_t ecap = 64;
        for (;;) {
            m.errors.resize(ecap + 1);
            const int rc = bw_parent_match(s_.get(), parent_root ? parent_root->data() : nullptr, trust_before,
                                           verify ? BW_UNPACK_VERIFY : 0, nodes.data(), nodes.size(), names.data(), names.size(),
                                           m.results.data(), m.read.data(), &m.counts, m.errors.data(), ecap);
            if (rc != BW_ENOSPC) {
                check(rc, ctx_.get());
                break;
            }
            ecap = m.counts.n_errors;
        }
        m.results.resize(nodes.size());
        m.read.resize(entries_.size());
        m.errors.resize(m.counts.n_errors);
        return m;
    }

private:
    Context& ctx_;
    Restore& s_;
    const std::vector<bw_unpack_entry>& entries_;
};

// ------------------------------------------------------------------ impact (no counterpart in the reference)
// Over an open Restore: mark() = the taint of every entry the roots reach when the entries of `bad` are
// lost (a lost tree blob is never opened), paths() = the affected paths under each root, opening nothing
// else.  Errors are collected and never end a call.
class Impact {
public:
    struct Mark {
        std::vector<uint8_t> taint;          // one byte per header entry: BW_IMPACT_SELF | BW_IMPACT_BELOW
        std::vector<uint8_t> root_affected;  // one byte per root
        bw_impact_counts counts{};
        std::vector<bw_prune_error> errors;  // in no particular order
    };
    struct Paths {
        std::vector<bw_impact_record> records;  // a parent before its children
        std::vector<uint8_t> names;
        std::vector<bw_impact_root> per_root;
        bw_impact_paths_counts counts{};
        std::vector<bw_prune_error> errors;

        std::string name(size_t i) const {
            const bw_impact_record& r = records[i];
            return std::string(names.begin() + r.name_off, names.begin() + r.name_off + r.name_len);
        }
        // the names joined through parent; a root's path is empty, an unreadable item's name is "?"
        std::string path(size_t i) const {
            const bw_impact_record& r = records[i];
            const std::string own = (r.flags & BW_IMPACT_UNREADABLE) ? "?" : name(i);
            if (r.parent == ~0ull) return (r.flags & BW_IMPACT_UNREADABLE) ? own : "";
            const std::string up = path(r.parent);
            return up.empty() ? own : up + "/" + own;
        }
    };

    Impact(Context& ctx, Restore& session, const std::vector<bw_unpack_entry>& entries)
        : ctx_(ctx), s_(session), entries_(entries) {}

    // the what-if vector: every entry of the packfiles at these positions
    std::vector<uint8_t> lost_packfiles(const std::vector<uint32_t>& positions) const {
        std::vector<uint8_t> bad(entries_.size(), 0);
        for (size_t e = 0; e < entries_.size(); e++)
            for (uint32_t p : positions)
                if (entries_[e].packfile == p) bad[e] = 1;
        return bad;
    }

    // bad: one byte per header entry, or empty: nothing is lost
    Mark mark(const std::vector<BlobHash>& roots, const std::vector<uint8_t>& bad, bool verify = false) {
        if (!bad.empty() && bad.size() != entries_.size()) throw Error(BW_EINVAL, "impact: bad holds another number of entries");
        Mark m;
        m.taint.resize(entries_.size() + 1);
        m.root_affected.resize(roots.size() + 1);
        const std::vector<uint8_t> flat = flat_roots(roots);
        uint64_t ecap = 64;
        for (;;) {
            m.errors.resize(ecap + 1);
            const int rc = bw_impact_mark(s_.get(), flat.data(), roots.size(), bad.empty() ? nullptr : bad.data(),
                                          verify ? BW_UNPACK_VERIFY : 0, m.taint.data(), m.root_affected.data(), &m.counts,
                                          m.errors.data(), ecap);
            if (rc != BW_ENOSPC) {
                check(rc, ctx_.get());
                break;
            }
            ecap = m.counts.n_errors;
        }
        m.taint.resize(entries_.size());
        m.root_affected.resize(roots.size());
        m.errors.resize(m.counts.n_errors);
        return m;
    }

    // taint as mark() returned it; the buffers grow until the walk fits them
    Paths paths(const std::vector<BlobHash>& roots, const std::vector<uint8_t>& taint, bool verify = false) {
        if (taint.size() != entries_.size()) throw Error(BW_EINVAL, "impact: taint holds another number of entries");
        Paths d;
        const std::vector<uint8_t> flat = flat_roots(roots);
        uint64_t rcap = 1024, ncap = 1 << 16, ecap = 64;
        for (;;) {
            d.records.resize(rcap + 1);
            d.names.resize(ncap + 1);
            d.errors.resize(ecap + 1);
            d.per_root.assign(roots.size() + 1, bw_impact_root{});
            const int rc = bw_impact_paths(s_.get(), flat.data(), roots.size(), taint.data(), verify ? BW_UNPACK_VERIFY : 0,
                                           d.records.data(), rcap, d.names.data(), ncap, d.per_root.data(), &d.counts,
                                           d.errors.data(), ecap);
            if (rc != BW_ENOSPC) {
                check(rc, ctx_.get());
                break;
            }
            // the counts are the totals up to the level that did not fit
            if (d.counts.n_records > rcap) rcap = std::max<uint64_t>(2 * rcap, d.counts.n_records);
            if (d.counts.name_bytes > ncap) ncap = std::max<uint64_t>(2 * ncap, d.counts.name_bytes);
            if (d.counts.n_errors > ecap) ecap = d.counts.n_errors;
        }
        d.records.resize(d.counts.n_records);
        d.names.resize(d.counts.name_bytes);
        d.errors.resize(d.counts.n_errors);
        d.per_root.resize(roots.size());
        return d;
    }

private:
    static std::vector<uint8_t> flat_roots(const std::vector<BlobHash>& roots) {
        std::vector<uint8_t> flat(32 * roots.size() + 1);
        for (size_t i = 0; i < roots.size(); i++) std::copy(roots[i].begin(), roots[i].end(), flat.begin() + 32 * i);
        return flat;
    }

    Context& ctx_;
    Restore& s_;
    const std::vector<bw_unpack_entry>& entries_;
};

// ------------------------------------------------------------------ find (no counterpart in the reference)
// Over an open Restore: paths() = the records of every item the walk looked at under each root, the hits
// flagged, for up to BW_FIND_MAX_PATTERNS glob patterns; a directory no pattern can match below is not
// opened.  Errors are collected and never end a call.
class Find {
public:
    struct Query {
        std::vector<std::string> patterns;
        uint32_t kinds = 0;  // 1u << BW_TREE_FILE, 1u << BW_TREE_DIR; 0 = both
        uint64_t size_min = 0, size_max = ~0ull, mtime_min = 0, mtime_max = ~0ull;
    };
    struct Paths {
        std::vector<bw_find_record> records;  // a parent before its children
        std::vector<uint8_t> names;
        std::vector<uint8_t> chunks;  // 32 bytes a row: the hit files' rows with BW_FIND_CHUNKS
        std::vector<bw_find_root> per_root;
        bw_find_counts counts{};
        std::vector<bw_prune_error> errors;

        std::string name(size_t i) const {
            const bw_find_record& r = records[i];
            return std::string(names.begin() + r.name_off, names.begin() + r.name_off + r.name_len);
        }
        // the names joined through parent; a root's path is empty, an unreadable item's name is "?"
        std::string path(size_t i) const {
            const bw_find_record& r = records[i];
            const std::string own = (r.flags & BW_FIND_UNREADABLE) ? "?" : name(i);
            if (r.parent == ~0ull) return (r.flags & BW_FIND_UNREADABLE) ? own : "";
            const std::string up = path(r.parent);
            return up.empty() ? own : up + "/" + own;
        }
    };

    Find(Context& ctx, Restore& session) : ctx_(ctx), s_(session) {}

    // flags: BW_FIND_ICASE | BW_FIND_SUBTREE | BW_FIND_CHUNKS | BW_UNPACK_VERIFY; the buffers grow until the walk fits them
    Paths paths(const std::vector<BlobHash>& roots, const Query& q, uint32_t flags = 0) {
        Paths d;
        std::vector<uint8_t> flat(32 * roots.size() + 1), bytes(1);
        for (size_t i = 0; i < roots.size(); i++) std::copy(roots[i].begin(), roots[i].end(), flat.begin() + 32 * i);
        std::vector<uint64_t> off(1, 0);
        for (const std::string& p : q.patterns) {
            bytes.insert(bytes.end() - 1, p.begin(), p.end());
            off.push_back(bytes.size() - 1);
        }
        bw_find_query fq{};
        fq.patterns = bytes.data();
        fq.pattern_off = off.data();
        fq.n_patterns = (uint32_t)q.patterns.size();
        fq.kinds = q.kinds;
        fq.size_min = q.size_min;
        fq.size_max = q.size_max;
        fq.mtime_min = q.mtime_min;
        fq.mtime_max = q.mtime_max;
        uint64_t rcap = 1024, ncap = 1 << 16, ccap = 1024, ecap = 64;
        for (;;) {
            d.records.resize(rcap + 1);
            d.names.resize(ncap + 1);
            d.chunks.resize(32 * ccap + 1);
            d.errors.resize(ecap + 1);
            d.per_root.assign(roots.size() + 1, bw_find_root{});
            const int rc = bw_find_paths(s_.get(), flat.data(), roots.size(), &fq, flags, d.records.data(), rcap, d.names.data(), ncap,
                                         d.chunks.data(), ccap, d.per_root.data(), &d.counts, d.errors.data(), ecap);
            if (rc != BW_ENOSPC) {
                check(rc, ctx_.get());
                break;
            }
            // the counts are the totals up to the level that did not fit
            if (d.counts.n_records > rcap) rcap = std::max<uint64_t>(2 * rcap, d.counts.n_records);
            if (d.counts.name_bytes > ncap) ncap = std::max<uint64_t>(2 * ncap, d.counts.name_bytes);
            if (d.counts.n_chunks > ccap) ccap = std::max<uint64_t>(2 * ccap, d.counts.n_chunks);
            if (d.counts.n_errors > ecap) ecap = d.counts.n_errors;
        }
        d.records.resize(d.counts.n_records);
        d.names.resize(d.counts.name_bytes);
        d.chunks.resize(32 * d.counts.n_chunks);
        d.errors.resize(d.counts.n_errors);
        d.per_root.resize(roots.size());
        return d;
    }

private:
    Context& ctx_;
    Restore& s_;
};

// ------------------------------------------------------------------ retain (no counterpart in the reference)
// Over an open Restore: mark() = for every header entry the set of roots that reach it, from one walk over
// all roots, with what each root reaches and what it alone holds; drop() = what forgetting each of some
// sets of roots frees: the live vector and the per-packfile sums a prune mark over the kept roots would
// give, ready for bw_prune_plan.  Errors are collected and never end a call.
class Retain {
public:
    struct Mark {
        uint64_t n_roots = 0, words = 1;  // W: the u64 words of one root set
        std::vector<uint64_t> masks;      // n_entries x W, entry-major: bit r % 64 of word r / 64 = root r
        std::vector<uint8_t> damaged;     // one byte per header entry
        std::vector<bw_retain_root> per_root;
        bw_retain_counts counts{};
        std::vector<bw_prune_error> errors;  // in no particular order

        bool reaches(uint64_t root, uint64_t entry) const { return masks[entry * words + root / 64] >> (root % 64) & 1; }
        // a snapshot whose figures are exact, not lower bounds
        bool complete(uint64_t root) const { return per_root[root].status == 0 && per_root[root].n_damaged == 0; }
    };
    struct Drop {
        std::vector<uint8_t> live;                  // n_sets x n_entries
        std::vector<bw_prune_packfile_stat> stats;  // n_sets x n_packfiles
        std::vector<bw_retain_freed> freed;         // one per set
    };

    Retain(Context& ctx, Restore& session, const std::vector<bw_unpack_entry>& entries, uint64_t n_packfiles)
        : ctx_(ctx), s_(session), entries_(entries), n_pf_(n_packfiles) {}

    static uint64_t words(uint64_t n_roots) { return n_roots ? (n_roots + 63) / 64 : 1; }

    // the words of the set of these root indices
    static std::vector<uint64_t> mask_of(const std::vector<uint64_t>& indices, uint64_t n_roots) {
        std::vector<uint64_t> out(words(n_roots), 0);
        for (uint64_t r : indices) {
            if (r >= n_roots) throw Error(BW_EINVAL, "retain: a root index past the roots given");
            out[r / 64] |= 1ull << (r % 64);
        }
        return out;
    }

    Mark mark(const std::vector<BlobHash>& roots, bool verify = false) {
        Mark m;
        m.n_roots = roots.size();
        m.words = words(roots.size());
        m.masks.resize(entries_.size() * m.words + 1);
        m.damaged.resize(entries_.size() + 1);
        m.per_root.resize(roots.size() + 1);
        std::vector<uint8_t> flat(32 * roots.size() + 1);
        for (size_t i = 0; i < roots.size(); i++) std::copy(roots[i].begin(), roots[i].end(), flat.begin() + 32 * i);
        uint64_t ecap = 64;
        for (;;) {
            m.errors.resize(ecap + 1);
            const int rc = bw_retain_mark(s_.get(), flat.data(), roots.size(), verify ? BW_UNPACK_VERIFY : 0, m.masks.data(),
                                          m.damaged.data(), m.per_root.data(), &m.counts, m.errors.data(), ecap);
            if (rc != BW_ENOSPC) {
                check(rc, ctx_.get());
                break;
            }
            ecap = m.counts.n_errors;
        }
        m.masks.resize(entries_.size() * m.words);
        m.damaged.resize(entries_.size());
        m.per_root.resize(roots.size());
        m.errors.resize(m.counts.n_errors);
        return m;
    }

    // sets: one list of root indices per question
    Drop drop(const Mark& m, const std::vector<std::vector<uint64_t>>& sets) {
        Drop d;
        std::vector<uint64_t> words;
        for (const auto& set : sets) {
            const std::vector<uint64_t> w = mask_of(set, m.n_roots);
            words.insert(words.end(), w.begin(), w.end());
        }
        words.push_back(0);
        d.live.resize(sets.size() * entries_.size() + 1);
        d.stats.resize(sets.size() * n_pf_ + 1);
        d.freed.resize(sets.size() + 1);
        check(bw_retain_drop(s_.get(), m.masks.data(), m.n_roots, words.data(), sets.size(), d.live.data(), d.stats.data(),
                             d.freed.data()),
              ctx_.get());
        d.live.resize(sets.size() * entries_.size());
        d.stats.resize(sets.size() * n_pf_);
        d.freed.resize(sets.size());
        return d;
    }

private:
    Context& ctx_;
    Restore& s_;
    const std::vector<bw_unpack_entry>& entries_;
    uint64_t n_pf_;
};

// ------------------------------------------------------------------ check (no counterpart in the reference)
// Over an open Restore: structure() = headers against index items and the layout of every blob
// section, data() = every selected entry's bytes (BW_CHECK_AUTH: tags only, BW_CHECK_FULL: the unpack
// chain with verify); auth() = AES-GCM tags of sealed items in a host buffer, nothing decrypted.
class Check {
public:
    struct Structure {
        std::vector<uint8_t> entry_flags;           // BW_CHECK_E_* per header entry
        std::vector<uint8_t> item_status;           // per index item
        std::vector<bw_check_packfile_stat> stats;  // per packfile
        bw_check_counts counts{};
    };

    Check(Context& ctx, Restore& session, const PackfileTable& t, const std::vector<bw_unpack_entry>& entries, size_t n_items)
        : ctx_(ctx), s_(session), n_pf_(t.tab.size()), n_entries_(entries.size()), n_items_(n_items) {}

    Structure structure() {
        Structure r;
        r.entry_flags.resize(n_entries_ + 1);
        r.item_status.resize(n_items_ + 1);
        r.stats.resize(n_pf_ + 1);
        check(bw_check_structure(s_.get(), r.entry_flags.data(), r.item_status.data(), r.stats.data(), &r.counts), ctx_.get());
        r.entry_flags.resize(n_entries_);
        r.item_status.resize(n_items_);
        r.stats.resize(n_pf_);
        return r;
    }

    // one status per header entry; select: one byte per entry, empty = all
    std::vector<uint8_t> data(uint32_t mode, const std::vector<uint8_t>& select = {}) {
        if (!select.empty() && select.size() != n_entries_) throw Error(BW_EINVAL, "check: one select byte per entry");
        std::vector<uint8_t> st(n_entries_ + 1);
        check(bw_check_data(s_.get(), mode, select.empty() ? nullptr : select.data(), st.data()), ctx_.get());
        st.resize(n_entries_);
        return st;
    }

    // ok per item: src_len includes the tag, infos holds info_len bytes per item, nonces 12
    static std::vector<uint8_t> auth(Context& ctx, const std::array<uint8_t, 32>& prk, const std::vector<uint8_t>& src,
                                     const std::vector<uint64_t>& src_off, const std::vector<uint64_t>& src_len,
                                     const std::vector<uint8_t>& infos, uint32_t info_len, const std::vector<uint8_t>& nonces) {
        std::vector<uint8_t> ok(src_off.size() + 1);
        check(bw_auth(ctx.get(), prk.data(), src.data(), src_off.data(), src_len.data(), src_off.size(), infos.data(), info_len,
                      nonces.data(), ok.data()),
              ctx.get());
        ok.resize(src_off.size());
        return ok;
    }

private:
    Context& ctx_;
    Restore& s_;
    size_t n_pf_, n_entries_, n_items_;
};

// ------------------------------------------------------------------ rekey (no counterpart in the reference)
// A store under a new backup secret without a plaintext byte stored: store() reseals every header and
// blob of an open Restore into a buffer with the same packfile table; reseal() does it to sealed items
// in a host buffer.
class Rekey {
public:
    struct Store {
        std::vector<uint8_t> data;             // the new packfiles, at the session's offsets
        std::vector<uint8_t> entry_status;     // BW_UNPACK_OK, _ETAG or _ERANGE per header entry
        std::vector<uint8_t> packfile_status;  // the header's verdict per packfile
    };
    struct Items {
        std::vector<uint8_t> data;  // output i: src_len[i] bytes at dst_off[i]
        std::vector<uint8_t> ok;    // 1 where item i was authentic under the old PRK
    };

    static Store store(Context& ctx, Restore& session, const PackfileTable& t, size_t n_entries,
                       const std::array<uint8_t, 32>& new_prk) {
        Store r;
        uint64_t end = 0;
        for (const auto& f : t.tab) end = std::max<uint64_t>(end, f.offset + f.size);
        r.data.resize(end + 1);
        r.entry_status.resize(n_entries + 1);
        r.packfile_status.resize(t.tab.size() + 1);
        check(bw_rekey_store(session.get(), new_prk.data(), r.data.data(), r.entry_status.data(), r.packfile_status.data()),
              ctx.get());
        r.data.resize(end);
        r.entry_status.resize(n_entries);
        r.packfile_status.resize(t.tab.size());
        return r;
    }

    // src_len includes the tag; infos holds info_len bytes per item, nonces 12; new_nonces empty = kept
    static Items reseal(Context& ctx, const std::array<uint8_t, 32>& old_prk, const std::array<uint8_t, 32>& new_prk,
                        const std::vector<uint8_t>& src, const std::vector<uint64_t>& src_off,
                        const std::vector<uint64_t>& src_len, const std::vector<uint8_t>& infos, uint32_t info_len,
                        const std::vector<uint8_t>& nonces, const std::vector<uint8_t>& new_nonces,
                        const std::vector<uint64_t>& dst_off, uint64_t dst_size) {
        Items r;
        r.data.resize(dst_size + 1);
        r.ok.resize(src_off.size() + 1);
        check(bw_reseal(ctx.get(), old_prk.data(), new_prk.data(), src.data(), src_off.data(), src_len.data(), src_off.size(),
                        infos.data(), info_len, nonces.data(), new_nonces.empty() ? nullptr : new_nonces.data(), r.data.data(),
                        dst_off.data(), r.ok.data()),
              ctx.get());
        r.data.resize(dst_size);
        r.ok.resize(src_off.size());
        return r;
    }
};

// ------------------------------------------------------------------ parity (no counterpart in the reference)
// Reed-Solomon shards over a packfile table and repair from them: plan() groups the packfiles, build()
// writes every parity shard and returns every shard's BLAKE3, solve() is the host Gauss-Jordan, repair()
// rebuilds one group's missing or damaged shards; matmul() is the GF(2^8) primitive under both.
class Parity {
public:
    struct Plan {
        std::vector<bw_parity_group> groups;
        uint64_t out_bytes = 0;
    };
    struct Built {
        std::vector<uint8_t> parity;   // parity shard i of group g at groups[g].out_offset + i * shard_len
        std::vector<uint8_t> digests;  // 32 bytes per shard: per group the data shards, then the parity shards
    };
    struct Solved {
        std::vector<uint32_t> used, missing;
        std::vector<uint8_t> matrix;  // missing.size() x k
    };
    struct Repaired {
        std::vector<uint8_t> data;    // a rebuilt shard s: shard_len bytes at out_off[s]
        std::vector<uint8_t> status;  // BW_PARITY_* per shard
    };

    static Plan plan(const std::vector<uint64_t>& sizes, uint32_t k, uint32_t m) {
        Plan p;
        uint64_t n = 0;
        int rc = bw_parity_plan(sizes.data(), sizes.size(), k, m, nullptr, 0, &n, &p.out_bytes);
        if (rc != BW_ENOSPC) check(rc);
        p.groups.resize(n + 1);
        check(bw_parity_plan(sizes.data(), sizes.size(), k, m, p.groups.data(), n, &n, &p.out_bytes));
        p.groups.resize(n);
        return p;
    }

    static Built build(Context& ctx, const PackfileTable& t, const Plan& p) {
        Built b;
        size_t shards = 0;
        for (const auto& g : p.groups) shards += g.k + g.m;
        b.parity.resize(p.out_bytes + 1);
        b.digests.resize(32 * shards + 1);
        check(bw_parity_build(ctx.get(), t.data.data(), t.tab.data(), t.tab.size(), p.groups.data(), p.groups.size(),
                              b.parity.data(), p.out_bytes, b.digests.data()),
              ctx.get());
        b.parity.resize(p.out_bytes);
        b.digests.resize(32 * shards);
        return b;
    }

    // throws Error with rc BW_ETOOFEW where fewer than k shards are present
    static Solved solve(uint32_t k, uint32_t m, const std::vector<uint8_t>& present) {
        Solved s;
        s.used.resize(k + 1);
        s.missing.resize(k + m + 1);
        s.matrix.resize((size_t)(k + m) * k + 1);
        uint32_t n = 0;
        check(bw_parity_solve(k, m, present.data(), s.used.data(), s.missing.data(), &n, s.matrix.data()));
        s.used.resize(k);
        s.missing.resize(n);
        s.matrix.resize((size_t)n * k);
        return s;
    }

    // digests: (k + m) x 32 as build() returned them for the group, or empty for none
    static Repaired repair(Context& ctx, const bw_parity_group& g, const std::vector<uint8_t>& present,
                           const std::vector<uint8_t>& shards, const std::vector<uint64_t>& shard_off,
                           const std::vector<uint64_t>& shard_size, const std::vector<uint8_t>& digests,
                           const std::vector<uint64_t>& out_off, uint64_t out_size) {
        Repaired r;
        r.data.resize(out_size + 1);
        r.status.resize(g.k + g.m + 1);
        check(bw_parity_repair(ctx.get(), &g, present.data(), shards.data(), shard_off.data(), shard_size.data(),
                               digests.empty() ? nullptr : digests.data(), r.data.data(), out_off.data(), r.status.data()),
              ctx.get());
        r.data.resize(out_size);
        r.status.resize(g.k + g.m);
        return r;
    }

    // row r of the result: len bytes at dst_off[r]; matrix is dst_off.size() x src_off.size(), row-major
    static std::vector<uint8_t> matmul(Context& ctx, const std::vector<uint8_t>& matrix, const std::vector<uint8_t>& src,
                                       const std::vector<uint64_t>& src_off, const std::vector<uint64_t>& src_len,
                                       const std::vector<uint64_t>& dst_off, uint64_t len, uint64_t dst_size) {
        std::vector<uint8_t> out(dst_size + 1);
        check(bw_gf_matmul(ctx.get(), matrix.data(), (uint32_t)dst_off.size(), (uint32_t)src_off.size(), src.data(),
                           src_off.data(), src_len.data(), out.data(), dst_off.data(), len),
              ctx.get());
        out.resize(dst_size);
        return out;
    }
};

// ------------------------------------------------------------------ index files (blob_index.rs)
using IndexEntry = std::pair<BlobHash, PackfileId>;

// BlobIndex::push for every entry, then the final unconditional flush: (file_num, bytes) per file
inline std::vector<std::pair<uint32_t, std::vector<uint8_t>>> index_flush(Context& ctx,
                                                                         const std::array<uint8_t, 32>& prk,
                                                                         const std::vector<IndexEntry>& entries,
                                                                         uint32_t last_file_num) {
    std::vector<uint8_t> e;
    for (const auto& x : entries) {
        e.insert(e.end(), x.first.begin(), x.first.end());
        e.insert(e.end(), x.second.begin(), x.second.end());
    }
    uint64_t nf = 0, total = 0;
    int rc = bw_index_files_build(ctx.get(), prk.data(), e.data(), entries.size(), last_file_num, nullptr, 0, nullptr,
                                  0, &nf, &total);
    if (rc != BW_ENOSPC) check(rc, ctx.get());
    std::vector<uint8_t> out(total);
    std::vector<bw_index_file> files(nf);
    check(bw_index_files_build(ctx.get(), prk.data(), e.data(), entries.size(), last_file_num, out.data(), total,
                               files.data(), nf, &nf, &total),
          ctx.get());
    std::vector<std::pair<uint32_t, std::vector<uint8_t>>> res;
    for (const auto& f : files)
        res.emplace_back(f.file_num, std::vector<uint8_t>(out.begin() + f.offset, out.begin() + f.offset + f.size));
    return res;
}

// BlobIndex::load: decrypt + parse the files on the GPU and seed the context's index; returns
// `items` sorted by hash as the reference keeps them (blob_index.rs:197).
inline std::vector<IndexEntry> index_load(Context& ctx, const std::array<uint8_t, 32>& prk,
                                          const std::vector<std::pair<uint32_t, std::vector<uint8_t>>>& files) {
    std::vector<uint8_t> data;
    std::vector<bw_index_file> tab;
    uint64_t cap = 0;
    for (const auto& f : files) {
        tab.push_back(bw_index_file{f.first, 0, data.size(), f.second.size(), 0});
        data.insert(data.end(), f.second.begin(), f.second.end());
        cap += f.second.size() / BW_INDEX_ENTRY_BYTES + 1;
    }
    std::vector<uint8_t> rec(cap * BW_INDEX_ENTRY_BYTES);
    uint64_t n = 0, bad = 0;
    check(bw_index_load_files(ctx.get(), prk.data(), data.data(), tab.data(), tab.size(), rec.data(), cap, &n, &bad),
          ctx.get());
    std::vector<IndexEntry> items(n);
    for (uint64_t i = 0; i < n; i++) {
        std::copy(rec.begin() + i * 44, rec.begin() + i * 44 + 32, items[i].first.begin());
        std::copy(rec.begin() + i * 44 + 32, rec.begin() + i * 44 + 44, items[i].second.begin());
    }
    std::sort(items.begin(), items.end(), [](const IndexEntry& a, const IndexEntry& b) { return a.first < b.first; });
    return items;
}

// ---------------------------------------------------------------- every GPU of the node
// The drop-ins' context pool (the Rust crate's Pool, INTEGRATION.md "Every GPU of the node"): the
// reference's tasks call FastCDC::new / blake3::hash with no context, one task per file on one
// worker thread per core (client/src/main.rs:43, dir_packer.rs:166).  `per_device` contexts per
// listed device (a device may repeat), context j on devices[j % n]; the k-th calling thread gets home
// slot k and home device devices[k % n]; with_context takes the first free context from the home
// slot on; hash() sends a small message to the home device's hash service with no context held
// (bw_blake3_hash_dropin_device), and BW_EAGAIN (a message over 64 KiB, a service that could not take
// it in time) through a pooled context's launch path.
class Pool {
public:
    explicit Pool(std::vector<int> devices = {}, int per_device = 16) : devices_(std::move(devices)) {
        if (devices_.empty()) {
            int n = 0;
            check(bw_device_count(&n));
            if (n <= 0) throw Error(BW_EINVAL, "no GPU for the drop-in pool");
            for (int d = 0; d < n; d++) devices_.push_back(d);
        }
        const size_t total = (size_t)std::max(per_device, 1) * devices_.size();
        for (size_t j = 0; j < total; j++) ctx_.emplace_back(new Context(devices_[j % devices_.size()]));
        mu_ = std::vector<std::mutex>(total);
    }
    const std::vector<int>& devices() const { return devices_; }
    size_t home_slot() const {
        thread_local size_t slot = next_slot().fetch_add(1);
        return slot;
    }
    int home_device() const { return devices_[home_slot() % devices_.size()]; }
    template <class F>
    auto with_context(F&& f) -> decltype(f(std::declval<Context&>())) {
        const size_t n = ctx_.size(), start = home_slot() % n;
        for (size_t k = 0; k < n; k++) {
            const size_t j = (start + k) % n;
            std::unique_lock<std::mutex> lk(mu_[j], std::try_to_lock);
            if (lk.owns_lock()) return f(*ctx_[j]);
        }
        std::lock_guard<std::mutex> lk(mu_[start]);
        return f(*ctx_[start]);
    }
    // blake3::hash(data) for read-only memory (kept chunk digests answer first)
    BlobHash hash(const uint8_t* data, size_t len) {
        BlobHash h{};
        const int rc = bw_blake3_hash_dropin_device(home_device(), data, len, h.data());
        if (rc == BW_OK) return h;
        if (rc != BW_EAGAIN) check(rc);
        return with_context([&](Context& c) {
            const uint64_t off = 0, n = len;
            static const uint8_t empty[16] = {0};
            check(bw_blake3_hash_many(c.get(), len ? data : empty, len, &off, &n, 1, h.data()), c.get());
            return h;
        });
    }

private:
    static std::atomic<size_t>& next_slot() {
        static std::atomic<size_t> n{0};
        return n;
    }
    std::vector<int> devices_;
    std::vector<std::unique_ptr<Context>> ctx_;
    std::vector<std::mutex> mu_;
};

// ---------------------------------------------------------------- N ranks in one process
// One backup session over N ranks of THIS process (the reference packs in one process,
// client/src/backup/mod.rs:64): rank r = a context on devices[r] whose index is rank r's shard of
// the session's BlobIndex (owner = digest[0] >> (8 - log2 N)) and a communicator from
// bw_comm_init_all (RCCL, one device per rank) or bw_comm_init_local (in-process transport).
// process_files shards the batch's files rank-major (contiguous, balanced by bytes), and each rank's
// thread submits its share with BW_F_NO_DEDUP, exchanges its digests and waits for its verdicts;
// the blobs come back in canonical order with `file` = the index in the batch.
class NodeSession {
public:
    NodeSession(const std::vector<int>& devices, bool rccl, uint64_t index_hint = 1u << 16,
                const bw_params* params = nullptr)
        : comms_(devices.size(), nullptr) {
        const size_t n = devices.size();
        if (n == 0 || (n & (n - 1))) throw Error(BW_EINVAL, "NodeSession: a power-of-two number of ranks");
        check(rccl ? bw_comm_init_all(devices.data(), (int)n, BW_COMM_DEFAULT_TIMEOUT_MS, comms_.data())
                   : bw_comm_init_local(devices.data(), (int)n, comms_.data()));
        for (int d : devices) {
            ctx_.emplace_back(new Context(d));
            check(bw_index_reset(ctx_.back()->get(), index_hint), ctx_.back()->get());
        }
        if (params) p_ = *params;
        else bw_params_default(&p_);
        p_.flags |= BW_F_NO_DEDUP;
    }
    ~NodeSession() {  // the communicators first: destroying one finishes its queued exchanges, which use the contexts
        for (bw_comm* c : comms_) bw_comm_destroy(c);
        ctx_.clear();
    }
    NodeSession(const NodeSession&) = delete;
    NodeSession& operator=(const NodeSession&) = delete;

    std::vector<bw_blob> process_files(const uint8_t* data, const std::vector<uint64_t>& file_off,
                                       const std::vector<uint64_t>& file_len) {
        const size_t n = ctx_.size(), nf = file_len.size();
        double total = 0;
        for (uint64_t l : file_len) total += (double)l + 1.0;  // (+1: empty files count too)
        std::vector<size_t> cut(n + 1, 0);
        double acc = 0;
        size_t f = 0;
        for (size_t r = 1; r < n; r++) {
            while (f < nf && acc + (double)file_len[f] + 1.0 <= total * (double)r / (double)n) acc += (double)file_len[f++] + 1.0;
            cut[r] = f;
        }
        cut[n] = nf;
        std::vector<std::vector<bw_blob>> out(n);
        std::vector<std::exception_ptr> err(n);
        std::vector<std::thread> th;
        for (size_t r = 0; r < n; r++)
            th.emplace_back([&, r] {
                try {
                    const size_t lo = cut[r], hi = cut[r + 1];
                    uint64_t a = 0, b = 0;
                    if (hi > lo) {
                        a = UINT64_MAX;
                        for (size_t i = lo; i < hi; i++) {
                            a = std::min(a, file_off[i]);
                            b = std::max(b, file_off[i] + file_len[i]);
                        }
                    }
                    std::vector<uint64_t> offs(hi - lo), lens(file_len.begin() + lo, file_len.begin() + hi);
                    // every chunk but a file's last is >= min(2 * (min / 2), max) bytes, as in process_files
                    const uint32_t s0 = 2 * (p_.min_size / 2);
                    const uint64_t mc = s0 < p_.max_size ? s0 : p_.max_size;
                    uint64_t cap = 1;
                    for (size_t i = lo; i < hi; i++) {
                        offs[i - lo] = file_off[i] - a;
                        cap += file_len[i] / (mc ? mc : 1) + 2;
                    }
                    bw_ctx* c = ctx_[r]->get();
                    uint64_t t = 0, got = 0;
                    check(bw_submit_host(c, b > a ? data + a : nullptr, b - a, offs.data(), lens.data(), offs.size(), &p_, &t), c);
                    check(bw_exchange_dedup(c, comms_[r], t), c);
                    out[r].resize(cap);
                    check(bw_wait(c, t, out[r].data(), cap, &got), c);
                    out[r].resize(got);
                    for (auto& x : out[r]) x.file += lo;
                } catch (...) {
                    err[r] = std::current_exception();
                }
            });
        for (auto& t : th) t.join();
        for (auto& e : err)
            if (e) std::rethrow_exception(e);
        std::vector<bw_blob> all;
        for (auto& v : out) all.insert(all.end(), v.begin(), v.end());
        return all;
    }

private:
    std::vector<std::unique_ptr<Context>> ctx_;
    std::vector<bw_comm*> comms_;
    bw_params p_{};
};

}  // namespace backuwup
