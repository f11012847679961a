"""ctypes binding of libbackuwup_amd.so (the C ABI in include/backuwup_gpu.h).

There is no fallback: if the HIP library is missing or cannot be loaded this raises, and
every compute call runs on the GPU through the library.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BW_LIB") or os.path.join(HERE, "libbackuwup_amd.so")

BW_OK, BW_EINVAL, BW_ENOSPC, BW_EHIP, BW_ENOMEM, BW_ECOLLISION, BW_ESTATE = 0, -1, -2, -3, -4, -5, -6
BW_ECRYPTO, BW_EFORMAT, BW_ECOMM, BW_EAGAIN, BW_ETOOFEW = -7, -8, -9, -10, -11
BW_COMM_ID_BYTES = 128
BW_COMM_DEFAULT_TIMEOUT_MS = 120000
BW_ZSTD_LANES = 6  # include/backuwup_gpu.h: asynchronous zstd batches in flight per context
BW_F_NO_HASH, BW_F_NO_DEDUP, BW_F_SERIAL_RESOLVE = 1, 2, 4
BW_OPT_DEPTH, BW_OPT_SCAN_SMALL_BYTES, BW_OPT_CAND_CAP, BW_OPT_STAGE_CHUNK, BW_OPT_B3_LOADS = 1, 2, 3, 4, 5
BW_OPT_SCAN_WAVES, BW_OPT_LATENCY_STREAM, BW_OPT_ZSTD_SLOTS, BW_OPT_ZSTD_BATCH_BYTES = 6, 7, 8, 9
BW_OPT_ORDER_HASH, BW_OPT_SPLIT = 10, 11
BW_OPT_PROFILE_MASK, BW_OPT_SCAN_FIRST, BW_OPT_B3_UPPER, BW_OPT_B3_GROUP = 12, 13, 14, 15
# bw_batch_counters: index -> name, in the order of the header's BW_BC_* enum
BW_BC_NAMES = ("scan_tiles", "ovf_tiles", "cand_found", "cand_stored", "trunc", "cdc_files", "segments",
               "serial_files", "tile_bytes", "seg_bytes")
BW_BC_NONE = (1 << 64) - 1  # "trunc" when every candidate fit
BW_B3_LOADS_DEFAULT = 2 # the library's BW_OPT_B3_LOADS default (bw_capi.hip)

u8p = ctypes.POINTER(ctypes.c_uint8)
u64p = ctypes.POINTER(ctypes.c_uint64)
vp = ctypes.c_void_p


class BwChunk(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint64), ("offset", ctypes.c_uint64), ("length", ctypes.c_uint64)]


class BwBlob(ctypes.Structure):
    _fields_ = [("file", ctypes.c_uint64), ("offset", ctypes.c_uint64), ("length", ctypes.c_uint64),
                ("gear_hash", ctypes.c_uint64), ("digest", ctypes.c_uint8 * 32),
                ("is_dup", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 7)]


class BwParams(ctypes.Structure):
    _fields_ = [("min_size", ctypes.c_uint32), ("avg_size", ctypes.c_uint32),
                ("max_size", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("small_file_threshold", ctypes.c_uint64)]


class BwTree(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("size", ctypes.c_uint64),
                ("mtime", ctypes.c_uint64), ("ctime", ctypes.c_uint64), ("name", vp),
                ("name_len", ctypes.c_uint64), ("children", vp), ("n_children", ctypes.c_uint64)]


class BwTreeBlob(ctypes.Structure):
    _fields_ = [("tree", ctypes.c_uint64), ("piece", ctypes.c_uint64), ("length", ctypes.c_uint64),
                ("hash", ctypes.c_uint8 * 32), ("is_dup", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 7)]


class BwStreamShard(ctypes.Structure):
    _fields_ = [("ticket", ctypes.c_uint64), ("first_blob", ctypes.c_uint64), ("n_blobs", ctypes.c_uint64),
                ("chain_start", ctypes.c_uint64), ("rounds", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class BwPackfile(ctypes.Structure):
    _fields_ = [("first_blob", ctypes.c_uint64), ("n_blobs", ctypes.c_uint64), ("offset", ctypes.c_uint64),
                ("size", ctypes.c_uint64), ("header_len", ctypes.c_uint64)]


class BwIndexFile(ctypes.Structure):
    _fields_ = [("file_num", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("offset", ctypes.c_uint64),
                ("size", ctypes.c_uint64), ("n_entries", ctypes.c_uint64)]


BW_PACKFILE_TARGET_SIZE, BW_PACKFILE_MAX_SIZE, BW_PACKFILE_MAX_BLOBS = 3 * 1024 * 1024, 16 * 1024 * 1024, 100_000
BW_BLOB_NONCE_SIZE, BW_INDEX_MAX_FILE_ENTRIES, BW_INDEX_ENTRY_BYTES = 12, 50_000, 44
BW_BLOB_FILE_CHUNK, BW_BLOB_TREE = 0, 1
BW_PACK_ZSTD_STORE = 1

BW_UNPACK_VERIFY = 1
BW_UNPACK_OK, BW_UNPACK_ETAG, BW_UNPACK_EZSTD, BW_UNPACK_EDIGEST, BW_UNPACK_ERANGE = 0, 1, 2, 3, 4
BW_BLOB_MAX_UNCOMPRESSED_SIZE = 3 * 1024 * 1024


class BwUnpackEntry(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("packfile", ctypes.c_uint32), ("kind", ctypes.c_uint8),
                ("compression", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 2), ("length", ctypes.c_uint64),
                ("offset", ctypes.c_uint64)]


BW_RESTORE_OK, BW_RESTORE_ENOTFOUND, BW_RESTORE_EMISMATCH, BW_RESTORE_ENOPACKFILE = 0, 16, 17, 18
BW_RESTORE_ENOTTREE, BW_RESTORE_EFORMAT = 19, 20
BW_RESTORE_SKEW_SLOTS = 0x100  # test hook: the gather's unaligned-source path


class BwRestoreNode(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("size", ctypes.c_uint64),
                ("mtime", ctypes.c_uint64), ("ctime", ctypes.c_uint64), ("parent", ctypes.c_uint64),
                ("child_first", ctypes.c_uint64), ("n_children", ctypes.c_uint64), ("name_off", ctypes.c_uint64),
                ("name_len", ctypes.c_uint64)]


class BwRestoreCounts(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_uint64), ("name_bytes", ctypes.c_uint64), ("n_chunks", ctypes.c_uint64)]


class BwRestoreError(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("reason", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class BwPrunePackfileStat(ctypes.Structure):
    _fields_ = [("live_blobs", ctypes.c_uint64), ("live_bytes", ctypes.c_uint64), ("total_blobs", ctypes.c_uint64),
                ("total_bytes", ctypes.c_uint64)]


class BwPruneCounts(ctypes.Structure):
    _fields_ = [("live_blobs", ctypes.c_uint64), ("live_bytes", ctypes.c_uint64), ("total_blobs", ctypes.c_uint64),
                ("total_bytes", ctypes.c_uint64), ("n_trees_expanded", ctypes.c_uint64), ("n_levels", ctypes.c_uint64),
                ("n_errors", ctypes.c_uint64)]


class BwPruneError(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("parent", ctypes.c_uint8 * 32), ("child_pos", ctypes.c_uint64),
                ("reason", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


BW_DIFF_ADDED, BW_DIFF_REMOVED, BW_DIFF_MODIFIED, BW_DIFF_TYPE_CHANGED = 1, 2, 3, 4
BW_DIFF_UNREADABLE, BW_DIFF_TRUNCATED = 1, 2


class BwDiffSide(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("kind", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("size", ctypes.c_uint64), ("mtime", ctypes.c_uint64), ("ctime", ctypes.c_uint64),
                ("n_children", ctypes.c_uint64)]


class BwDiffRecord(ctypes.Structure):
    _fields_ = [("change", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("parent", ctypes.c_uint64),
                ("name_off", ctypes.c_uint64), ("name_len", ctypes.c_uint64), ("a", BwDiffSide), ("b", BwDiffSide),
                ("common_prefix", ctypes.c_uint64), ("common_suffix", ctypes.c_uint64), ("n_new", ctypes.c_uint64)]


class BwDiffCounts(ctypes.Structure):
    _fields_ = [("n_records", ctypes.c_uint64), ("name_bytes", ctypes.c_uint64), ("n_read", ctypes.c_uint64),
                ("n_levels", ctypes.c_uint64), ("n_errors", ctypes.c_uint64)]


BW_PARENT_NEW, BW_PARENT_UNCHANGED, BW_PARENT_CHANGED, BW_PARENT_RACY, BW_PARENT_DIR, BW_PARENT_TYPE_CHANGED = range(6)


class BwParentResult(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("status", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class BwParentCounts(ctypes.Structure):
    _fields_ = [("n_read", ctypes.c_uint64), ("n_levels", ctypes.c_uint64), ("n_errors", ctypes.c_uint64),
                ("n_unchanged", ctypes.c_uint64), ("unchanged_bytes", ctypes.c_uint64)]


BW_IMPACT_SELF, BW_IMPACT_BELOW = 1, 2
BW_IMPACT_UNREADABLE, BW_IMPACT_TRUNCATED, BW_IMPACT_CYCLIC = 1, 2, 4


class BwImpactCounts(ctypes.Structure):
    _fields_ = [("n_trees_expanded", ctypes.c_uint64), ("n_levels", ctypes.c_uint64), ("n_edges", ctypes.c_uint64),
                ("n_sweeps", ctypes.c_uint64), ("n_tainted", ctypes.c_uint64), ("n_errors", ctypes.c_uint64),
                ("n_roots_affected", ctypes.c_uint64)]


class BwImpactRecord(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("root", ctypes.c_uint64), ("parent", ctypes.c_uint64),
                ("name_off", ctypes.c_uint64), ("name_len", ctypes.c_uint64), ("kind", ctypes.c_uint32),
                ("meta_flags", ctypes.c_uint32), ("size", ctypes.c_uint64), ("mtime", ctypes.c_uint64),
                ("ctime", ctypes.c_uint64), ("n_children", ctypes.c_uint64), ("n_affected", ctypes.c_uint64),
                ("first_affected", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class BwImpactRoot(ctypes.Structure):
    _fields_ = [("n_records", ctypes.c_uint64), ("n_files", ctypes.c_uint64), ("n_unreadable", ctypes.c_uint64),
                ("lost_chunk_refs", ctypes.c_uint64)]


class BwImpactPathsCounts(ctypes.Structure):
    _fields_ = [("n_records", ctypes.c_uint64), ("name_bytes", ctypes.c_uint64), ("n_levels", ctypes.c_uint64),
                ("n_errors", ctypes.c_uint64)]


BW_RETAIN_MAX_ROOTS = 4096


class BwRetainRoot(ctypes.Structure):
    _fields_ = [("reached_blobs", ctypes.c_uint64), ("reached_bytes", ctypes.c_uint64), ("unique_blobs", ctypes.c_uint64),
                ("unique_bytes", ctypes.c_uint64), ("n_damaged", ctypes.c_uint64), ("status", ctypes.c_uint32),
                ("pad", ctypes.c_uint32)]


class BwRetainCounts(ctypes.Structure):
    _fields_ = [("n_trees_expanded", ctypes.c_uint64), ("n_levels", ctypes.c_uint64), ("n_edges", ctypes.c_uint64),
                ("n_sweeps", ctypes.c_uint64), ("n_errors", ctypes.c_uint64), ("reached_blobs", ctypes.c_uint64),
                ("reached_bytes", ctypes.c_uint64), ("orphan_blobs", ctypes.c_uint64), ("orphan_bytes", ctypes.c_uint64)]


class BwRetainFreed(ctypes.Structure):
    _fields_ = [("freed_blobs", ctypes.c_uint64), ("freed_bytes", ctypes.c_uint64), ("live_blobs", ctypes.c_uint64),
                ("live_bytes", ctypes.c_uint64)]


BW_FIND_MAX_PATTERNS = 32
BW_FIND_ICASE, BW_FIND_SUBTREE, BW_FIND_CHUNKS = 2, 4, 8
BW_FIND_HIT, BW_FIND_UNREADABLE, BW_FIND_TRUNCATED, BW_FIND_CYCLIC, BW_FIND_PRUNED = 1, 2, 4, 8, 16


class BwFindQuery(ctypes.Structure):
    _fields_ = [("patterns", ctypes.c_void_p), ("pattern_off", ctypes.c_void_p), ("n_patterns", ctypes.c_uint32),
                ("kinds", ctypes.c_uint32), ("size_min", ctypes.c_uint64), ("size_max", ctypes.c_uint64),
                ("mtime_min", ctypes.c_uint64), ("mtime_max", ctypes.c_uint64)]


class BwFindRecord(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("root", ctypes.c_uint64), ("parent", ctypes.c_uint64),
                ("name_off", ctypes.c_uint64), ("name_len", ctypes.c_uint64), ("kind", ctypes.c_uint32),
                ("meta_flags", ctypes.c_uint32), ("size", ctypes.c_uint64), ("mtime", ctypes.c_uint64),
                ("ctime", ctypes.c_uint64), ("child_first", ctypes.c_uint64), ("n_children", ctypes.c_uint64),
                ("patterns", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class BwFindRoot(ctypes.Structure):
    _fields_ = [("n_records", ctypes.c_uint64), ("n_hits", ctypes.c_uint64), ("n_hit_files", ctypes.c_uint64),
                ("hit_bytes", ctypes.c_uint64), ("n_unreadable", ctypes.c_uint64)]


class BwFindCounts(ctypes.Structure):
    _fields_ = [("n_records", ctypes.c_uint64), ("name_bytes", ctypes.c_uint64), ("n_chunks", ctypes.c_uint64),
                ("n_levels", ctypes.c_uint64), ("n_opened", ctypes.c_uint64), ("n_pruned", ctypes.c_uint64),
                ("n_errors", ctypes.c_uint64)]


BW_CHECK_E_RANGE, BW_CHECK_E_ORDER, BW_CHECK_E_UNINDEXED, BW_CHECK_E_SHADOWED = 1, 2, 4, 8
BW_CHECK_SKIPPED, BW_CHECK_IDUPLICATE = 32, 33
BW_CHECK_AUTH, BW_CHECK_FULL = 1, 2


class BwCheckPackfileStat(ctypes.Structure):
    _fields_ = [("n_entries", ctypes.c_uint64), ("n_range", ctypes.c_uint64), ("n_order", ctypes.c_uint64),
                ("n_unindexed", ctypes.c_uint64), ("n_shadowed", ctypes.c_uint64), ("claimed_bytes", ctypes.c_uint64),
                ("section_bytes", ctypes.c_uint64), ("tail", ctypes.c_int64)]


class BwCheckCounts(ctypes.Structure):
    _fields_ = [("n_entries", ctypes.c_uint64), ("n_range", ctypes.c_uint64), ("n_order", ctypes.c_uint64),
                ("n_unindexed", ctypes.c_uint64), ("n_shadowed", ctypes.c_uint64), ("claimed_bytes", ctypes.c_uint64),
                ("section_bytes", ctypes.c_uint64), ("n_items_ok", ctypes.c_uint64), ("n_items_nopackfile", ctypes.c_uint64),
                ("n_items_mismatch", ctypes.c_uint64), ("n_items_duplicate", ctypes.c_uint64),
                ("n_packfiles_clean", ctypes.c_uint64)]


class BwParityGroup(ctypes.Structure):
    _fields_ = [("first_packfile", ctypes.c_uint64), ("k", ctypes.c_uint32), ("m", ctypes.c_uint32),
                ("shard_len", ctypes.c_uint64), ("out_offset", ctypes.c_uint64)]


BW_PARITY_OK, BW_PARITY_DAMAGED, BW_PARITY_REBUILT, BW_PARITY_REBUILT_BAD, BW_PARITY_LOST = 0, 1, 2, 3, 4
# bw_internal.h: k_gf_matmul's row tile, bytes per wave task, and bytes per destination row of one grid pass
GF_ROW_TILE, GF_WAVE_BYTES, GF_GRID_BYTES = 8, 2048, 1024 * 4 * 2048

BW_TREE_FILE, BW_TREE_DIR = 0, 1
BW_TREE_HAS_SIZE, BW_TREE_HAS_MTIME, BW_TREE_HAS_CTIME = 1, 2, 4
BW_TREE_BLOB_MAX_CHILDREN = 10000

# (name, restype, argtypes) for every symbol of include/backuwup_gpu.h
SIGNATURES = [
    ("bw_params_default", None, [ctypes.POINTER(BwParams)]),
    ("bw_strerror", ctypes.c_char_p, [ctypes.c_int]),
    ("bw_create", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(vp)]),
    ("bw_destroy", None, [vp]),
    ("bw_last_error", ctypes.c_char_p, [vp]),
    ("bw_set_stream", ctypes.c_int, [vp, vp]),
    ("bw_get_stream", vp, [vp]),
    ("bw_fastcdc_chunks", ctypes.c_int, [vp, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.c_uint32, ctypes.POINTER(BwChunk), ctypes.c_uint64, u64p]),
    ("bw_blake3_hash", ctypes.c_int, [vp, vp, ctypes.c_uint64, u8p]),
    ("bw_blake3_hash_many", ctypes.c_int, [vp, vp, ctypes.c_uint64, u64p, u64p, ctypes.c_uint64, u8p]),
    ("bw_index_reset", ctypes.c_int, [vp, ctypes.c_uint64]),
    ("bw_index_seed", ctypes.c_int, [vp, vp, ctypes.c_uint64]),
    ("bw_index_check_insert", ctypes.c_int, [vp, vp, ctypes.c_uint64, u8p]),
    ("bw_index_size", ctypes.c_int, [vp, u64p]),
    ("bw_index_check", ctypes.c_int, [vp]),
    ("bw_index_create", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(vp)]),
    ("bw_index_destroy", None, [vp]),
    ("bw_attach_index", ctypes.c_int, [vp, vp]),
    ("bw_set_option", ctypes.c_int, [vp, ctypes.c_int, ctypes.c_uint64]),
    ("bw_submit_device", ctypes.c_int, [vp, vp, ctypes.c_uint64, u64p, u64p, ctypes.c_uint64,
                                        ctypes.POINTER(BwParams), u64p]),
    ("bw_submit_host", ctypes.c_int, [vp, vp, ctypes.c_uint64, u64p, u64p, ctypes.c_uint64,
                                      ctypes.POINTER(BwParams), u64p]),
    ("bw_wait", ctypes.c_int, [vp, ctypes.c_uint64, ctypes.POINTER(BwBlob), ctypes.c_uint64, u64p]),
    ("bw_host_register", ctypes.c_int, [vp, ctypes.c_uint64]),
    ("bw_host_unregister", ctypes.c_int, [vp]),
    ("bw_process_files", ctypes.c_int, [vp, vp, ctypes.c_uint64, u64p, u64p, ctypes.c_uint64,
                                        ctypes.POINTER(BwParams), ctypes.POINTER(BwBlob), ctypes.c_uint64,
                                        u64p]),
    ("bw_process_files_device", ctypes.c_int, [vp, vp, ctypes.c_uint64, u64p, u64p, ctypes.c_uint64,
                                               ctypes.POINTER(BwParams)]),
    ("bw_results", ctypes.c_int, [vp, ctypes.POINTER(BwBlob), ctypes.c_uint64, u64p]),
    ("bw_batch_device_views", ctypes.c_int, [vp, u64p, ctypes.POINTER(vp), ctypes.POINTER(vp)]),
    ("bw_partition_by_owner", ctypes.c_int, [vp, vp, ctypes.c_uint64, ctypes.c_uint32, vp, vp, u64p]),
    ("bw_index_check_insert_device", ctypes.c_int, [vp, vp, ctypes.c_uint64, vp]),
    ("bw_scatter_verdicts", ctypes.c_int, [vp, vp, vp, ctypes.c_uint64, vp]),
    ("bw_batch_views", ctypes.c_int, [vp, ctypes.c_uint64, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                      ctypes.POINTER(vp), u64p]),
    ("bw_batch_counters", ctypes.c_int, [vp, ctypes.c_uint64, u64p, ctypes.c_uint32,
                                         ctypes.POINTER(ctypes.c_uint32)]),
    ("bw_partition_buckets", ctypes.c_int, [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, vp, vp,
                                            vp]),
    ("bw_index_check_insert_buckets", ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, vp]),
    ("bw_scatter_buckets", ctypes.c_int, [vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, vp]),
    ("bw_comm_unique_id", ctypes.c_int, [u8p]),
    ("bw_comm_init", ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, u8p, ctypes.POINTER(vp)]),
    ("bw_comm_init_timeout", ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, u8p, ctypes.c_uint32,
                                            ctypes.POINTER(vp)]),
    ("bw_comm_set_timeout", ctypes.c_int, [vp, ctypes.c_uint32]),
    ("bw_comm_status", ctypes.c_int, [vp]),
    ("bw_comm_init_host", ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.POINTER(vp)]),
    ("bw_comm_init_all", ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(vp)]),
    ("bw_comm_init_local", ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(vp)]),
    ("bw_comm_destroy", None, [vp]),
    ("bw_comm_last_error", ctypes.c_char_p, [vp]),
    ("bw_comm_set_capacity", ctypes.c_int, [vp, ctypes.c_uint64]),
    ("bw_exchange_dedup", ctypes.c_int, [vp, vp, ctypes.c_uint64]),
    ("bw_comm_progress", ctypes.c_int, [vp]),
    ("bw_stream_window", ctypes.c_int, [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, u64p, u64p]),
    ("bw_chunk_stream_shard", ctypes.c_int, [vp, vp, vp, ctypes.c_uint64, ctypes.POINTER(BwParams),
                                             ctypes.POINTER(BwStreamShard)]),
    ("bw_tree_serialize", ctypes.c_int, [ctypes.POINTER(BwTree), vp, vp, ctypes.c_uint64, u64p]),
    ("bw_tree_blobs", ctypes.c_int, [vp, ctypes.POINTER(BwTree), ctypes.c_uint64, ctypes.c_uint32, vp,
                                     ctypes.POINTER(BwTreeBlob), ctypes.c_uint64, u64p]),
    ("bw_seal_device", ctypes.c_int, [vp, vp, vp, u64p, u64p, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp,
                                      u64p]),
    ("bw_open_device", ctypes.c_int, [vp, vp, vp, u64p, u64p, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp,
                                      u64p, u8p]),
    ("bw_seal", ctypes.c_int, [vp, vp, vp, u64p, u64p, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, u64p]),
    ("bw_open", ctypes.c_int, [vp, vp, vp, u64p, u64p, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, u64p, u8p]),
    ("bw_zstd_store_size", ctypes.c_uint64, [ctypes.c_uint64]),
    ("bw_zstd_compress_device", ctypes.c_int, [vp, vp, u64p, u64p, ctypes.c_uint64, vp, u64p, u64p]),
    ("bw_zstd_compress", ctypes.c_int, [vp, vp, u64p, u64p, ctypes.c_uint64, vp, u64p, u64p]),
    ("bw_zstd_submit_device", ctypes.c_int, [vp, vp, u64p, u64p, ctypes.c_uint64, vp, u64p, u64p]),
    ("bw_zstd_wait", ctypes.c_int, [vp, ctypes.c_uint64, u64p]),
    ("bw_pack_plan", ctypes.c_int, [u64p, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(BwPackfile),
                                    ctypes.c_uint64, u64p, u64p]),
    ("bw_pack_plan_session", ctypes.c_int, [vp, vp, u64p, ctypes.c_uint64, ctypes.c_uint32,
                                            ctypes.POINTER(BwPackfile), ctypes.c_uint64, u64p, u64p, u64p]),
    ("bw_pack_build_device", ctypes.c_int, [vp, vp, vp, u64p, u64p, ctypes.c_uint64, vp, vp, vp, ctypes.c_uint32,
                                            ctypes.POINTER(BwPackfile), ctypes.c_uint64, vp, vp]),
    ("bw_pack_build", ctypes.c_int, [vp, vp, vp, u64p, u64p, ctypes.c_uint64, vp, vp, vp, ctypes.c_uint32,
                                     ctypes.POINTER(BwPackfile), ctypes.c_uint64, vp, vp]),
    ("bw_pack_compress_device", ctypes.c_int, [vp, vp, u64p, u64p, ctypes.c_uint64, u64p]),
    ("bw_pack_build_compressed", ctypes.c_int, [vp, vp, vp, vp, vp, ctypes.POINTER(BwPackfile), ctypes.c_uint64,
                                                vp, vp]),
    ("bw_pack_compress", ctypes.c_int, [vp, vp, u64p, u64p, ctypes.c_uint64, u64p]),
    ("bw_pack_build_compressed_host", ctypes.c_int, [vp, vp, vp, vp, vp, ctypes.POINTER(BwPackfile),
                                                     ctypes.c_uint64, vp, vp]),
    ("bw_index_files_build", ctypes.c_int, [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint32, vp, ctypes.c_uint64,
                                            ctypes.POINTER(BwIndexFile), ctypes.c_uint64, u64p, u64p]),
    ("bw_index_load_files", ctypes.c_int, [vp, vp, vp, ctypes.POINTER(BwIndexFile), ctypes.c_uint64, vp,
                                           ctypes.c_uint64, u64p, u64p]),
    ("bw_zstd_decompress_device", ctypes.c_int, [vp, vp, u64p, u64p, ctypes.c_uint64, vp, u64p, u64p, u64p, u8p]),
    ("bw_zstd_decompress", ctypes.c_int, [vp, vp, u64p, u64p, ctypes.c_uint64, vp, u64p, u64p, u64p, u8p]),
    ("bw_unpack_headers", ctypes.c_int, [vp, vp, vp, ctypes.POINTER(BwPackfile), vp, ctypes.c_uint64,
                                         ctypes.POINTER(BwUnpackEntry), ctypes.c_uint64, u64p, u64p]),
    ("bw_unpack_blobs_device", ctypes.c_int, [vp, vp, vp, ctypes.POINTER(BwPackfile), ctypes.c_uint64,
                                              ctypes.POINTER(BwUnpackEntry), ctypes.c_uint64, ctypes.c_uint32, vp, u64p,
                                              u64p, u8p]),
    ("bw_unpack_blobs", ctypes.c_int, [vp, vp, vp, ctypes.POINTER(BwPackfile), ctypes.c_uint64,
                                       ctypes.POINTER(BwUnpackEntry), ctypes.c_uint64, ctypes.c_uint32, vp, u64p, u64p,
                                       u8p]),
    ("bw_restore_open", ctypes.c_int, [vp, vp, vp, ctypes.POINTER(BwPackfile), vp, ctypes.c_uint64,
                                       ctypes.POINTER(BwUnpackEntry), ctypes.c_uint64, vp, ctypes.c_uint64,
                                       ctypes.c_uint32, ctypes.POINTER(vp)]),
    ("bw_restore_open_host", ctypes.c_int, [vp, vp, vp, ctypes.POINTER(BwPackfile), vp, ctypes.c_uint64,
                                            ctypes.POINTER(BwUnpackEntry), ctypes.c_uint64, vp, ctypes.c_uint64,
                                            ctypes.c_uint32, ctypes.POINTER(vp)]),
    ("bw_restore_close", ctypes.c_int, [vp]),
    ("bw_restore_locate", ctypes.c_int, [vp, vp, ctypes.c_uint64, u64p, u8p]),
    ("bw_restore_trees", ctypes.c_int, [vp, vp, ctypes.c_uint32, ctypes.POINTER(BwRestoreNode), ctypes.c_uint64, vp,
                                        ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.POINTER(BwRestoreCounts),
                                        ctypes.POINTER(BwRestoreError)]),
    ("bw_restore_files_device", ctypes.c_int, [vp, vp, u64p, ctypes.c_uint64, ctypes.c_uint32, vp, ctypes.c_uint64,
                                               u64p, u64p, u8p, u64p, u64p]),
    ("bw_restore_files", ctypes.c_int, [vp, vp, u64p, ctypes.c_uint64, ctypes.c_uint32, vp, ctypes.c_uint64,
                                        u64p, u64p, u8p, u64p, u64p]),
    ("bw_prune_mark", ctypes.c_int, [vp, vp, ctypes.c_uint64, ctypes.c_uint32, u8p, ctypes.POINTER(BwPrunePackfileStat),
                                     ctypes.POINTER(BwPruneCounts), ctypes.POINTER(BwPruneError), ctypes.c_uint64]),
    ("bw_prune_plan", ctypes.c_int, [ctypes.POINTER(BwUnpackEntry), ctypes.c_uint64, ctypes.POINTER(BwPackfile),
                                     ctypes.c_uint64, u8p, u8p, u64p, ctypes.c_uint64, u64p, ctypes.POINTER(BwPackfile),
                                     ctypes.c_uint64, u64p, u64p, u64p]),
    ("bw_prune_repack_device", ctypes.c_int, [vp, u64p, ctypes.c_uint64, ctypes.POINTER(BwPackfile), ctypes.c_uint64, vp,
                                              vp]),
    ("bw_prune_repack", ctypes.c_int, [vp, u64p, ctypes.c_uint64, ctypes.POINTER(BwPackfile), ctypes.c_uint64, vp, vp]),
    ("bw_diff_trees", ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.POINTER(BwDiffRecord), ctypes.c_uint64, vp,
                                     ctypes.c_uint64, u8p, ctypes.POINTER(BwDiffCounts), ctypes.POINTER(BwPruneError),
                                     ctypes.c_uint64]),
    ("bw_parent_match", ctypes.c_int, [vp, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(BwRestoreNode), ctypes.c_uint64,
                                       vp, ctypes.c_uint64, ctypes.POINTER(BwParentResult), u8p,
                                       ctypes.POINTER(BwParentCounts), ctypes.POINTER(BwPruneError), ctypes.c_uint64]),
    ("bw_impact_mark", ctypes.c_int, [vp, vp, ctypes.c_uint64, u8p, ctypes.c_uint32, u8p, u8p, ctypes.POINTER(BwImpactCounts),
                                      ctypes.POINTER(BwPruneError), ctypes.c_uint64]),
    ("bw_impact_paths", ctypes.c_int, [vp, vp, ctypes.c_uint64, u8p, ctypes.c_uint32, ctypes.POINTER(BwImpactRecord),
                                       ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.POINTER(BwImpactRoot),
                                       ctypes.POINTER(BwImpactPathsCounts), ctypes.POINTER(BwPruneError), ctypes.c_uint64]),
    ("bw_retain_mark", ctypes.c_int, [vp, vp, ctypes.c_uint64, ctypes.c_uint32, u64p, u8p, ctypes.POINTER(BwRetainRoot),
                                      ctypes.POINTER(BwRetainCounts), ctypes.POINTER(BwPruneError), ctypes.c_uint64]),
    ("bw_retain_drop", ctypes.c_int, [vp, u64p, ctypes.c_uint64, u64p, ctypes.c_uint64, u8p,
                                      ctypes.POINTER(BwPrunePackfileStat), ctypes.POINTER(BwRetainFreed)]),
    ("bw_find_paths", ctypes.c_int, [vp, vp, ctypes.c_uint64, ctypes.POINTER(BwFindQuery), ctypes.c_uint32,
                                     ctypes.POINTER(BwFindRecord), ctypes.c_uint64, vp, ctypes.c_uint64, vp, ctypes.c_uint64,
                                     ctypes.POINTER(BwFindRoot), ctypes.POINTER(BwFindCounts), ctypes.POINTER(BwPruneError),
                                     ctypes.c_uint64]),
    ("bw_auth_device", ctypes.c_int, [vp, vp, vp, u64p, u64p, ctypes.c_uint64, vp, ctypes.c_uint32, vp, u8p]),
    ("bw_auth", ctypes.c_int, [vp, vp, vp, u64p, u64p, ctypes.c_uint64, vp, ctypes.c_uint32, vp, u8p]),
    ("bw_check_structure", ctypes.c_int, [vp, u8p, u8p, ctypes.POINTER(BwCheckPackfileStat),
                                          ctypes.POINTER(BwCheckCounts)]),
    ("bw_check_data", ctypes.c_int, [vp, ctypes.c_uint32, u8p, u8p]),
    ("bw_reseal_device", ctypes.c_int, [vp, vp, vp, vp, u64p, u64p, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, vp, u64p,
                                        u8p]),
    ("bw_reseal", ctypes.c_int, [vp, vp, vp, vp, u64p, u64p, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, vp, u64p, u8p]),
    ("bw_rekey_store_device", ctypes.c_int, [vp, vp, vp, u8p, u8p]),
    ("bw_rekey_store", ctypes.c_int, [vp, vp, vp, u8p, u8p]),
    ("bw_gf_matmul_device", ctypes.c_int, [vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, u64p, u64p, vp, u64p,
                                           ctypes.c_uint64]),
    ("bw_gf_matmul", ctypes.c_int, [vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, u64p, u64p, vp, u64p, ctypes.c_uint64]),
    ("bw_parity_plan", ctypes.c_int, [u64p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.POINTER(BwParityGroup), ctypes.c_uint64, u64p, u64p]),
    ("bw_parity_build_device", ctypes.c_int, [vp, vp, ctypes.POINTER(BwPackfile), ctypes.c_uint64,
                                              ctypes.POINTER(BwParityGroup), ctypes.c_uint64, vp, ctypes.c_uint64, u8p]),
    ("bw_parity_build", ctypes.c_int, [vp, vp, ctypes.POINTER(BwPackfile), ctypes.c_uint64,
                                       ctypes.POINTER(BwParityGroup), ctypes.c_uint64, vp, ctypes.c_uint64, u8p]),
    ("bw_parity_solve", ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, u8p, ctypes.POINTER(ctypes.c_uint32),
                                       ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), u8p]),
    ("bw_parity_repair_device", ctypes.c_int, [vp, ctypes.POINTER(BwParityGroup), u8p, vp, u64p, u64p, u8p, vp, u64p,
                                               u8p]),
    ("bw_parity_repair", ctypes.c_int, [vp, ctypes.POINTER(BwParityGroup), u8p, vp, u64p, u64p, u8p, vp, u64p, u8p]),
    ("bw_profile_enable", ctypes.c_int, [vp, ctypes.c_int]),
    ("bw_fastcdc_chunks_hashed", ctypes.c_int, [vp, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                                ctypes.c_uint32, vp, ctypes.c_uint64, u64p, u64p]),
    ("bw_fastcdc_release", None, [ctypes.c_uint64]),
    ("bw_blake3_kept_hits", ctypes.c_uint64, []),
    ("bw_blake3_hash_dropin", ctypes.c_int, [vp, vp, ctypes.c_uint64, u8p]),
    ("bw_blake3_hash_dropin_device", ctypes.c_int, [ctypes.c_int, vp, ctypes.c_uint64, u8p]),
    ("bw_blake3_coalesce_stats", ctypes.c_int, [ctypes.c_int, u64p, u64p]),
    ("bw_blake3_service_faults", ctypes.c_int, [ctypes.c_int, u64p, u64p, u64p]),
    ("bw_device_count", ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    ("bw_profile_read", ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double), u64p]),
    ("bw_profile_intervals", ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_uint64, u64p]),
    ("bw_calibrate_b3", ctypes.c_int, [vp, ctypes.c_double, ctypes.POINTER(ctypes.c_double)]),
]

STAGES = ["scan", "compact", "resolve", "assemble", "b3_leaf", "b3_tree", "dedup", "pack"]
# the kernel each stage's events bracket (names as rocprofv3 reports them)
STAGE_KERNELS = {"scan": "k_scan", "b3_leaf": "k_b3_lines", "b3_tree": "k_b3_upper"}

_lib = None


def load():
    """Load the HIP library; raises OSError/RuntimeError when it is absent (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libbackuwup_amd.so not built (run __graft_entry__.build() or "
                           "python backuwup_amd/build.py); there is no CPU fallback")
    # torch ships its own libamdhip64; load it first so the process holds one HIP runtime (our
    # library binds to the already-loaded soname).  Loaded the other way round, both runtimes end
    # up mapped and bw_create fails with a HIP error on the GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class BwError(RuntimeError):
    def __init__(self, rc, msg=""):
        self.rc = rc
        text = load().bw_strerror(rc).decode()
        super().__init__("backuwup_amd error %d (%s)%s" % (rc, text, (": " + msg) if msg else ""))


def check(rc, ctx=None):
    if rc != BW_OK:
        msg = ""
        if ctx is not None:
            m = load().bw_last_error(ctx)
            msg = m.decode() if m else ""
        raise BwError(rc, msg)
