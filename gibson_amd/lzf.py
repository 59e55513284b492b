"""ctypes mirror of liblzf_hip.so (include/lzf.h, include/lzf_gpu.h).

Names, argument meaning and error behaviour follow the reference API:
``lzf_compress(in, out_len)`` returns the stream or ``None`` (the C call's 0,
src/lzf_c.c:131/176/263/276); ``lzf_decompress(in, out_len)`` returns
``(bytes, 0)`` or ``(None, errno)`` with errno E2BIG / EINVAL in the order of
src/lzf_d.c:72-131.  There is no Python or CPU codec behind these names: a
missing or unloadable library raises ``LzfLibraryMissing``.
"""
import contextlib
import ctypes
import os

LZF_VERSION = 0x0105  # src/lzf.h:49

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

LZF_GPU_OK = 0
_ERRS = {-1: "EARG", -2: "ELAUNCH", -3: "ENODEV", -4: "ENOMEM"}

EXPORTS = (
    "lzf_compress",
    "lzf_decompress",
    "lzf_gpu_compress_batch",
    "lzf_gpu_decompress_batch",
    "lzf_gpu_synth_fill",
    "lzf_host_compress_batch",
    "lzf_host_decompress_batch",
    "lzf_gpu_kernel_info",
    "lzf_gpu_kv_frame_work_size",
    "lzf_gpu_kv_frame",
    "lzf_gpu_release",
    "lzf_host_register",
    "lzf_host_unregister",
    "lzf_gpu_device_plan",
    "lzf_host_last_spread",
    "lzf_host_split",
    "lzf_host_split_block",
    "lzf_host_split_policy",
    "lzf_gpu_parse_device_list",
    "lzf_gpu_size_class",
    "lzf_gpu_size_partition_work_size",
    "lzf_gpu_size_partition",
    "lzf_host_size_partition",
    "lzf_gpu_mixed_work_size",
    "lzf_gpu_compress_mixed",
    "lzf_gpu_decompress_mixed",
    "lzf_gpu_mixed_last_plan",
    "lzf_host_compress_mixed",
    "lzf_host_decompress_mixed",
    "lzf_gpu_set_store_work_size",
    "lzf_gpu_set_store",
    "lzf_host_store_stats",
    "lzf_gpu_store_delete",
    "lzf_gpu_store_expire",
    "lzf_gpu_store_usage",
    "lzf_gpu_store_compact_work_size",
    "lzf_gpu_store_compact",
    "lzf_gpu_store_select_work_size",
    "lzf_gpu_store_select_prefix",
    "lzf_gpu_store_select_ordered_work_size",
    "lzf_gpu_store_select_ordered",
    "lzf_host_store_select_ordered",
    "lzf_gpu_store_mget_work_size",
    "lzf_gpu_store_mget",
    "lzf_gpu_store_count",
    "lzf_gpu_store_mttl",
    "lzf_gpu_key_index_bytes",
    "lzf_host_key_home",
    "lzf_gpu_key_index_insert",
    "lzf_gpu_key_index_lookup",
    "lzf_gpu_store_mlock",
    "lzf_gpu_store_munlock",
    "lzf_gpu_store_mdel",
    "lzf_gpu_store_minc_work_size",
    "lzf_gpu_store_minc",
    "lzf_host_parse_long",
    "lzf_gpu_store_set_guard",
    "lzf_gpu_store_mset_work_size",
    "lzf_gpu_store_mset",
    "lzf_gpu_store_gc",
    "lzf_host_meta_field",
    "lzf_gpu_store_meta",
    "lzf_gpu_store_keys_work_size",
    "lzf_gpu_store_keys",
    "lzf_gpu_store_replies_work_size",
    "lzf_gpu_store_replies",
    "lzf_host_reply_code",
    "lzf_gpu_store_renumber_work_size",
    "lzf_gpu_store_renumber",
    "lzf_gpu_store_remap",
    "lzf_gpu_key_index_rebuild",
    "lzf_gpu_request_parse",
    "lzf_host_request_parse",
    "lzf_host_request_reply_code",
    "lzf_gpu_store_append_keys_work_size",
    "lzf_gpu_store_append_keys",
    "lzf_host_request_class",
    "lzf_gpu_request_bucket_work_size",
    "lzf_gpu_request_bucket",
    "lzf_host_request_bucket",
    "lzf_gpu_request_stitch",
    "lzf_host_request_stitch",
)

# size classes of the mixed calls (include/lzf_gpu.h)
NCLASS = 5
KIND_COMPRESS, KIND_DECOMPRESS = 0, 1

# *status of set_store (include/lzf_gpu.h)
STORE_OK, STORE_FULL, STORE_EWORK = 0, 1, 2
# *status of store_compact and store_renumber only: a live item's value bytes
# (its key bytes) leave the source arena
STORE_ERANGE = 3
# remap of a dead item (store_renumber), and what store_remap leaves for one
STORE_NO_INDEX = 0xFFFFFFFF
# result[3] of store_mget (include/lzf_gpu.h)
MGET_OK, MGET_NOT_FOUND, MGET_TOO_BIG, MGET_EDECODE = 0, 1, 2, 3
# *status of key_index_insert (include/lzf_gpu.h)
KIDX_OK, KIDX_FULL = 0, 1
# entry_status of store_mlock / _munlock / _mdel / _minc (include/lzf_gpu.h)
ENT_DONE, ENT_DEAD, ENT_EXPIRED, ENT_LOCKED, ENT_NAN, ENT_CONVERTED, ENT_UNCHANGED = 0, 1, 2, 3, 4, 5, 6
# entry_status of store_replies: an LZF item did not decode to val_len
ENT_EDECODE = 7
# mode and result[3] of store_replies (include/lzf_gpu.h)
REPLY_GET, REPLY_VALUE = 0, 1
REPLY_OK, REPLY_TOO_BIG = 0, 1
# field of store_meta, as meta_field resolves a name (include/lzf_gpu.h)
META_SIZE, META_ENCODING, META_ACCESS, META_CREATED, META_TTL, META_LEFT, META_LOCK = 0, 1, 2, 3, 4, 5, 6

# item encodings (src/net.h:274-278) and the MGET reply code (src/query.h:71)
ENC_PLAIN, ENC_LZF, ENC_NUMBER, ENC_NULL = 0x00, 0x01, 0x02, 0xFF
REPL_KVAL = 7
# the reply codes of store_replies (src/query.h:64-70)
REPL_ERR, REPL_ERR_NOT_FOUND, REPL_ERR_NAN, REPL_ERR_LOCKED, REPL_OK, REPL_VAL = 0, 1, 2, 4, 5, 6
# the opcodes of a request (src/query.h:37-59) and the status of request_parse
(OP_SET, OP_TTL, OP_GET, OP_DEL, OP_INC, OP_DEC, OP_LOCK, OP_UNLOCK, OP_MSET, OP_MTTL, OP_MGET, OP_MDEL, OP_MINC,
 OP_MDEC, OP_MLOCK, OP_MUNLOCK, OP_COUNT, OP_STATS, OP_PING, OP_META, OP_KEYS) = range(1, 22)
OP_END = 0xFF
REQ_OK, REQ_ERR, REQ_NAN, REQ_BADOP, REQ_SHORT, REQ_ERANGE, REQ_OTHER = 0, 1, 2, 3, 4, 5, 6
REQ_NSTATUS = 7
# request dispatch: the classes of request_bucket, class_mode and out_kind of request_stitch
RQ_NCLASS = 23
STITCH_HOST, STITCH_ARENA, STITCH_CODE = 0, 1, 2
OUT_REPLY, OUT_CLOSE, OUT_HOST = 0, 1, 2


class LzfLibraryMissing(ImportError):
    pass


def lib_path():
    return os.path.join(_HERE, "liblzf_hip.so")


def diag_lib_path():
    """The diagnostic build (cross-check kernel forms; never the product)."""
    return os.path.join(_HERE, "liblzf_hip_diag.so")


_LOADED = {}


def lib():
    """Load liblzf_hip.so (built in-tree by __graft_entry__.build())."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # LZF_HIP_LIB: load a diagnostic build (e.g. liblzf_hip_stats.so) instead
    _LIB = _load(os.environ.get("LZF_HIP_LIB") or lib_path())
    return _LIB


@contextlib.contextmanager
def using(path):
    """Route this module's calls through the library at ``path`` (e.g. the
    diagnostic build) for the duration of the block."""
    global _LIB
    prev = _LIB
    _LIB = _load(path)
    try:
        yield _LIB
    finally:
        _LIB = prev


def _load(path):
    if path in _LOADED:
        return _LOADED[path]
    if not os.path.exists(path):
        raise LzfLibraryMissing(f"{path} not built: run __graft_entry__.build() "
                                "(make -C gibson_amd/csrc); there is no CPU fallback")
    try:
        L = ctypes.CDLL(path, use_errno=True)
    except OSError as e:
        raise LzfLibraryMissing(f"cannot load {path}: {e}") from e
    u32, u64, vp, i32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int32
    L.lzf_compress.restype = ctypes.c_uint
    L.lzf_compress.argtypes = [vp, ctypes.c_uint, vp, ctypes.c_uint]
    L.lzf_decompress.restype = ctypes.c_uint
    L.lzf_decompress.argtypes = [vp, ctypes.c_uint, vp, ctypes.c_uint]
    L.lzf_gpu_compress_batch.restype = ctypes.c_int
    L.lzf_gpu_compress_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u32, vp]
    L.lzf_gpu_decompress_batch.restype = ctypes.c_int
    L.lzf_gpu_decompress_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, vp]
    L.lzf_gpu_synth_fill.restype = ctypes.c_int
    L.lzf_gpu_synth_fill.argtypes = [ctypes.c_int, u64, u64, u64, u32, u32, vp, vp]
    L.lzf_host_compress_batch.restype = ctypes.c_int
    L.lzf_host_compress_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32]
    L.lzf_host_decompress_batch.restype = ctypes.c_int
    L.lzf_host_decompress_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32]
    L.lzf_gpu_release.restype = None
    L.lzf_gpu_release.argtypes = []
    L.lzf_gpu_kernel_info.restype = ctypes.c_char_p
    L.lzf_gpu_kernel_info.argtypes = []
    L.lzf_gpu_selfcheck.restype = ctypes.c_int
    L.lzf_gpu_selfcheck.argtypes = []
    L.lzf_gpu_lds_order_probe.restype = ctypes.c_int
    L.lzf_gpu_lds_order_probe.argtypes = []
    L.lzf_gpu_decoded_size_batch.restype = ctypes.c_int
    L.lzf_gpu_decoded_size_batch.argtypes = [vp, vp, vp, vp, vp, u32, u32, vp]
    L.lzf_host_decoded_size_batch.restype = ctypes.c_int
    L.lzf_host_decoded_size_batch.argtypes = [vp, vp, vp, vp, vp, u32, u32]
    L.lzf_gpu_kv_frame_work_size.restype = u64
    L.lzf_gpu_kv_frame_work_size.argtypes = [u32]
    L.lzf_gpu_kv_frame.restype = ctypes.c_int
    L.lzf_gpu_kv_frame.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, ctypes.c_int,
                                   vp, u64, vp, vp, vp]
    L.lzf_host_register.restype = ctypes.c_int
    L.lzf_host_register.argtypes = [vp, u64]
    L.lzf_host_unregister.restype = ctypes.c_int
    L.lzf_host_unregister.argtypes = [vp]
    L.lzf_gpu_device_plan.restype = ctypes.c_int
    L.lzf_gpu_device_plan.argtypes = [vp, vp, vp, ctypes.c_int]
    L.lzf_host_last_spread.restype = ctypes.c_int
    L.lzf_host_last_spread.argtypes = [vp, vp, ctypes.c_int]
    L.lzf_host_split.restype = u32
    L.lzf_host_split.argtypes = [u32, u32, u32, vp, vp]
    L.lzf_host_split_block.restype = u32
    L.lzf_host_split_block.argtypes = [u32, u32, u32, vp]
    L.lzf_host_split_policy.restype = ctypes.c_int
    L.lzf_host_split_policy.argtypes = []
    L.lzf_gpu_parse_device_list.restype = ctypes.c_int
    L.lzf_gpu_parse_device_list.argtypes = [ctypes.c_char_p, ctypes.c_int, vp, ctypes.c_int]
    if hasattr(L, "lzf_gpu_compress_mixed"):
        _bind_mixed(L)
    if hasattr(L, "lzf_gpu_set_store"):
        _bind_store(L)
    if hasattr(L, "lzf_gpu_store_compact"):
        _bind_store_lifecycle(L)
    if hasattr(L, "lzf_gpu_store_mget"):
        _bind_store_index(L)
    if hasattr(L, "lzf_gpu_key_index_insert"):
        _bind_key_index(L)
    if hasattr(L, "lzf_gpu_store_minc"):
        _bind_store_ops(L)
    if hasattr(L, "lzf_gpu_store_mset"):
        _bind_store_mset(L)
    if hasattr(L, "lzf_gpu_store_replies"):
        _bind_store_replies(L)
    if hasattr(L, "lzf_gpu_store_renumber"):
        _bind_store_renumber(L)
    if hasattr(L, "lzf_gpu_request_parse"):
        _bind_request(L)
    if hasattr(L, "lzf_gpu_request_bucket"):
        _bind_dispatch(L)
    del i32
    _LOADED[path] = L
    return L


def _bind_mixed(L):
    """The mixed-size calls.  A build from before they existed, given by
    LZF_HIP_LIB for an A/B of the uniform calls, has none of them: the mixed
    helpers below then raise AttributeError, they do not fall back."""
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.lzf_gpu_size_class.restype = ctypes.c_int
    L.lzf_gpu_size_class.argtypes = [u32, ctypes.c_int]
    L.lzf_gpu_size_partition_work_size.restype = u64
    L.lzf_gpu_size_partition_work_size.argtypes = [u32]
    L.lzf_gpu_size_partition.restype = ctypes.c_int
    L.lzf_gpu_size_partition.argtypes = [vp, u32, u32, ctypes.c_int, vp, vp, vp, vp, vp]
    L.lzf_host_size_partition.restype = ctypes.c_int
    L.lzf_host_size_partition.argtypes = [vp, u32, u32, ctypes.c_int, vp, vp, vp]
    L.lzf_gpu_mixed_work_size.restype = u64
    L.lzf_gpu_mixed_work_size.argtypes = [u32]
    L.lzf_gpu_compress_mixed.restype = ctypes.c_int
    L.lzf_gpu_compress_mixed.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u32, vp, vp]
    L.lzf_gpu_decompress_mixed.restype = ctypes.c_int
    L.lzf_gpu_decompress_mixed.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, vp, vp]
    L.lzf_gpu_mixed_last_plan.restype = ctypes.c_int
    L.lzf_gpu_mixed_last_plan.argtypes = [vp, vp, vp, ctypes.c_int]
    L.lzf_host_compress_mixed.restype = ctypes.c_int
    L.lzf_host_compress_mixed.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32]
    L.lzf_host_decompress_mixed.restype = ctypes.c_int
    L.lzf_host_decompress_mixed.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32]


def _bind_store(L):
    """The device SET path; like the mixed calls, absent from an older build
    given by LZF_HIP_LIB (the helpers below then raise AttributeError)."""
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.lzf_gpu_set_store_work_size.restype = u64
    L.lzf_gpu_set_store_work_size.argtypes = [u32, u64]
    L.lzf_gpu_set_store.restype = ctypes.c_int
    L.lzf_gpu_set_store.argtypes = [vp, vp, vp, u32, u32, u64, u32, vp, u64, vp, vp, vp, vp, vp, vp, vp]
    L.lzf_host_store_stats.restype = ctypes.c_int
    L.lzf_host_store_stats.argtypes = [vp, vp, vp, u32, vp, vp]


def _bind_store_lifecycle(L):
    """Delete, expire, usage and compact of the device store; absent from an
    older build given by LZF_HIP_LIB (the helpers below then raise
    AttributeError)."""
    u32, u64, vp, i64 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64
    L.lzf_gpu_store_delete.restype = ctypes.c_int
    L.lzf_gpu_store_delete.argtypes = [vp, u32, vp, u32, vp]
    L.lzf_gpu_store_expire.restype = ctypes.c_int
    L.lzf_gpu_store_expire.argtypes = [vp, vp, i64, vp, u32, vp, vp]
    L.lzf_gpu_store_usage.restype = ctypes.c_int
    L.lzf_gpu_store_usage.argtypes = [vp, vp, u32, vp, vp, vp]
    L.lzf_gpu_store_compact_work_size.restype = u64
    L.lzf_gpu_store_compact_work_size.argtypes = [u32]
    L.lzf_gpu_store_compact.restype = ctypes.c_int
    L.lzf_gpu_store_compact.argtypes = [vp, u64, vp, vp, vp, u32, vp, u64, vp, vp, vp, vp, vp]


class _StoreItems(ctypes.Structure):
    """lzf_store_items of include/lzf_gpu.h: ten device pointers"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("val_off", "val_size", "enc", "val_len", "key_off", "key_len",
                                               "item_time", "item_ttl", "item_lock", "last_access")]


def _bind_store_renumber(L):
    """The renumbering, the remap of an index list and the key index's
    rebuild; absent from an older build given by LZF_HIP_LIB (the helpers
    below then raise AttributeError)."""
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    items = vp                             # const lzf_store_items *, passed with ctypes.byref
    L.lzf_gpu_store_renumber_work_size.restype = u64
    L.lzf_gpu_store_renumber_work_size.argtypes = [u32]
    L.lzf_gpu_store_renumber.restype = ctypes.c_int
    L.lzf_gpu_store_renumber.argtypes = [items, u32, vp, u64, items, u32, vp, u64, vp, vp, vp, vp, vp, vp]
    L.lzf_gpu_store_remap.restype = ctypes.c_int
    L.lzf_gpu_store_remap.argtypes = [vp, u32, vp, u32, vp]
    L.lzf_gpu_key_index_rebuild.restype = ctypes.c_int
    L.lzf_gpu_key_index_rebuild.argtypes = [vp, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp]


def _bind_request(L):
    """Request ingest: the parse of raw requests and the key append of a SET
    batch; absent from an older build given by LZF_HIP_LIB (the helpers below
    then raise AttributeError)."""
    u32, u64, vp, i64, i32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    L.lzf_gpu_request_parse.restype = ctypes.c_int
    L.lzf_gpu_request_parse.argtypes = [vp, u64, vp, vp, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lzf_host_request_parse.restype = ctypes.c_int
    L.lzf_host_request_parse.argtypes = [vp, u64, vp, vp, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lzf_host_request_reply_code.restype = ctypes.c_int
    L.lzf_host_request_reply_code.argtypes = [ctypes.c_int]
    L.lzf_gpu_store_append_keys_work_size.restype = u64
    L.lzf_gpu_store_append_keys_work_size.argtypes = [u32]
    L.lzf_gpu_store_append_keys.restype = ctypes.c_int
    L.lzf_gpu_store_append_keys.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp, vp,
                                            u32, u32, i64, i32, vp, vp, vp, vp, vp]


def _bind_dispatch(L):
    """Request dispatch: the bucket of a parsed batch by operator class and the
    stitch of its replies; absent from an older build given by LZF_HIP_LIB (the
    helpers below then raise AttributeError)."""
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.lzf_host_request_class.restype = ctypes.c_int
    L.lzf_host_request_class.argtypes = [ctypes.c_int, ctypes.c_int]
    L.lzf_gpu_request_bucket_work_size.restype = u64
    L.lzf_gpu_request_bucket_work_size.argtypes = [u32]
    L.lzf_gpu_request_bucket.restype = ctypes.c_int
    L.lzf_gpu_request_bucket.argtypes = [vp] * 7 + [u32] + [vp] * 10 + [vp, vp]
    L.lzf_host_request_bucket.restype = ctypes.c_int
    L.lzf_host_request_bucket.argtypes = [vp] * 7 + [u32] + [vp] * 10
    L.lzf_gpu_request_stitch.restype = ctypes.c_int
    L.lzf_gpu_request_stitch.argtypes = [vp, vp, vp, u32] + [vp] * 8 + [u64, u64, vp, vp, vp, vp, vp]
    L.lzf_host_request_stitch.restype = ctypes.c_int
    L.lzf_host_request_stitch.argtypes = [vp, vp, vp, u32] + [vp] * 8 + [u64, u64, vp, vp, vp, vp]


def _bind_store_index(L):
    """The prefix select and the index-list operators (MGET, COUNT, MTTL) of
    the device store; absent from an older build given by LZF_HIP_LIB (the
    helpers below then raise AttributeError)."""
    u32, u64, vp, i64, i32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    L.lzf_gpu_store_select_work_size.restype = u64
    L.lzf_gpu_store_select_work_size.argtypes = [u32]
    L.lzf_gpu_store_select_prefix.restype = ctypes.c_int
    L.lzf_gpu_store_select_prefix.argtypes = [vp, vp, vp, vp, u32, vp, u32, vp, u32, vp, vp, vp]
    L.lzf_gpu_store_select_ordered_work_size.restype = u64
    L.lzf_gpu_store_select_ordered_work_size.argtypes = [u32, u32, u64, u32]
    L.lzf_gpu_store_select_ordered.restype = ctypes.c_int
    L.lzf_gpu_store_select_ordered.argtypes = [vp, vp, vp, vp, u32, vp, u32, i64, u32, u64, vp, u32, vp, vp, vp]
    L.lzf_host_store_select_ordered.restype = ctypes.c_int
    L.lzf_host_store_select_ordered.argtypes = [vp, vp, vp, vp, u32, vp, u32, i64, u32, u64, vp, u32, vp]
    L.lzf_gpu_store_mget_work_size.restype = u64
    L.lzf_gpu_store_mget_work_size.argtypes = [u32]
    L.lzf_gpu_store_mget.restype = ctypes.c_int
    L.lzf_gpu_store_mget.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp, i64, vp, u32, ctypes.c_int,
                                     vp, u64, vp, vp, vp, vp]
    L.lzf_gpu_store_count.restype = ctypes.c_int
    L.lzf_gpu_store_count.argtypes = [vp, u32, vp, u32, vp, vp, i64, vp, vp, vp]
    L.lzf_gpu_store_mttl.restype = ctypes.c_int
    L.lzf_gpu_store_mttl.argtypes = [vp, u32, i32, vp, u32, vp, vp, i64, vp, vp, vp]


def _bind_key_index(L):
    """The device key index; absent from an older build given by LZF_HIP_LIB
    (the helpers below then raise AttributeError)."""
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.lzf_gpu_key_index_bytes.restype = u64
    L.lzf_gpu_key_index_bytes.argtypes = [u32]
    L.lzf_host_key_home.restype = u32
    L.lzf_host_key_home.argtypes = [vp, u32, u32]
    L.lzf_gpu_key_index_insert.restype = ctypes.c_int
    L.lzf_gpu_key_index_insert.argtypes = [vp, u32, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp]
    L.lzf_gpu_key_index_lookup.restype = ctypes.c_int
    L.lzf_gpu_key_index_lookup.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp]


def _bind_store_ops(L):
    """Locks, the lock-aware DEL, INC / DEC and the SET guard of the device
    store; absent from an older build given by LZF_HIP_LIB (the helpers below
    then raise AttributeError)."""
    u32, u64, vp, i64 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64
    L.lzf_gpu_store_mlock.restype = ctypes.c_int
    L.lzf_gpu_store_mlock.argtypes = [vp, u32, i64, vp, u32, vp, vp, vp, i64, vp, vp, vp, vp]
    L.lzf_gpu_store_munlock.restype = ctypes.c_int
    L.lzf_gpu_store_munlock.argtypes = [vp, u32, vp, u32, vp, vp, vp, i64, vp, vp, vp, vp]
    L.lzf_gpu_store_mdel.restype = ctypes.c_int
    L.lzf_gpu_store_mdel.argtypes = [vp, u32, vp, u32, vp, vp, vp, i64, vp, vp, vp]
    L.lzf_gpu_store_minc_work_size.restype = u64
    L.lzf_gpu_store_minc_work_size.argtypes = [u32]
    L.lzf_gpu_store_minc.restype = ctypes.c_int
    L.lzf_gpu_store_minc.argtypes = [vp, u32, i64, ctypes.c_int, vp, u64, vp, vp, vp, vp, u32, vp, vp, vp, i64, vp,
                                     vp, vp, vp, vp, vp, vp]
    L.lzf_host_parse_long.restype = ctypes.c_int
    L.lzf_host_parse_long.argtypes = [vp, u32, vp]
    L.lzf_gpu_store_set_guard.restype = ctypes.c_int
    L.lzf_gpu_store_set_guard.argtypes = [vp, u32, u32, vp, u32, vp, vp, i64, vp, vp, vp]


def _bind_store_mset(L):
    """MSET by prefix, the memory sweep, META and the KEYS frame of the device
    store; absent from an older build given by LZF_HIP_LIB (the helpers below
    then raise AttributeError)."""
    u32, u64, vp, i64 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64
    L.lzf_gpu_store_mset_work_size.restype = u64
    L.lzf_gpu_store_mset_work_size.argtypes = [u32, u32]
    L.lzf_gpu_store_mset.restype = ctypes.c_int
    L.lzf_gpu_store_mset.argtypes = [vp, u32, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp, u32, vp, vp, vp, i64, vp, vp,
                                     vp, vp, vp, vp]
    L.lzf_gpu_store_gc.restype = ctypes.c_int
    L.lzf_gpu_store_gc.argtypes = [vp, i64, i64, vp, vp, u32, vp, u64, vp, vp]
    L.lzf_host_meta_field.restype = ctypes.c_int
    L.lzf_host_meta_field.argtypes = [vp, u32]
    L.lzf_gpu_store_meta.restype = ctypes.c_int
    L.lzf_gpu_store_meta.argtypes = [vp, u32, ctypes.c_int, vp, vp, u32, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    L.lzf_gpu_store_keys_work_size.restype = u64
    L.lzf_gpu_store_keys_work_size.argtypes = [u32]
    L.lzf_gpu_store_keys.restype = ctypes.c_int
    L.lzf_gpu_store_keys.argtypes = [vp, u32, vp, vp, vp, vp, u32, ctypes.c_int, vp, u64, vp, vp, vp, vp]


def _bind_store_replies(L):
    """The per-request replies of the device store; absent from an older build
    given by LZF_HIP_LIB (the helpers below then raise AttributeError)."""
    u32, u64, vp, i64 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64
    L.lzf_gpu_store_replies_work_size.restype = u64
    L.lzf_gpu_store_replies_work_size.argtypes = [u32]
    L.lzf_gpu_store_replies.restype = ctypes.c_int
    L.lzf_gpu_store_replies.argtypes = [vp, u32, ctypes.c_int, vp, vp, vp, vp, vp, vp, u32, vp, vp, i64, vp, u32,
                                        vp, u64, vp, vp, vp, vp, vp, vp, vp]
    L.lzf_host_reply_code.restype = ctypes.c_int
    L.lzf_host_reply_code.argtypes = [ctypes.c_int]


def selfcheck():
    """lzf_gpu_selfcheck(): 1 when the lane-ordered LDS exchange held on the
    current device, 0 when compress batches fall back to window64."""
    return int(lib().lzf_gpu_selfcheck())


def lds_order_probe():
    """lzf_gpu_lds_order_probe(): mismatching lanes of a fresh probe run."""
    return int(lib().lzf_gpu_lds_order_probe())


def decoded_size_batch(inp, in_off, in_len, out_size, err, out_limit, stream=None):
    """Device pre-pass: out_size/err of lzf_decompress at out_len = out_limit."""
    _check(lib().lzf_gpu_decoded_size_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out_size), _ptr(err),
                                            int(in_off.numel()), int(out_limit), _stream_handle(stream)),
           "lzf_gpu_decoded_size_batch")


def kernel_info():
    return lib().lzf_gpu_kernel_info().decode()


def release():
    """lzf_gpu_release(): free the device scratch and this thread's staging."""
    lib().lzf_gpu_release()


def _check(rc, what):
    if rc != LZF_GPU_OK:
        raise RuntimeError(f"{what} failed: {_ERRS.get(rc, rc)}")


# ---- single-call drop-in (src/lzf.h:76-97) -------------------------------

def lzf_compress(data, out_len):
    """Compress ``data`` into at most ``out_len`` bytes; None if it does not fit."""
    data = bytes(data)
    src = ctypes.create_string_buffer(data, max(len(data), 1))
    dst = ctypes.create_string_buffer(max(out_len, 1))
    r = lib().lzf_compress(src, len(data), dst, out_len)
    return dst.raw[:r] if r else None


def lzf_decompress(data, out_len):
    """Decode ``data``; returns (bytes, 0) or (None, errno)."""
    data = bytes(data)
    # the reference reads one control byte even when in_len == 0
    src = ctypes.create_string_buffer(data + b"\xff", len(data) + 1)
    dst = ctypes.create_string_buffer(max(out_len, 1))
    ctypes.set_errno(0)
    r = lib().lzf_decompress(src, len(data), dst, out_len)
    if r:
        return dst.raw[:r], 0
    return None, ctypes.get_errno()


# ---- device batches over torch tensors -------------------------------------

def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream_handle(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream)


def compress_batch(inp, in_off, in_len, out, out_off, out_cap, out_len, max_in_len, stream=None):
    """Device batch compress; all tensors on the same CUDA (HIP) device.
    inp/out uint8, *_off int64, in_len/out_cap/out_len int32 (read as u32)."""
    n = in_len.numel()
    rc = lib().lzf_gpu_compress_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out),
                                      _ptr(out_off), _ptr(out_cap), _ptr(out_len), n,
                                      int(max_in_len), _stream_handle(stream))
    _check(rc, "lzf_gpu_compress_batch")


def decompress_batch(inp, in_off, in_len, out, out_off, out_cap, out_len, err, max_out_cap,
                     stream=None):
    n = in_len.numel()
    rc = lib().lzf_gpu_decompress_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out),
                                        _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(err),
                                        n, int(max_out_cap), _stream_handle(stream))
    _check(rc, "lzf_gpu_decompress_batch")


def synth_fill(kind, seed, first, stride, count, n, out, stream=None):
    rc = lib().lzf_gpu_synth_fill(int(kind), int(seed), int(first), int(stride), int(count),
                                  int(n), _ptr(out), _stream_handle(stream))
    _check(rc, "lzf_gpu_synth_fill")


def _np_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def host_compress_batch(inp, in_off, in_len, out, out_off, out_cap, out_len):
    """Host-memory batch (numpy arrays): PCIe staging inside the library."""
    rc = lib().lzf_host_compress_batch(_np_ptr(inp), _np_ptr(in_off), _np_ptr(in_len),
                                       _np_ptr(out), _np_ptr(out_off), _np_ptr(out_cap),
                                       _np_ptr(out_len), len(in_len))
    _check(rc, "lzf_host_compress_batch")


def host_decompress_batch(inp, in_off, in_len, out, out_off, out_cap, out_len, err):
    rc = lib().lzf_host_decompress_batch(_np_ptr(inp), _np_ptr(in_off), _np_ptr(in_len),
                                         _np_ptr(out), _np_ptr(out_off), _np_ptr(out_cap),
                                         _np_ptr(out_len), _np_ptr(err), len(in_len))
    _check(rc, "lzf_host_decompress_batch")


# ---- mixed-size batches: one class batch per size class --------------------

def size_class(n, kind):
    """lzf_gpu_size_class(): the class of a length (KIND_COMPRESS: in_len,
    KIND_DECOMPRESS: out_cap)."""
    c = int(lib().lzf_gpu_size_class(int(n), int(kind)))
    if c < 0:
        raise ValueError(f"lzf_gpu_size_class: bad kind {kind}")
    return c


def size_partition(lens, bound, kind, stream=None):
    """Device partition of an int32 CUDA tensor of lengths (read as u32):
    returns (perm, class_count, class_max) as CUDA int32 tensors, the last two
    of NCLASS + 1 entries (the last: values past ``bound``)."""
    import torch
    n = lens.numel()
    perm = torch.empty(n, dtype=torch.int32, device=lens.device)
    cc = torch.empty(NCLASS + 1, dtype=torch.int32, device=lens.device)
    cm = torch.empty(NCLASS + 1, dtype=torch.int32, device=lens.device)
    work = torch.empty(int(lib().lzf_gpu_size_partition_work_size(n)), dtype=torch.uint8, device=lens.device)
    _check(lib().lzf_gpu_size_partition(_ptr(lens), n, int(bound), int(kind), _ptr(perm), _ptr(cc), _ptr(cm),
                                        _ptr(work), _stream_handle(stream)), "lzf_gpu_size_partition")
    return perm, cc, cm


def host_size_partition(lens, bound, kind):
    """The same partition over a numpy uint32 array, on the host (no GPU):
    (perm, class_count, class_max) as numpy uint32 arrays."""
    import numpy as np
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    perm = np.empty(len(lens), dtype=np.uint32)
    cc = np.empty(NCLASS + 1, dtype=np.uint32)
    cm = np.empty(NCLASS + 1, dtype=np.uint32)
    _check(lib().lzf_host_size_partition(_np_ptr(lens), len(lens), int(bound), int(kind), _np_ptr(perm),
                                         _np_ptr(cc), _np_ptr(cm)), "lzf_host_size_partition")
    return perm, cc, cm


def mixed_work(count, device):
    """A scratch tensor for one mixed device call of ``count`` values."""
    import torch
    return torch.empty(int(lib().lzf_gpu_mixed_work_size(int(count))), dtype=torch.uint8, device=device)


def compress_mixed(inp, in_off, in_len, out, out_off, out_cap, out_len, max_in_len, work=None, stream=None):
    """compress_batch with per-class routing.  Waits once for the 48-byte
    plan before it launches the class batches; ``work`` (mixed_work) defaults
    to a fresh tensor and must outlive the stream's work."""
    n = in_len.numel()
    if work is None:
        work = mixed_work(n, inp.device)
    rc = lib().lzf_gpu_compress_mixed(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off),
                                      _ptr(out_cap), _ptr(out_len), n, int(max_in_len), _ptr(work),
                                      _stream_handle(stream))
    _check(rc, "lzf_gpu_compress_mixed")
    return work


def decompress_mixed(inp, in_off, in_len, out, out_off, out_cap, out_len, err, max_out_cap, work=None,
                     stream=None):
    """decompress_batch with per-class routing (see compress_mixed)."""
    n = in_len.numel()
    if work is None:
        work = mixed_work(n, inp.device)
    rc = lib().lzf_gpu_decompress_mixed(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off),
                                        _ptr(out_cap), _ptr(out_len), _ptr(err), n, int(max_out_cap),
                                        _ptr(work), _stream_handle(stream))
    _check(rc, "lzf_gpu_decompress_mixed")
    return work


def mixed_last_plan():
    """This thread's last mixed device call: {"batches", "class_count",
    "class_max", "route"}, lists of NCLASS + 1 entries.  route: 0 empty;
    compress 1 lane, 2 table, 3 window64; decompress 1 tokpar, 2 tokpar-far,
    3 pipe."""
    cc, cm = (ctypes.c_uint32 * (NCLASS + 1))(), (ctypes.c_uint32 * (NCLASS + 1))()
    rt = (ctypes.c_int * (NCLASS + 1))()
    n = lib().lzf_gpu_mixed_last_plan(cc, cm, rt, NCLASS + 1)
    return {"batches": int(n), "class_count": list(cc), "class_max": list(cm), "route": list(rt)}


def host_compress_mixed(inp, in_off, in_len, out, out_off, out_cap, out_len):
    """host_compress_batch, one uniform host call per size class."""
    rc = lib().lzf_host_compress_mixed(_np_ptr(inp), _np_ptr(in_off), _np_ptr(in_len), _np_ptr(out),
                                       _np_ptr(out_off), _np_ptr(out_cap), _np_ptr(out_len), len(in_len))
    _check(rc, "lzf_host_compress_mixed")


def host_decompress_mixed(inp, in_off, in_len, out, out_off, out_cap, out_len, err):
    rc = lib().lzf_host_decompress_mixed(_np_ptr(inp), _np_ptr(in_off), _np_ptr(in_len), _np_ptr(out),
                                         _np_ptr(out_off), _np_ptr(out_cap), _np_ptr(out_len), _np_ptr(err),
                                         len(in_len))
    _check(rc, "lzf_host_decompress_mixed")


# ---- SET batch into a device-resident store ---------------------------------

def set_store_work(count, in_bytes, device):
    """A scratch tensor for one set_store call of ``count`` values whose
    lengths sum to at most ``in_bytes``."""
    import torch
    return torch.empty(int(lib().lzf_gpu_set_store_work_size(int(count), int(in_bytes))), dtype=torch.uint8,
                       device=device)


def set_store(inp, in_off, in_len, compression, max_in_len, in_bytes, store, store_used, val_off, val_size, enc,
              status, work=None, stream=None):
    """gbSingleSet for a batch, the values staying on the device: compress
    every value longer than ``compression``, decide LZF / PLAIN, and pack the
    stored bytes densely into ``store`` from ``store_used[0]`` on, which is
    advanced.  Writes the arrays kv_frame reads (pass ``in_len`` there as
    val_len).  Tensors on one device: inp/store/enc uint8, in_off/val_off/
    store_used (1 element) int64, in_len/val_size/status (1 element) int32.
    status: STORE_OK, or STORE_FULL / STORE_EWORK with the whole batch refused
    (every enc ENC_NULL).  No host wait; ``work`` (set_store_work) defaults to
    a fresh tensor and must outlive the stream's work."""
    n = in_len.numel()
    if work is None:
        work = set_store_work(n, in_bytes, inp.device)
    rc = lib().lzf_gpu_set_store(_ptr(inp), _ptr(in_off), _ptr(in_len), n, int(max_in_len), int(in_bytes),
                                 int(compression), _ptr(store), int(store.numel()), _ptr(store_used), _ptr(val_off),
                                 _ptr(val_size), _ptr(enc), _ptr(status), _ptr(work), _stream_handle(stream))
    _check(rc, "lzf_gpu_set_store")
    return work


def store_stats(enc, val_size, val_len, compravg=0.0, ncompressed=0):
    """lzf_host_store_stats(): the STATS running mean (src/query.c:400-405)
    folded over a set_store batch's results in request order, on the host.
    Takes numpy arrays or tensors (copied to the host); returns
    (compravg, ncompressed)."""
    import numpy as np

    def host(a, dt):
        if hasattr(a, "cpu"):
            a = a.cpu().numpy()
        a = np.ascontiguousarray(a)
        return a.view(dt) if a.dtype.itemsize == np.dtype(dt).itemsize else a.astype(dt)

    e, s, v = host(enc, np.uint8), host(val_size, np.uint32), host(val_len, np.uint32)
    if not len(e) == len(s) == len(v):
        raise ValueError("store_stats: arrays of different lengths")
    avg, n = ctypes.c_double(compravg), ctypes.c_uint64(ncompressed)
    _check(lib().lzf_host_store_stats(_np_ptr(e), _np_ptr(s), _np_ptr(v), len(e), ctypes.byref(avg),
                                      ctypes.byref(n)), "lzf_host_store_stats")
    return avg.value, n.value


# ---- the device store's lifecycle --------------------------------------------

def store_delete(idx, enc, stream=None):
    """DEL / overwrite by index: enc[idx[k]] = ENC_NULL.  idx int32 (read as
    u32), enc uint8, on one device; an index past enc's length is ignored and
    duplicates are fine.  No host wait."""
    _check(lib().lzf_gpu_store_delete(_ptr(idx), int(idx.numel()), _ptr(enc), int(enc.numel()),
                                      _stream_handle(stream)), "lzf_gpu_store_delete")


def store_expire(item_time, ttl, now, enc, expired, stream=None):
    """TTL sweep (src/query.c:186-189): item i becomes ENC_NULL iff ttl[i] > 0
    and now - item_time[i] >= ttl[i].  item_time int64, ttl int32, enc uint8,
    expired (1 element, int32) receives how many items this call nulled.  No
    host wait."""
    _check(lib().lzf_gpu_store_expire(_ptr(item_time), _ptr(ttl), int(now), _ptr(enc), int(enc.numel()),
                                      _ptr(expired), _stream_handle(stream)), "lzf_gpu_store_expire")


def store_compact_work(count, device):
    """A scratch tensor for one store_usage or store_compact call over
    ``count`` items."""
    import torch
    return torch.empty(int(lib().lzf_gpu_store_compact_work_size(int(count))), dtype=torch.uint8, device=device)


def store_usage(val_size, enc, report, work=None, stream=None):
    """report (4 elements, int64) = live items, their bytes, dead items, the
    bytes the dead items' sizes still name.  No host wait; returns ``work``,
    which must outlive the stream's work."""
    n = enc.numel()
    if work is None:
        work = store_compact_work(n, enc.device)
    _check(lib().lzf_gpu_store_usage(_ptr(val_size), _ptr(enc), n, _ptr(report), _ptr(work),
                                     _stream_handle(stream)), "lzf_gpu_store_usage")
    return work


def store_compact(src, val_off, val_size, enc, dst, dst_used, report, status, work=None, stream=None):
    """Semispace compaction: the stored bytes of every item with enc !=
    ENC_NULL copied from ``src`` and packed densely in index order into
    ``dst`` from ``dst_used[0]`` on, which is advanced; val_off / val_size
    rewritten for ``dst`` (a dead item: size 0).  The caps are the tensors'
    lengths.  status (1 element, int32): STORE_OK, or STORE_FULL /
    STORE_ERANGE with the call refused whole and nothing changed; report as
    store_usage fills it, either way.  No host wait; returns ``work``
    (store_compact_work), which must outlive the stream's work."""
    n = enc.numel()
    if work is None:
        work = store_compact_work(n, src.device)
    rc = lib().lzf_gpu_store_compact(_ptr(src), int(src.numel()), _ptr(val_off), _ptr(val_size), _ptr(enc), n,
                                     _ptr(dst), int(dst.numel()), _ptr(dst_used), _ptr(report), _ptr(status),
                                     _ptr(work), _stream_handle(stream))
    _check(rc, "lzf_gpu_store_compact")
    return work


# ---- prefix operators over the device store -----------------------------------

def _opt_ptr(t):
    return ctypes.c_void_p(0) if t is None else _ptr(t)


# ---- the renumbering: item indices and key bytes given back ---------------------

class StoreItems:
    """One set of the store's item arrays (lzf_store_items): val_off int64,
    val_size int32, enc uint8, val_len int32, key_off int64, key_len int32,
    and the optional item_time int64 with item_ttl int32, item_lock int64,
    last_access int64.  Tensors of one length on one device; an absent
    optional member is None."""
    FIELDS = tuple(n for n, _ in _StoreItems._fields_)

    def __init__(self, val_off, val_size, enc, val_len, key_off, key_len, item_time=None, item_ttl=None,
                 item_lock=None, last_access=None):
        self.val_off, self.val_size, self.enc, self.val_len = val_off, val_size, enc, val_len
        self.key_off, self.key_len = key_off, key_len
        self.item_time, self.item_ttl, self.item_lock, self.last_access = item_time, item_ttl, item_lock, last_access

    @classmethod
    def of(cls, items):
        """``items`` itself, or a StoreItems from a dict with these names"""
        return items if isinstance(items, cls) else cls(**dict(items))

    def _struct(self):
        s = _StoreItems()
        for n in self.FIELDS:
            t = getattr(self, n)
            setattr(s, n, None if t is None else t.data_ptr())
        return s


def store_renumber_work(count, device):
    """A scratch tensor for one store_renumber call over ``count`` items."""
    import torch
    return torch.empty(int(lib().lzf_gpu_store_renumber_work_size(int(count))), dtype=torch.uint8, device=device)


def store_renumber(src, src_keys, dst, dst_keys, dst_keys_used, report, status, remap=None, work=None, stream=None):
    """The live items of ``src`` (a StoreItems, or a dict with its names;
    count = the length of src.enc) copied dense and in index order into
    ``dst`` (dst_cap = the length of dst.enc), their key bytes packed from
    ``src_keys`` into ``dst_keys`` from ``dst_keys_used[0]`` on, which is
    advanced; the entries of dst past the live items become dead items.  The
    key caps are the tensors' lengths.  remap (count elements, int32 read as
    u32, optional): the new index per old item, STORE_NO_INDEX for a dead one.
    report (4 elements, int64) = live items, their key bytes, dead items, the
    key bytes the dead items still name; status (1 element, int32): STORE_OK,
    or STORE_FULL / STORE_ERANGE with the call refused whole and nothing
    written.  Value bytes do not move (store_compact does that) and the TTL
    rule is not applied (store_expire does that).  No host wait; returns
    ``work`` (store_renumber_work), which must outlive the stream's work."""
    src, dst = StoreItems.of(src), StoreItems.of(dst)
    n = src.enc.numel()
    if work is None:
        work = store_renumber_work(n, src.enc.device)
    s, d = src._struct(), dst._struct()
    rc = lib().lzf_gpu_store_renumber(ctypes.byref(s), n, _ptr(src_keys), int(src_keys.numel()), ctypes.byref(d),
                                      int(dst.enc.numel()), _ptr(dst_keys), int(dst_keys.numel()),
                                      _ptr(dst_keys_used), _opt_ptr(remap), _ptr(report), _ptr(status), _ptr(work),
                                      _stream_handle(stream))
    _check(rc, "lzf_gpu_store_renumber")
    return work


def store_remap(idx, remap, stream=None):
    """An index list from before a store_renumber translated in place through
    its ``remap``: idx[k] = remap[idx[k]], STORE_NO_INDEX for an entry past the
    old store (padding included).  No host wait."""
    _check(lib().lzf_gpu_store_remap(_ptr(idx), int(idx.numel()), _ptr(remap), int(remap.numel()),
                                     _stream_handle(stream)), "lzf_gpu_store_remap")


def store_select_work(count, device):
    """A scratch tensor for one store_select_prefix call over ``count`` items."""
    import torch
    return torch.empty(int(lib().lzf_gpu_store_select_work_size(int(count))), dtype=torch.uint8, device=device)


def store_select_prefix(keys, key_off, key_len, enc, prefix, sel, result, work=None, stream=None):
    """tr_search on the device: sel (int32, read as u32; its length is the cap)
    receives, in ascending order, the indices of the items that are not
    ENC_NULL and whose key starts with ``prefix`` (a uint8 tensor on the
    device), padded with 0xFFFFFFFF (-1); result (2 elements, int32) = [min(matches,
    cap), matches].  Expired items match too: the consuming operator drops
    them.  Index order is not the reference's trie order (include/lzf_gpu.h).
    No host wait; returns ``work`` (store_select_work), which must outlive the
    stream's work."""
    n = enc.numel()
    if work is None:
        work = store_select_work(n, enc.device)
    rc = lib().lzf_gpu_store_select_prefix(_ptr(keys), _ptr(key_off), _ptr(key_len), _ptr(enc), n, _ptr(prefix),
                                           int(prefix.numel()), _ptr(sel), int(sel.numel()), _ptr(result),
                                           _ptr(work), _stream_handle(stream))
    _check(rc, "lzf_gpu_store_select_prefix")
    return work


ORDER_OK, ORDER_EWORK = 0, 1                     # lzf_gpu.h: LZF_ORDER_*


def store_select_ordered_work(count, cand_cap, node_cap, cap, device):
    """A scratch tensor for one store_select_ordered call over ``count`` items
    with room for ``cand_cap`` candidates and ``node_cap`` node words."""
    import torch
    size = int(lib().lzf_gpu_store_select_ordered_work_size(int(count), int(cand_cap), int(node_cap), int(cap)))
    if size == 2**64 - 1:
        raise ValueError("store_select_ordered_work: the size does not fit 64 bits")
    return torch.empty(size, dtype=torch.uint8, device=device)


def store_select_ordered(keys, key_off, key_len, enc, prefix, sel, result, limit=-1, cand_cap=None, node_cap=None,
                         work=None, stream=None):
    """tr_search on the device, in the reference's order: sel (int32, read as
    u32; its length is the cap) receives the indices of the items that are not
    ENC_NULL and whose key starts with ``prefix`` (a uint8 tensor on the
    device) in trie pre-order with the children in creation order, cut to
    ``limit`` when it is positive, padded with 0xFFFFFFFF (-1).  The order
    follows from the keys of all the items, dead ones included
    (include/lzf_gpu.h).  result (5 elements, int64) = entries written, live
    matches, candidates (matches and dead items of the prefix), node words
    needed, ORDER_OK or ORDER_EWORK: more candidates than ``cand_cap`` (default:
    the item count) or more node words than ``node_cap`` (default: the length
    of ``keys``); sel is then all padding, and result[2] and result[3] say what
    a repeat needs.  No host wait; returns ``work``
    (store_select_ordered_work), which must outlive the stream's work."""
    n = enc.numel()
    cand_cap = n if cand_cap is None else int(cand_cap)
    node_cap = max(1, int(keys.numel())) if node_cap is None else int(node_cap)
    if work is None:
        work = store_select_ordered_work(n, cand_cap, node_cap, sel.numel(), enc.device)
    rc = lib().lzf_gpu_store_select_ordered(_ptr(keys), _ptr(key_off), _ptr(key_len), _ptr(enc), n, _ptr(prefix),
                                            int(prefix.numel()), int(limit), cand_cap, node_cap, _ptr(sel),
                                            int(sel.numel()), _ptr(result), _ptr(work), _stream_handle(stream))
    _check(rc, "lzf_gpu_store_select_ordered")
    return work


def host_select_ordered(keys, key_off, key_len, enc, prefix, cap, limit=-1, cand_cap=None, node_cap=None):
    """lzf_host_store_select_ordered(): the same rule over numpy arrays on the
    host, as the reference's trie and its walk.  keys/enc/prefix uint8, key_off
    uint64, key_len uint32.  Returns (sel, result): uint32[cap] and uint64[5]."""
    import numpy as np
    k, o = np.ascontiguousarray(keys, np.uint8), np.ascontiguousarray(key_off).astype(np.uint64)
    ln, e = np.ascontiguousarray(key_len).astype(np.uint32), np.ascontiguousarray(enc, np.uint8)
    p = np.ascontiguousarray(prefix, np.uint8)
    if not len(o) == len(ln) == len(e):
        raise ValueError("host_select_ordered: arrays of different lengths")
    sel, result = np.zeros(int(cap), np.uint32), np.zeros(5, np.uint64)
    cand_cap = len(e) if cand_cap is None else int(cand_cap)
    node_cap = max(1, len(k)) if node_cap is None else int(node_cap)
    _check(lib().lzf_host_store_select_ordered(_np_ptr(k), _np_ptr(o), _np_ptr(ln), _np_ptr(e), len(e), _np_ptr(p),
                                               len(p), int(limit), cand_cap, node_cap, _np_ptr(sel), int(cap),
                                               _np_ptr(result)), "lzf_host_store_select_ordered")
    return sel, result


def store_mget_work(n, device):
    """A scratch tensor for one store_mget call over a list of ``n`` entries."""
    import torch
    return torch.empty(int(lib().lzf_gpu_store_mget_work_size(int(n))), dtype=torch.uint8, device=device)


def store_mget(idx, keys, key_off, key_len, store, val_off, val_size, enc, val_len, item_time, item_ttl, now,
               max_val_len, frame, max_response, frame_len, result, last_access=None, work=None, reply_header=True,
               stream=None):
    """MGET over the index list ``idx`` (int32, read as u32; entries past
    enc's length are ignored): dead and expired entries drop out, expired ones
    become ENC_NULL in enc, valid ones get last_access = now, and the reply
    frame of kv_frame is built over the valid entries in list order with the
    element count taken on the device.  item_time (int64) and item_ttl (int32)
    may both be None: nothing expires.  result (4 elements, int64) = found,
    expired, skipped, MGET_*; frame_len (1 element, int64) is 0 unless
    MGET_OK.  No host wait; returns ``work`` (store_mget_work), which must
    outlive the stream's work."""
    n = idx.numel()
    if work is None:
        work = store_mget_work(n, frame.device)
    rc = lib().lzf_gpu_store_mget(_ptr(idx), n, _ptr(keys), _ptr(key_off), _ptr(key_len), _ptr(store), _ptr(val_off),
                                  _ptr(val_size), _ptr(enc), _ptr(val_len), int(enc.numel()), _opt_ptr(item_time),
                                  _opt_ptr(item_ttl), int(now), _opt_ptr(last_access), int(max_val_len),
                                  1 if reply_header else 0, _ptr(frame), int(max_response), _ptr(frame_len),
                                  _ptr(result), _ptr(work), _stream_handle(stream))
    _check(rc, "lzf_gpu_store_mget")
    return work


def store_replies_work(n, device):
    """A scratch tensor for one store_replies call over a list of ``n`` entries."""
    import torch
    return torch.empty(int(lib().lzf_gpu_store_replies_work_size(int(n))), dtype=torch.uint8, device=device)


def store_replies(idx, mode, store, val_off, val_size, enc, val_len, item_time, item_ttl, now, max_val_len, replies,
                  rep_used, rep_off, rep_len, entry_status, result, op_status=None, last_access=None, work=None,
                  stream=None):
    """One reply frame per entry of the index list ``idx`` (int32, read as
    u32), packed into the arena ``replies`` (uint8; its length is the cap) in
    list order: reply k is replies[rep_off[k] : rep_off[k] + rep_len[k]],
    ``[i16 code][u8 encoding][u32 size][bytes]``, LZF items decoded in place.
    REPLY_GET applies the validity rule as store_mget does (op_status None);
    REPLY_VALUE maps op_status (uint8, one ENT_* per entry, as store_minc
    leaves it) to the reply codes and writes neither enc nor last_access.
    rep_used (1 element, int64), rep_off (n, int64), rep_len (n, int32),
    entry_status (n, uint8, ENT_EDECODE for an item that did not decode);
    result (6 elements, int64) = item replies, expired, dead or code replies,
    REPLY_*, bytes needed, decode failures.  On REPLY_TOO_BIG no arena byte is
    written and rep_used is 0.  No host wait; returns ``work``
    (store_replies_work), which must outlive the stream's work."""
    n = idx.numel()
    if work is None:
        work = store_replies_work(n, replies.device)
    rc = lib().lzf_gpu_store_replies(_ptr(idx), n, int(mode), _opt_ptr(op_status), _ptr(store), _ptr(val_off),
                                     _ptr(val_size), _ptr(enc), _ptr(val_len), int(enc.numel()), _opt_ptr(item_time),
                                     _opt_ptr(item_ttl), int(now), _opt_ptr(last_access), int(max_val_len),
                                     _ptr(replies), int(replies.numel()), _ptr(rep_used), _ptr(rep_off),
                                     _ptr(rep_len), _ptr(entry_status), _ptr(result), _ptr(work),
                                     _stream_handle(stream))
    _check(rc, "lzf_gpu_store_replies")
    return work


def reply_code(ent_status):
    """lzf_host_reply_code: the REPL_* code of an ENT_* entry status, the rule
    store_replies applies in REPLY_VALUE mode.  No device call."""
    return int(lib().lzf_host_reply_code(int(ent_status)))


def store_count(idx, enc, item_time, item_ttl, now, result, last_access=None, stream=None):
    """COUNT over an index list: result (2 elements, int64) = valid entries,
    entries this call expired (and nulled in enc); valid entries get
    last_access = now.  MDEL is store_count followed by store_delete over the
    same list.  No host wait."""
    _check(lib().lzf_gpu_store_count(_ptr(idx), int(idx.numel()), _ptr(enc), int(enc.numel()), _opt_ptr(item_time),
                                     _opt_ptr(item_ttl), int(now), _opt_ptr(last_access), _ptr(result),
                                     _stream_handle(stream)), "lzf_gpu_store_count")


def store_mttl(idx, ttl, enc, item_time, item_ttl, now, result, last_access=None, stream=None):
    """MTTL over an index list of distinct entries: a valid entry gets
    item_time = last_access = now and item_ttl = ttl (already clamped to
    maxitemttl); result (2 elements, int64) = entries changed, entries this
    call expired.  No host wait."""
    _check(lib().lzf_gpu_store_mttl(_ptr(idx), int(idx.numel()), int(ttl), _ptr(enc), int(enc.numel()),
                                    _ptr(item_time), _ptr(item_ttl), int(now), _opt_ptr(last_access), _ptr(result),
                                    _stream_handle(stream)), "lzf_gpu_store_mttl")


# ---- the device key index: exact-key lookup and upsert -------------------------

def key_index_bytes(slots):
    """lzf_gpu_key_index_bytes(): the table's size for ``slots`` slots, a power
    of two in [16, 2**31].  A tensor of that many bytes filled with 0xFF is an
    empty table."""
    b = int(lib().lzf_gpu_key_index_bytes(int(slots)))
    if not b:
        raise ValueError(f"key_index_bytes: bad slots {slots}")
    return b


def key_home(key_bytes, slots):
    """lzf_host_key_home(): the home slot of a key; its probe sequence is
    home, home + 1, ... modulo ``slots``.  No GPU."""
    key = bytes(key_bytes)
    h = int(lib().lzf_host_key_home(ctypes.c_char_p(key), len(key), int(slots)))
    if h == 0xFFFFFFFF:
        raise ValueError(f"key_home: bad slots {slots}")
    return h


def _key_index_slots(table):
    return int(table.numel() * table.element_size() // 8)


def key_index_insert(table, used, keys, key_off, key_len, enc, first, n, result, status, stream=None):
    """Upsert of the store's items [first, first + n) into ``table`` (a tensor
    of key_index_bytes(slots) bytes; slots is taken from its size), in request
    order: among equal keys of the batch the highest index stays and the
    others become ENC_NULL, and a live item that held the key before becomes
    ENC_NULL.  used (1 element, int32) counts claimed slots and is zeroed
    with the table; result (4 elements, int64) = mapped, replaced, superseded,
    skipped; status (1 element, int32) = KIDX_OK, or KIDX_FULL with the batch
    refused whole and nothing changed.  keys uint8, key_off int64, key_len
    int32, enc uint8, on one device.  No host wait."""
    rc = lib().lzf_gpu_key_index_insert(_ptr(table), _key_index_slots(table), _ptr(used), _ptr(keys), _ptr(key_off),
                                        _ptr(key_len), _ptr(enc), int(enc.numel()), int(first), int(n), _ptr(result),
                                        _ptr(status), _stream_handle(stream))
    _check(rc, "lzf_gpu_key_index_insert")


def key_index_rebuild(table, used, keys, key_off, key_len, enc, result, status, stream=None):
    """The table and ``used`` cleared on the stream, then every item of
    [0, enc.numel()) inserted as key_index_insert does.  KIDX_FULL is judged
    on the items the insert will not skip (live, with a key), counted on the
    device, so the dead tail a store_renumber leaves costs nothing; on FULL
    the table stays empty, used is 0 and no enc changes.  result and status as
    key_index_insert.  No host wait."""
    rc = lib().lzf_gpu_key_index_rebuild(_ptr(table), _key_index_slots(table), _ptr(used), _ptr(keys), _ptr(key_off),
                                         _ptr(key_len), _ptr(enc), int(enc.numel()), _ptr(result), _ptr(status),
                                         _stream_handle(stream))
    _check(rc, "lzf_gpu_key_index_rebuild")


def key_index_lookup(table, keys, key_off, key_len, enc, qkeys, q_off, q_len, idx, result, stream=None):
    """Lookup of the query keys qkeys / q_off / q_len (as many as q_len has
    entries): idx (int32, read as u32) receives the item index per key, or
    0xFFFFFFFF (-1) for an absent key, a dead item or an empty key -- the
    padding store_mget, store_count, store_delete and store_mttl ignore, so
    idx feeds them as it is.  result (3 elements, int64) = hits, misses, slots
    examined.  No host wait."""
    rc = lib().lzf_gpu_key_index_lookup(_ptr(table), _key_index_slots(table), _ptr(keys), _ptr(key_off), _ptr(key_len),
                                        _ptr(enc), int(enc.numel()), _ptr(qkeys), _ptr(q_off), _ptr(q_len),
                                        int(q_len.numel()), _ptr(idx), _ptr(result), _stream_handle(stream))
    _check(rc, "lzf_gpu_key_index_lookup")


# ---- locks, the lock-aware DEL, INC / DEC over an index list --------------------

def store_mlock(idx, lock_time, enc, item_time, item_ttl, item_lock, now, result, last_access=None,
                entry_status=None, stream=None):
    """LOCK / MLOCK over an index list of distinct entries: an entry that is
    valid and not locked (item_lock == -1, or now - item_time < item_lock)
    gets item_time = last_access = now and item_lock = lock_time; an expired
    one becomes ENC_NULL.  item_time / item_lock int64, item_ttl int32;
    entry_status (uint8, one ENT_* per entry) is optional; result (3 elements,
    int64) = locked by this call, expired, refused as locked.  No host wait."""
    _check(lib().lzf_gpu_store_mlock(_ptr(idx), int(idx.numel()), int(lock_time), _ptr(enc), int(enc.numel()),
                                     _ptr(item_time), _ptr(item_ttl), _ptr(item_lock), int(now),
                                     _opt_ptr(last_access), _opt_ptr(entry_status), _ptr(result),
                                     _stream_handle(stream)), "lzf_gpu_store_mlock")


def store_munlock(idx, enc, item_time, item_ttl, item_lock, now, result, last_access=None, entry_status=None,
                  stream=None):
    """UNLOCK / MUNLOCK over an index list: a valid entry gets item_lock = 0
    and last_access = now, locked or not; result (2 elements, int64) = found,
    expired.  No host wait."""
    _check(lib().lzf_gpu_store_munlock(_ptr(idx), int(idx.numel()), _ptr(enc), int(enc.numel()), _ptr(item_time),
                                       _ptr(item_ttl), _ptr(item_lock), int(now), _opt_ptr(last_access),
                                       _opt_ptr(entry_status), _ptr(result), _stream_handle(stream)),
           "lzf_gpu_store_munlock")


def store_mdel(idx, enc, item_time, item_ttl, item_lock, now, result, entry_status=None, stream=None):
    """The lock-aware DEL / MDEL over an index list, in one launch: a locked
    entry is left alone (the lock is tested first, on an expired item too), an
    expired one becomes ENC_NULL uncounted, a valid one becomes ENC_NULL.
    item_time / item_ttl may both be None, item_lock may be None; result (3
    elements, int64) = deleted, expired, locked.  No host wait."""
    _check(lib().lzf_gpu_store_mdel(_ptr(idx), int(idx.numel()), _ptr(enc), int(enc.numel()), _opt_ptr(item_time),
                                    _opt_ptr(item_ttl), _opt_ptr(item_lock), int(now), _opt_ptr(entry_status),
                                    _ptr(result), _stream_handle(stream)), "lzf_gpu_store_mdel")


def store_minc_work(n, device):
    """A scratch tensor for one store_minc call over a list of ``n`` entries."""
    import torch
    return torch.empty(int(lib().lzf_gpu_store_minc_work_size(int(n))), dtype=torch.uint8, device=device)


def store_minc(idx, delta, store, store_used, val_off, val_size, enc, item_time, item_ttl, item_lock, now, result,
               status, single=False, last_access=None, entry_status=None, entry_value=None, work=None, stream=None):
    """INC / DEC / MINC / MDEC over an index list of distinct entries: a NUMBER
    item's 8 stored bytes become value + delta; a PLAIN item whose bytes parse
    (parse_long) becomes a NUMBER item in a fresh 8-byte slot appended to
    ``store`` in list order from ``store_used[0]`` on, which is advanced; an
    LZF item is counted and left (``single``: not a number).  Locked entries
    are left alone, expired ones become ENC_NULL.  The cap is the store
    tensor's length.  item_time / item_ttl may both be None, item_lock may be
    None.  result (6 elements, int64) = found, expired, locked, nan,
    converted, unchanged; status (1 element, int32) = STORE_OK, or STORE_FULL
    with nothing changed and result zero; entry_status (uint8) and entry_value
    (int64, the new numbers) are optional.  No host wait; returns ``work``
    (store_minc_work), which must outlive the stream's work."""
    n = idx.numel()
    if work is None:
        work = store_minc_work(n, store.device)
    rc = lib().lzf_gpu_store_minc(_ptr(idx), n, int(delta), 1 if single else 0, _ptr(store), int(store.numel()),
                                  _ptr(store_used), _ptr(val_off), _ptr(val_size), _ptr(enc), int(enc.numel()),
                                  _opt_ptr(item_time), _opt_ptr(item_ttl), _opt_ptr(item_lock), int(now),
                                  _opt_ptr(last_access), _opt_ptr(entry_status), _opt_ptr(entry_value), _ptr(result),
                                  _ptr(status), _ptr(work), _stream_handle(stream))
    _check(rc, "lzf_gpu_store_minc")
    return work


def parse_long(value):
    """lzf_host_parse_long(): gbQueryParseLong (src/query.c:39-76) over a bytes
    value -- the number, or None when the value is not one.  No GPU."""
    value = bytes(value)
    out = ctypes.c_int64(0)
    ok = lib().lzf_host_parse_long(ctypes.c_char_p(value), len(value), ctypes.byref(out))
    return int(out.value) if ok else None


def store_set_guard(occ, first, enc, item_time, item_lock, now, result, refused=None, stream=None):
    """SET on a locked key, between key_index_lookup of a batch's own keys
    (``occ``, int32 read as u32, one entry per new item from ``first`` on) and
    its key_index_insert: a new item whose key is held by a live, locked item
    outside the batch becomes ENC_NULL, so the insert skips it.  refused
    (uint8, optional) = 1 per refused item; result (1 element, int64) = how
    many.  No host wait."""
    _check(lib().lzf_gpu_store_set_guard(_ptr(occ), int(first), int(occ.numel()), _ptr(enc), int(enc.numel()),
                                         _ptr(item_time), _ptr(item_lock), int(now), _opt_ptr(refused), _ptr(result),
                                         _stream_handle(stream)), "lzf_gpu_store_set_guard")


# ---- request ingest: raw requests in, descriptors out ------------------------------

class ParsedRequests:
    """The seven output arrays of request_parse, n entries each: op and status
    uint8, key_off / val_off int64 (absolute into the request arena), key_len /
    val_len int32, num int64.  Tensors on one device, or numpy arrays from
    host_request_parse."""
    FIELDS = ("op", "status", "key_off", "key_len", "val_off", "val_len", "num")

    def __init__(self, op, status, key_off, key_len, val_off, val_len, num):
        self.op, self.status, self.key_off, self.key_len = op, status, key_off, key_len
        self.val_off, self.val_len, self.num = val_off, val_len, num

    @classmethod
    def empty(cls, n, device):
        import torch
        dt = {"op": torch.uint8, "status": torch.uint8, "key_len": torch.int32, "val_len": torch.int32}
        return cls(*(torch.empty(n, dtype=dt.get(f, torch.int64), device=device) for f in cls.FIELDS))


def request_parse(req, req_off, req_len, max_key, max_value, out, result, expect_op=0, stream=None):
    """The reference's request grammar over a batch: request k is
    ``req[req_off[k] : req_off[k] + req_len[k]]`` (req uint8, req_off int64,
    req_len int32 read as u32), ``[i16 opcode][payload]``.  ``out`` (a
    ParsedRequests) receives the opcode, a REQ_* status, the key and value
    spans with offsets absolute into ``req`` and the number; result
    (REQ_NSTATUS elements, int64) how many requests got each status.  With
    ``expect_op`` every other opcode is REQ_OTHER.  No byte outside ``req`` is
    read.  No host wait."""
    rc = lib().lzf_gpu_request_parse(_ptr(req), int(req.numel()), _ptr(req_off), _ptr(req_len), int(req_len.numel()),
                                     int(max_key), int(max_value), int(expect_op), _ptr(out.op), _ptr(out.status),
                                     _ptr(out.key_off), _ptr(out.key_len), _ptr(out.val_off), _ptr(out.val_len),
                                     _ptr(out.num), _ptr(result), _stream_handle(stream))
    _check(rc, "lzf_gpu_request_parse")
    return out


def host_request_parse(req, req_off, req_len, max_key, max_value, expect_op=0):
    """request_parse on the host over numpy arrays (req uint8, req_off uint64,
    req_len uint32), the same function in a loop: (ParsedRequests of numpy
    arrays, result as a numpy uint64 array).  No GPU."""
    import numpy as np
    req = np.ascontiguousarray(req, dtype=np.uint8)
    req_off = np.ascontiguousarray(req_off, dtype=np.uint64)
    req_len = np.ascontiguousarray(req_len, dtype=np.uint32)
    n = len(req_len)
    dt = {"op": np.uint8, "status": np.uint8, "key_off": np.uint64, "key_len": np.uint32, "val_off": np.uint64,
          "val_len": np.uint32, "num": np.int64}
    out = ParsedRequests(*(np.zeros(n, dtype=dt[f]) for f in ParsedRequests.FIELDS))
    result = np.zeros(REQ_NSTATUS, dtype=np.uint64)
    base = ctypes.c_void_p(req.ctypes.data if len(req) else ctypes.addressof(ctypes.create_string_buffer(1)))
    rc = lib().lzf_host_request_parse(base, len(req), _np_ptr(req_off), _np_ptr(req_len), n, int(max_key),
                                      int(max_value), int(expect_op), _np_ptr(out.op), _np_ptr(out.status),
                                      _np_ptr(out.key_off), _np_ptr(out.key_len), _np_ptr(out.val_off),
                                      _np_ptr(out.val_len), _np_ptr(out.num), _np_ptr(result))
    _check(rc, "lzf_host_request_parse")
    return out, result


def request_reply_code(status):
    """lzf_host_request_reply_code: -1 for REQ_OK (the operator replies), -2
    for REQ_BADOP (close the connection), REPL_ERR_NAN for REQ_NAN, REPL_ERR
    otherwise.  No device call."""
    return int(lib().lzf_host_request_reply_code(int(status)))


def store_append_keys_work(n, device):
    """A scratch tensor for one store_append_keys call over ``n`` requests."""
    import torch
    return torch.empty(int(lib().lzf_gpu_store_append_keys_work_size(int(n))), dtype=torch.uint8, device=device)


def store_append_keys(req, parsed, keys, keys_used, key_off, key_len, first, now, max_item_ttl, set_len, void_idx,
                      result, item_time=None, item_ttl=None, item_lock=None, last_access=None, work=None, stream=None):
    """SET's other half, after request_parse left ``parsed`` over ``req``: item
    ``first + k`` belongs to request k.  An accepted request (OP_SET, REQ_OK,
    its key inside ``req``) has its key appended to ``keys`` from
    ``keys_used[0]`` on, which is advanced, key_off / key_len of its item
    written, item_time = last_access = now, item_lock = 0, item_ttl = num > 0 ?
    min(max_item_ttl, num) : -1, set_len[k] = its value's length and
    void_idx[k] = -1; a refused one gets key_len 0, set_len 0 and void_idx[k] =
    first + k, for store_delete after set_store.  key_off .. last_access are
    the store's arrays (count = key_len's length); set_len and void_idx int32,
    one per request; result (4 elements, int64) = accepted, refused, key bytes,
    STORE_OK or STORE_FULL (the call refused whole, nothing appended).  No host
    wait; returns ``work`` (store_append_keys_work), which must outlive the
    stream's work."""
    n = parsed.status.numel()
    if work is None:
        work = store_append_keys_work(n, keys.device)
    rc = lib().lzf_gpu_store_append_keys(_ptr(req), int(req.numel()), _ptr(parsed.op), _ptr(parsed.status),
                                         _ptr(parsed.key_off), _ptr(parsed.key_len), _ptr(parsed.val_len),
                                         _ptr(parsed.num), n, _ptr(keys), int(keys.numel()), _ptr(keys_used),
                                         _ptr(key_off), _ptr(key_len), _opt_ptr(item_time), _opt_ptr(item_ttl),
                                         _opt_ptr(item_lock), _opt_ptr(last_access), int(first), int(key_len.numel()),
                                         int(now), int(max_item_ttl), _ptr(set_len), _ptr(void_idx), _ptr(result),
                                         _ptr(work), _stream_handle(stream))
    _check(rc, "lzf_gpu_store_append_keys")
    return work


# ---- request dispatch: bucket a mixed batch by operator, stitch the replies ----------

def request_class(op, status):
    """lzf_host_request_class: 0 for a refused request (every status but
    REQ_OK and REQ_NAN), the operator 1 .. 21 itself, RQ_NCLASS - 1 for OP_END.
    No device call."""
    return int(lib().lzf_host_request_class(int(op), int(status)))


class BucketedRequests:
    """What request_bucket makes of a ParsedRequests of n entries: perm and
    slot (int32 read as u32, n each; perm[slot[k]] == k), class_first
    (RQ_NCLASS + 1, int32) and ``b``, a ParsedRequests in bucket order.  Class
    c is the slice ``class_slice(c, first)`` of perm and of every array of
    ``b``, ``first`` being class_first copied to the host.  Tensors on one
    device, or numpy arrays from host_request_bucket."""

    def __init__(self, perm, slot, class_first, b):
        self.perm, self.slot, self.class_first, self.b = perm, slot, class_first, b

    @classmethod
    def empty(cls, n, device):
        import torch
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=device)
        return cls(i32(n), i32(n), i32(RQ_NCLASS + 1), ParsedRequests.empty(n, device))

    @staticmethod
    def class_slice(c, first):
        return slice(int(first[c]), int(first[c + 1]))


def request_bucket_work(n, device):
    """A scratch tensor for one request_bucket call over ``n`` requests."""
    import torch
    return torch.empty(int(lib().lzf_gpu_request_bucket_work_size(int(n))), dtype=torch.uint8, device=device)


def request_bucket(parsed, out, work=None, stream=None):
    """The stable partition of a parsed batch by operator class
    (request_class): ``out`` (a BucketedRequests) receives perm, slot,
    class_first and the seven arrays in bucket order, whose class slices feed
    key_index_lookup, store_append_keys and set_store as they are.  No host
    wait; the caller copies class_first (96 bytes) to size its per-class
    calls.  Returns ``work`` (request_bucket_work), which must outlive the
    stream's work."""
    n = parsed.status.numel()
    if work is None:
        work = request_bucket_work(n, parsed.status.device)
    b = out.b
    rc = lib().lzf_gpu_request_bucket(_ptr(parsed.op), _ptr(parsed.status), _ptr(parsed.key_off), _ptr(parsed.key_len),
                                      _ptr(parsed.val_off), _ptr(parsed.val_len), _ptr(parsed.num), n, _ptr(out.perm),
                                      _ptr(out.slot), _ptr(out.class_first), _ptr(b.op), _ptr(b.status),
                                      _ptr(b.key_off), _ptr(b.key_len), _ptr(b.val_off), _ptr(b.val_len), _ptr(b.num),
                                      _ptr(work), _stream_handle(stream))
    _check(rc, "lzf_gpu_request_bucket")
    return work


_PARSED_NP = (("op", "uint8"), ("status", "uint8"), ("key_off", "uint64"), ("key_len", "uint32"),
              ("val_off", "uint64"), ("val_len", "uint32"), ("num", "int64"))


def host_request_bucket(parsed):
    """request_bucket on the host over a ParsedRequests of numpy arrays (a
    counting sort): a BucketedRequests of numpy arrays, perm / slot /
    class_first uint32.  No GPU."""
    import numpy as np
    src = [np.ascontiguousarray(getattr(parsed, f), dtype=dt) for f, dt in _PARSED_NP]
    n = len(src[0])
    out = BucketedRequests(np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(RQ_NCLASS + 1, np.uint32),
                           ParsedRequests(*(np.zeros(n, dtype=dt) for _, dt in _PARSED_NP)))
    rc = lib().lzf_host_request_bucket(*(_np_ptr(a) for a in src), n, _np_ptr(out.perm), _np_ptr(out.slot),
                                       _np_ptr(out.class_first), *(_np_ptr(getattr(out.b, f)) for f, _ in _PARSED_NP))
    _check(rc, "lzf_host_request_bucket")
    return out


def _stitch_tables(class_mode, class_base):
    if len(class_mode) != RQ_NCLASS or len(class_base) != RQ_NCLASS:
        raise ValueError("class_mode and class_base have RQ_NCLASS entries")
    return ((ctypes.c_uint8 * RQ_NCLASS)(*(int(m) for m in class_mode)),
            (ctypes.c_uint64 * RQ_NCLASS)(*(int(b) for b in class_base)))


def request_stitch(op, status, slot, class_first, class_mode, class_base, replies, code_base, out_off, out_len,
                   out_kind, result, b_rep_off=None, b_rep_len=None, b_ent=None, b_refused=None, stream=None):
    """The reply table of a bucketed batch in request order, the overrides made
    on the device: request k gets out_off[k] (int64, absolute into ``replies``),
    out_len[k] (int32) and out_kind[k] (uint8: OUT_REPLY, OUT_CLOSE, OUT_HOST)
    by the seven rules of include/lzf_gpu.h.  class_mode (STITCH_*) and
    class_base are host sequences of RQ_NCLASS entries; b_rep_off / b_rep_len
    (what store_replies wrote, at each ARENA class's slice), b_ent (ENT_*, at
    each CODE class's slice) and b_refused (store_set_guard's, at the SET
    slice) are in bucket order.  The 64 bytes of ``replies`` at code_base
    receive the code frames.  result (5 elements, int64) = arena replies, code
    replies, closes, host, bad slices.  No reply byte is copied.  No host wait."""
    mode, base = _stitch_tables(class_mode, class_base)
    rc = lib().lzf_gpu_request_stitch(_ptr(op), _ptr(status), _ptr(slot), int(status.numel()), _ptr(class_first),
                                      mode, base, _opt_ptr(b_rep_off), _opt_ptr(b_rep_len), _opt_ptr(b_ent),
                                      _opt_ptr(b_refused), _ptr(replies), int(replies.numel()), int(code_base),
                                      _ptr(out_off), _ptr(out_len), _ptr(out_kind), _ptr(result),
                                      _stream_handle(stream))
    _check(rc, "lzf_gpu_request_stitch")


def host_request_stitch(op, status, slot, class_first, class_mode, class_base, replies, code_base, b_rep_off=None,
                        b_rep_len=None, b_ent=None, b_refused=None):
    """request_stitch on the host over numpy arrays (``replies`` a writable
    uint8 array, which receives the code frames): (out_off uint64, out_len
    uint32, out_kind uint8, result uint64).  No GPU."""
    import numpy as np
    mode, base = _stitch_tables(class_mode, class_base)
    arr = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
    op, status, slot = arr(op, np.uint8), arr(status, np.uint8), arr(slot, np.uint32)
    class_first = arr(class_first, np.uint32)
    b_rep_off, b_rep_len = arr(b_rep_off, np.uint64), arr(b_rep_len, np.uint32)
    b_ent, b_refused = arr(b_ent, np.uint8), arr(b_refused, np.uint8)
    n = len(status)
    out_off, out_len, out_kind = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    result = np.zeros(5, np.uint64)
    opt = lambda a: ctypes.c_void_p(0) if a is None else _np_ptr(a)
    rc = lib().lzf_host_request_stitch(_np_ptr(op), _np_ptr(status), _np_ptr(slot), n, _np_ptr(class_first), mode, base,
                                       opt(b_rep_off), opt(b_rep_len), opt(b_ent), opt(b_refused), _np_ptr(replies),
                                       len(replies), int(code_base), _np_ptr(out_off), _np_ptr(out_len),
                                       _np_ptr(out_kind), _np_ptr(result))
    _check(rc, "lzf_host_request_stitch")
    return out_off, out_len, out_kind, result


# ---- MSET by prefix, the memory sweep, META and the KEYS frame --------------------

def store_mset_work(n, vlen, device):
    """A scratch tensor for one store_mset call of a ``vlen``-byte value over a
    list of ``n`` entries."""
    import torch
    return torch.empty(int(lib().lzf_gpu_store_mset_work_size(int(n), int(vlen))), dtype=torch.uint8, device=device)


def store_mset(idx, value, compression, store, store_used, val_off, val_size, enc, val_len, item_time, item_ttl,
               item_lock, now, result, status, last_access=None, entry_status=None, work=None, stream=None):
    """MSET over an index list of distinct entries: every entry that is valid
    and not locked (the lock is tested first, on an expired item too) gets the
    new ``value`` (a uint8 tensor on the device, at least one byte).  Its
    stored form is decided once, as set_store decides it for that one value --
    compressed iff its length > ``compression``, kept LZF iff a stream of at
    most length - 4 bytes exists -- and every such entry gets its own copy,
    appended to ``store`` in list order from ``store_used[0]`` on, which is
    advanced; val_off, val_size, enc and val_len are rewritten, item_time =
    last_access = now, item_ttl = -1, item_lock = 0.  Expired entries become
    ENC_NULL.  The cap is the store tensor's length; ``value`` must not lie in
    the store's free part.  item_lock may be None.  result (5 elements, int64)
    = set, expired, locked, the stored size, the stored encoding; status (1
    element, int32) = STORE_OK, or STORE_FULL with nothing changed and result
    zero; entry_status (uint8, one ENT_* per entry) is optional.  No host wait;
    returns ``work`` (store_mset_work), which must outlive the stream's work."""
    n, vlen = idx.numel(), value.numel()
    if work is None:
        work = store_mset_work(n, vlen, store.device)
    rc = lib().lzf_gpu_store_mset(_ptr(idx), n, _ptr(value), vlen, int(compression), _ptr(store), int(store.numel()),
                                  _ptr(store_used), _ptr(val_off), _ptr(val_size), _ptr(enc), _ptr(val_len),
                                  int(enc.numel()), _ptr(item_time), _ptr(item_ttl), _opt_ptr(item_lock), int(now),
                                  _opt_ptr(last_access), _opt_ptr(entry_status), _ptr(result), _ptr(status),
                                  _ptr(work), _stream_handle(stream))
    _check(rc, "lzf_gpu_store_mset")
    return work


def store_gc(last_access, now, gc_ratio, enc, val_size, result, gate=None, max_bytes=0, stream=None):
    """The memory sweep over the whole store: a live item with now -
    last_access != 0 and >= ``gc_ratio`` becomes ENC_NULL, whatever its lock
    and TTL.  With ``gate`` (1 element, int64, normally store_used) the sweep
    runs only when gate[0] > ``max_bytes``.  result (3 elements, int64) = items
    freed, their stored bytes, 1 if the sweep ran.  No host wait."""
    _check(lib().lzf_gpu_store_gc(_ptr(last_access), int(now), int(gc_ratio), _ptr(enc), _ptr(val_size),
                                  int(enc.numel()), _opt_ptr(gate), int(max_bytes), _ptr(result),
                                  _stream_handle(stream)), "lzf_gpu_store_gc")


def meta_field(name):
    """lzf_host_meta_field(): the META_* code gbGetItemMeta (src/query.c:
    1255-1300) resolves a field name to, prefixes and over-long names as it
    does, or None.  No GPU."""
    name = bytes(name)
    f = int(lib().lzf_host_meta_field(ctypes.c_char_p(name), len(name)))
    return None if f < 0 else f


def store_meta(idx, field, enc, val_size, item_time, item_ttl, item_lock, now, entry_value, result, last_access=None,
               entry_status=None, stream=None):
    """META over an index list: entry_value (int64, one per entry) receives the
    field (a META_* code) of every valid entry, 0 otherwise; a valid entry then
    gets last_access = now (META_ACCESS reports the value before), an expired
    one becomes ENC_NULL.  item_lock may be None (0), last_access may be None
    except for META_ACCESS.  result (2 elements, int64) = found, expired.  No
    host wait."""
    _check(lib().lzf_gpu_store_meta(_ptr(idx), int(idx.numel()), int(field), _ptr(enc), _ptr(val_size),
                                    int(enc.numel()), _ptr(item_time), _ptr(item_ttl), _opt_ptr(item_lock), int(now),
                                    _opt_ptr(last_access), _opt_ptr(entry_status), _ptr(entry_value), _ptr(result),
                                    _stream_handle(stream)), "lzf_gpu_store_meta")


def store_keys_work(n, device):
    """A scratch tensor for one store_keys call over a list of ``n`` entries."""
    import torch
    return torch.empty(int(lib().lzf_gpu_store_keys_work_size(int(n))), dtype=torch.uint8, device=device)


def store_keys(idx, keys, key_off, key_len, enc, frame, max_response, frame_len, result, work=None,
               reply_header=True, stream=None):
    """The KEYS reply over an index list: the j-th entry that is in range, not
    ENC_NULL and has a key becomes the pair [decimal j -> the item's key, PLAIN]
    of a KVAL frame as kv_frame writes it.  No validity test, nothing nulled.
    result (2 elements, int64) = found, MGET_OK / MGET_NOT_FOUND /
    MGET_TOO_BIG; frame_len (1 element, int64) is 0 unless MGET_OK.  No host
    wait; returns ``work`` (store_keys_work), which must outlive the stream's
    work."""
    n = idx.numel()
    if work is None:
        work = store_keys_work(n, frame.device)
    rc = lib().lzf_gpu_store_keys(_ptr(idx), n, _ptr(keys), _ptr(key_off), _ptr(key_len), _ptr(enc), int(enc.numel()),
                                  1 if reply_header else 0, _ptr(frame), int(max_response), _ptr(frame_len),
                                  _ptr(result), _ptr(work), _stream_handle(stream))
    _check(rc, "lzf_gpu_store_keys")
    return work


def host_register(arr):
    """lzf_host_register over a numpy array's bytes: the host batches whose
    arenas lie in registered ranges move values without CPU copies."""
    _check(lib().lzf_host_register(_np_ptr(arr), arr.nbytes), "lzf_host_register")


def host_unregister(arr):
    _check(lib().lzf_host_unregister(_np_ptr(arr)), "lzf_host_unregister")


def device_plan():
    """[(device, numa_node, bound)] of the host-memory calls (LZF_GPU_DEVICES)."""
    d, n, b = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_int * 64)()
    g = lib().lzf_gpu_device_plan(d, n, b, 64)
    if g < 0:
        raise RuntimeError(f"lzf_gpu_device_plan failed: {_ERRS.get(g, g)}")
    return [(d[k], n[k], bool(b[k])) for k in range(g)]


def host_last_spread():
    """[(values, ms)] per plan entry of this thread's last host-memory call."""
    v, t = (ctypes.c_uint32 * 64)(), (ctypes.c_double * 64)()
    g = lib().lzf_host_last_spread(v, t, 64)
    return [(v[k], t[k]) for k in range(min(g, 64))]


def host_split(count, groups, g):
    """(first, stride, n): the values entry g of ``groups`` takes."""
    f, s = ctypes.c_uint32(), ctypes.c_uint32()
    n = lib().lzf_host_split(count, groups, g, ctypes.byref(f), ctypes.byref(s))
    return f.value, s.value, n


def host_split_block(count, groups, g):
    """(first, n): the contiguous span entry g of ``groups`` takes under
    LZF_GPU_SPLIT=block."""
    f = ctypes.c_uint32()
    n = lib().lzf_host_split_block(count, groups, g, ctypes.byref(f))
    return f.value, n


def host_split_policy():
    """"block" when LZF_GPU_SPLIT=block is in force, else "round-robin"."""
    return "block" if lib().lzf_host_split_policy() == 1 else "round-robin"


def parse_device_list(spec, visible):
    out = (ctypes.c_int * 64)()
    n = lib().lzf_gpu_parse_device_list(spec.encode(), visible, out, 64)
    return list(out[:n]) if n > 0 else n


def kv_frame(keys, key_off, key_len, vals, val_off, val_size, enc, val_len, elements,
             max_val_len, frame, max_response, frame_len, work=None, reply_header=True,
             stream=None):
    """MGET / KEYS reply (src/net.c:1256-1342, header src/net.c:1162-1205)
    built on the device, LZF items decoded in place.  Tensors on one device:
    keys/vals/enc/frame uint8, *_off int64, key_len/val_size/val_len int32,
    frame_len int64 (1 element; 0 = CHECK_SPACE failed or an item did not
    decode to its val_len).  ``work`` defaults to a fresh scratch tensor."""
    import torch
    n = key_len.numel()
    if work is None:
        work = torch.empty(int(lib().lzf_gpu_kv_frame_work_size(n)), dtype=torch.uint8,
                           device=frame.device)
    rc = lib().lzf_gpu_kv_frame(_ptr(keys), _ptr(key_off), _ptr(key_len), _ptr(vals),
                                _ptr(val_off), _ptr(val_size), _ptr(enc), _ptr(val_len), n,
                                int(elements), int(max_val_len), 1 if reply_header else 0,
                                _ptr(frame), int(max_response), _ptr(frame_len), _ptr(work),
                                _stream_handle(stream))
    _check(rc, "lzf_gpu_kv_frame")
