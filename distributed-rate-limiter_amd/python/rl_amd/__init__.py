"""ctypes binding of librl_engine.so (include/rl_engine.h) for tests and bench.py.

This is plumbing around the C-ABI: every decision is made by the HIP kernels in
librl_engine.so. There is no CPU fallback — if the library is missing or no GPU is
present, constructing an Engine raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPO = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("RL_ENGINE_LIB") or os.path.join(PKG_DIR, "librl_engine.so")  # A/B builds only
HEADER = os.path.join(REPO, "include", "rl_engine.h")

RL_OK = 0
RL_E_INVALID_ARG = -1
RL_E_INVALID_REQUEST = -2
RL_E_CAPACITY = -3
RL_E_DEVICE = -4
RL_E_NOMEM = -5
RL_E_TOO_LARGE = -6
RL_E_LIMITERS = -7
RL_E_INTERNAL = -8      # engine logic error (include/rl_engine.h)

SW, TB = 0, 1
OP_ACQUIRE, OP_PEEK, OP_RESET = 0, 1, 2
REM_UNKNOWN, REM_INVALID, REM_ERROR = -1, -2, -3
RETRY_NEVER, RETRY_INVALID = -1, -2   # RL_RETRY_* (rl_retry_after)
RETRY_ERROR = -3                      # RL_RETRY_ERROR (rl_router_retry_after: the owner's call failed)
QUOTA_INVALID = -2                    # RL_QUOTA_INVALID (rl_quota: every output of an invalid query)
TOP_KEYS_MAX, TOP_KEYS_CANDIDATES = 4096, 65536   # RL_TOP_KEYS_* (rl_top_keys)
TALLY_ROWS, TALLY_UNKNOWN, TALLY_ACCUMULATE = 256, 255, 1   # RL_TALLY_* (rl_tally_batch)
USAGE_BINS, USAGE_CANDIDATES = 16, 65536   # RL_USAGE_* (rl_limiter_usage, rl_top_consumers)
MOVE_KEYS_MAX = 8192                       # RL_MOVE_KEYS_MAX: keys per rl_copy_keys / rl_drop_keys
DIGEST_CACHE = 1                           # RL_DIGEST_CACHE: also digest the rejecting local-cache entries
# RL_DIGEST_K_SW / _K_TB / _K_CACHE and RL_DIGEST_C1 / _C2 (include/rl_engine.h): the entry hash
DIGEST_K = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9)
DIGEST_C1, DIGEST_C2 = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53
KEY_MAX_BYTES = 4096                       # RL_KEY_MAX_BYTES: longest key of a string-key batch
SNAPSHOT_MIN_CAP = 256                     # RL_SNAPSHOT_MIN_CAP: a snapshot cap that always makes progress
CHECK_CLASSES = 16                         # RL_CHECK_CLASSES: class ids of a table check (RL_CHECK_*)
(CHECK_WRONG_REGION, CHECK_UNREACHABLE, CHECK_DUPLICATE, CHECK_DEAD_MARK, CHECK_SW_START,
 CHECK_SW_COUNT, CHECK_SW_OFFSET, CHECK_TB_FLAGS, CHECK_TB_TOKENS, CHECK_IMAGE_LIMITER,
 CHECK_IMAGE_RESERVED) = range(11)         # (SW_COUNT, TB_TOKENS: reserved, never reported)
CHECK_NONE = 0xFFFFFFFFFFFFFFFF            # rl_check_report.first: no such slot
DEAD_MARK = 2                              # kDeadMark in csrc/rl_device.hpp
SHRINK_FILL_MAX, SHRINK_LEVELS = 104, 24   # RL_SHRINK_* (rl_shrink_plan, rl_shrink_limiter)
PUT_REJECT_ORDER, PUT_REJECT_LIMITER = 1, 2   # `rejected` bits of rl_put_keys_device's header
OPT_STAGE_TIMING = 1
OPT_PIPELINE = 2       # RL_OPT_PIPELINE: partition of batch k+1 overlaps batch k's decisions
OPT_FIXED_CAPACITY = 4  # RL_OPT_FIXED_CAPACITY: no on-demand table growth
REGION_SLOTS = 256          # kRegionSlots in csrc/rl_device.hpp (state slots per region)
MIN_REGIONS = 8             # kRegionsPerBin: every limiter has at least one bin of regions
DIST_UNIFORM, DIST_ZIPF = 0, 1
SMALL_BATCH_MAX = 1024      # RL_SMALL_BATCH_MAX

EXPORTS = [
    "rl_create", "rl_destroy", "rl_add_limiter", "rl_add_limiter_ex", "rl_try_acquire_batch",
    "rl_execute_batch", "rl_execute_batch_device", "rl_last_status", "rl_available", "rl_reset",
    "rl_batch_stats_get", "rl_stage_times", "rl_sync", "rl_strerror", "rl_abi_version",
    "rl_owner_of", "rl_route_partition", "rl_synth_trace_device", "rl_tune",
    "rl_route_pack", "rl_route_fold", "rl_route_unpack", "rl_debug_fetch",
    "rl_route_pack_wire", "rl_route_unwire", "rl_result_width", "rl_route_fold_packed",
    "rl_route_unpack_packed", "rl_export_state", "rl_import_state",
    "rl_sweep_expired", "rl_route_return_bytes", "rl_route_fold_return",
    "rl_route_unpack_return", "rl_route_partition_device", "rl_set_owner_directory",
    "rl_owner_of_engine", "rl_router_create", "rl_router_step", "rl_router_finish",
    "rl_router_plan_directory", "rl_router_destroy", "rl_pin_host", "rl_unpin_host",
    "rl_grow_limiter", "rl_limiter_slots", "rl_router_create_ex", "rl_router_stats_get",
    "rl_retry_after", "rl_retry_after_device", "rl_quota", "rl_quota_device",
    "rl_top_keys", "rl_top_keys_device", "rl_router_plan_directory_sampled",
    "rl_limiter_usage", "rl_top_consumers",
    "rl_limiter_digest", "rl_limiter_digest_device",
    "rl_copy_keys", "rl_drop_keys", "rl_put_keys",
    "rl_router_replan_directory", "rl_router_replan_directory_sampled",
    "rl_snapshot_keys", "rl_snapshot_keys_device", "rl_put_keys_device", "rl_restore_keys",
    "rl_shrink_plan", "rl_shrink_limiter",
    "rl_router_execute", "rl_router_retry_after", "rl_route_partition_skip_device",
    "rl_route_fold_ops", "rl_route_unfold_ops", "rl_route_unpack_wait",
    "rl_key_hash", "rl_hash_keys", "rl_hash_keys_device", "rl_execute_batch_keys",
    "rl_tally_batch", "rl_tally_batch_device", "rl_top_denied", "rl_top_denied_device",
    "rl_check_limiter", "rl_check_limiter_device", "rl_check_table_device", "rl_check_images",
    "rl_check_images_device", "rl_debug_alloc_fill", "rl_small_batches",
]
RCCL_EXPORTS = ["rl_rccl_unique_id", "rl_transport_rccl_create", "rl_transport_rccl_destroy"]
STATE_SW_BUCKET, STATE_TB_BUCKET = 0, 1
# rl_state_entry (include/rl_engine.h): one live Redis key ("rl:<key>:<W>" / "tb:<key>")
STATE_DTYPE = np.dtype([("key_hash", "<u8"), ("limiter", "<u2"), ("kind", "u1"),
                        ("reserved", "u1", (5,)), ("window_start_ms", "<i8"), ("count", "<i8"),
                        ("tokens", "<f8"), ("last_refill_ms", "<i8"), ("expire_at_ms", "<i8")])
assert STATE_DTYPE.itemsize == 56


class RlError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        super().__init__(f"{where}: {strerror(status)} ({status})")


class Opts(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("max_batch", ctypes.c_uint64), ("default_capacity", ctypes.c_uint64),
                ("shard_index", ctypes.c_uint32), ("shard_count", ctypes.c_uint32),
                ("max_skew_ms", ctypes.c_int64)]


LIM_LOCAL_CACHE = 1


class LimiterConfig(ctypes.Structure):
    _fields_ = [("algo", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("max_permits", ctypes.c_int64), ("window_ms", ctypes.c_int64),
                ("refill_per_s", ctypes.c_double), ("capacity", ctypes.c_uint64),
                ("local_cache_ttl_ms", ctypes.c_int64)]


class BatchStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("n", "allowed", "distinct_keys", "invalid",
                                                 "capacity_errors", "regions_touched",
                                                 "table_bytes", "cache_hits", "table_grows",
                                                 "hot_regions", "routed")]


class Usage(ctypes.Structure):
    """rl_usage (include/rl_engine.h): census of one limiter's table at one instant."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("slots", "used_slots", "live_keys", "redis_keys",
                                                 "exhausted_keys", "cache_blocked",
                                                 "used_permits")] + \
               [("hist", ctypes.c_uint64 * USAGE_BINS)]


class LimiterTally(ctypes.Structure):
    """rl_limiter_tally (include/rl_engine.h): one limiter's counts of a finished batch."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("requests", "invalid", "errors", "allowed", "denied",
                                                 "over_max", "peeks", "resets", "permits_allowed",
                                                 "permits_denied")] + \
               [("reserved", ctypes.c_uint64 * 2)]


TALLY_DTYPE = np.dtype([(n, "<u8") for n, _ in LimiterTally._fields_[:10]] + [("reserved", "<u8", (2,))])
assert TALLY_DTYPE.itemsize == ctypes.sizeof(LimiterTally) == 96


class BucketDigest(ctypes.Structure):
    """rl_bucket_digest (include/rl_engine.h): count, wrapping sum and xor of one bucket's entry
    hashes."""
    _fields_ = [("entries", ctypes.c_uint64), ("sum", ctypes.c_uint64), ("xr", ctypes.c_uint64)]


DIGEST_DTYPE = np.dtype([("entries", "<u8"), ("sum", "<u8"), ("xr", "<u8")])
assert DIGEST_DTYPE.itemsize == ctypes.sizeof(BucketDigest) == 24


class ShrinkReport(ctypes.Structure):
    """rl_shrink_report (include/rl_engine.h): the plan of a table shrink."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("slots_before", "slots_after", "used_before", "kept")] + \
               [("halvings", ctypes.c_uint32), ("levels", ctypes.c_uint32),
                ("fullest", ctypes.c_uint32 * SHRINK_LEVELS)]


class CheckReport(ctypes.Structure):
    """rl_check_report (include/rl_engine.h): what a table check found."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("regions", "slots", "used_slots", "state_slots",
                                                 "tombstones", "cache_words", "bad_slots")] + \
               [("violations", ctypes.c_uint64 * CHECK_CLASSES), ("first", ctypes.c_uint64 * CHECK_CLASSES)]


CHECK_WORDS = 7 + 2 * CHECK_CLASSES
assert ctypes.sizeof(CheckReport) == 8 * CHECK_WORDS == 312


def check_dict(r) -> dict:
    """A CheckReport, or its CHECK_WORDS 64-bit words (a device report copied back), as a dict;
    `violations` and `first` as lists of CHECK_CLASSES values (first: CHECK_NONE = none)."""
    if not isinstance(r, CheckReport):
        w = np.ascontiguousarray(np.asarray(r).reshape(-1).view(np.uint64))
        assert w.shape[0] == CHECK_WORDS
        r = CheckReport.from_buffer_copy(w.tobytes())
    d = {f: getattr(r, f) for f, _ in CheckReport._fields_[:7]}
    d["violations"] = list(r.violations)
    d["first"] = list(r.first)
    return d


class KeyImage(ctypes.Structure):
    """rl_key_image (include/rl_engine.h): one key's slot words and local-cache word as stored;
    opaque except key_hash / limiter."""
    _fields_ = [("key_hash", ctypes.c_uint64), ("word", ctypes.c_uint64 * 3),
                ("cache_word", ctypes.c_uint64), ("limiter", ctypes.c_uint16),
                ("reserved", ctypes.c_uint16 * 3)]


KEY_IMAGE_DTYPE = np.dtype([("key_hash", "<u8"), ("word", "<u8", (3,)), ("cache_word", "<u8"),
                            ("limiter", "<u2"), ("reserved", "<u2", (3,))])
assert KEY_IMAGE_DTYPE.itemsize == ctypes.sizeof(KeyImage) == 48


class TraceSpec(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("n_keys", ctypes.c_uint64), ("dist", ctypes.c_int32),
                ("permits_max", ctypes.c_int32), ("zipf_s", ctypes.c_double),
                ("t0_ns", ctypes.c_int64), ("span_ns", ctypes.c_int64),
                ("index_base", ctypes.c_uint64), ("n_total", ctypes.c_uint64),
                ("n_limiters", ctypes.c_uint16), ("reserved", ctypes.c_uint16 * 3)]


_lib = None


def build(force: bool = False) -> str:
    """Compile librl_engine.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", PKG_DIR, "clean"])
    subprocess.check_call(["make", "-s", "-j8", "-C", PKG_DIR])    # make skips up-to-date targets
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    # torch (ROCm) ships its own libamdhip64.so.7; the engine links the same soname. Load
    # torch first so both share ONE HIP runtime in this process (device pointers from torch
    # tensors are then valid for the engine and torch can still initialise afterwards).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `make -C {PKG_DIR}` (no CPU fallback)")
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, u16, u32, i32, i64, dbl = (ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint16,
                                       ctypes.c_uint32, ctypes.c_int32, ctypes.c_int64,
                                       ctypes.c_double)
    L.rl_create.argtypes = [ctypes.POINTER(Opts), ctypes.POINTER(vp)]
    L.rl_destroy.argtypes = [vp]
    L.rl_destroy.restype = None
    L.rl_add_limiter.argtypes = [vp, ctypes.c_int, i64, i64, dbl, ctypes.POINTER(u16)]
    L.rl_add_limiter_ex.argtypes = [vp, ctypes.POINTER(LimiterConfig), ctypes.POINTER(u16)]
    L.rl_try_acquire_batch.argtypes = [vp, sz] + [vp] * 7
    L.rl_execute_batch.argtypes = [vp, sz] + [vp] * 8
    L.rl_execute_batch_device.argtypes = [vp, sz] + [vp] * 9
    L.rl_last_status.argtypes = [vp]
    L.rl_available.argtypes = [vp, u16, sz, vp, vp, vp]
    L.rl_reset.argtypes = [vp, u16, sz, vp, vp]
    L.rl_batch_stats_get.argtypes = [vp, ctypes.POINTER(BatchStats)]
    L.rl_stage_times.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p),
                                 ctypes.POINTER(ctypes.c_float), ctypes.c_int]
    L.rl_sync.argtypes = [vp]
    L.rl_tune.argtypes = [vp, ctypes.c_char_p, i64]
    if hasattr(L, "rl_small_batches"):               # (an A/B build of an older revision has none)
        L.rl_small_batches.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.rl_strerror.argtypes = [ctypes.c_int]
    L.rl_strerror.restype = ctypes.c_char_p
    L.rl_owner_of.argtypes = [ctypes.c_uint64, u16, u32]
    L.rl_owner_of.restype = u32
    L.rl_route_partition.argtypes = [vp, sz, vp, vp, u32, vp, vp, vp]
    L.rl_route_pack.argtypes = [vp, sz] + [vp] * 10
    L.rl_route_fold.argtypes = [vp, sz] + [vp] * 4
    L.rl_route_unpack.argtypes = [vp, sz] + [vp] * 5
    L.rl_route_pack_wire.argtypes = [vp, sz] + [vp] * 9
    L.rl_route_unwire.argtypes = [vp, sz, vp, u32, vp, vp, vp, vp, vp, vp]
    L.rl_result_width.argtypes = [vp]
    L.rl_route_fold_packed.argtypes = [vp, sz, vp, vp, vp, ctypes.c_int, vp]
    L.rl_route_unpack_packed.argtypes = [vp, sz, vp, vp, ctypes.c_int, vp, vp, vp]
    L.rl_debug_fetch.argtypes = [vp, ctypes.c_char_p, vp, sz]
    L.rl_synth_trace_device.argtypes = [vp, ctypes.POINTER(TraceSpec), sz, vp, vp, vp, vp, vp]
    L.rl_export_state.argtypes = [vp, i64, vp, sz, ctypes.POINTER(sz)]
    L.rl_import_state.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
    L.rl_sweep_expired.argtypes = [vp, i64, ctypes.POINTER(ctypes.c_uint64)]
    L.rl_route_return_bytes.argtypes = [u32, vp, ctypes.c_int, u32]
    L.rl_route_return_bytes.restype = ctypes.c_uint64
    L.rl_route_fold_return.argtypes = [vp, sz, vp, vp, vp, ctypes.c_int, u32, vp, u32, vp]
    L.rl_route_unpack_return.argtypes = [vp, sz, vp, vp, ctypes.c_int, u32, vp, u32, vp, vp, vp, vp]
    L.rl_route_partition_device.argtypes = [vp, sz, vp, u32, vp, vp, sz, vp]
    L.rl_set_owner_directory.argtypes = [vp, sz, vp, vp]
    L.rl_owner_of_engine.argtypes = [vp, ctypes.c_uint64]
    L.rl_pin_host.argtypes = [vp, vp, sz]
    L.rl_grow_limiter.argtypes = [vp, u16, ctypes.c_uint64]
    L.rl_limiter_slots.argtypes = [vp, u16, ctypes.POINTER(ctypes.c_uint64)]
    L.rl_unpin_host.argtypes = [vp, vp]
    L.rl_retry_after.argtypes = [vp, sz] + [vp] * 6
    L.rl_retry_after_device.argtypes = [vp, sz] + [vp] * 7
    L.rl_quota.argtypes = [vp, sz] + [vp] * 8
    L.rl_quota_device.argtypes = [vp, sz] + [vp] * 9
    L.rl_top_keys.argtypes = [vp, sz, vp, u32, ctypes.c_uint64, vp, vp, ctypes.POINTER(sz),
                              ctypes.POINTER(ctypes.c_uint64)]
    L.rl_top_keys_device.argtypes = [vp, sz, vp, u32, ctypes.c_uint64, vp, vp, vp, vp]
    L.rl_router_plan_directory_sampled.argtypes = [vp, sz, vp, u32, ctypes.c_uint64,
                                                   ctypes.POINTER(u32), vp]
    L.rl_limiter_usage.argtypes = [vp, u16, i64, ctypes.POINTER(Usage)]
    L.rl_top_consumers.argtypes = [vp, u16, i64, u32, i64, vp, vp, ctypes.POINTER(sz),
                                   ctypes.POINTER(ctypes.c_uint64)]
    L.rl_limiter_digest.argtypes = [vp, u16, i64, u32, u32, vp, ctypes.POINTER(BucketDigest)]
    L.rl_limiter_digest_device.argtypes = [vp, u16, i64, u32, u32, vp, vp]
    L.rl_owner_of_engine.restype = u32
    L.rl_copy_keys.argtypes = [vp, sz, vp, vp, sz, ctypes.POINTER(sz)]
    L.rl_drop_keys.argtypes = [vp, sz, vp, ctypes.POINTER(ctypes.c_uint64)]
    L.rl_put_keys.argtypes = [vp, sz, vp, ctypes.POINTER(sz)]
    L.rl_router_replan_directory.argtypes = [vp, sz, vp, vp, ctypes.c_uint64, u32,
                                             ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_uint64), vp]
    L.rl_router_replan_directory_sampled.argtypes = [vp, sz, vp, u32, ctypes.c_uint64,
                                                     ctypes.POINTER(u32),
                                                     ctypes.POINTER(ctypes.c_uint64), vp]
    L.rl_snapshot_keys.argtypes = [vp, u16, ctypes.c_uint64, ctypes.c_uint64, vp, sz,
                                   ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64),
                                   ctypes.POINTER(ctypes.c_uint64)]
    L.rl_snapshot_keys_device.argtypes = [vp, u16, ctypes.c_uint64, ctypes.c_uint64, vp, sz, vp, vp]
    L.rl_put_keys_device.argtypes = [vp, sz, vp, vp, vp]
    L.rl_restore_keys.argtypes = [vp, sz, vp, ctypes.POINTER(sz)]
    L.rl_shrink_plan.argtypes = [vp, u16, i64, ctypes.c_uint64, ctypes.POINTER(ShrinkReport)]
    L.rl_shrink_limiter.argtypes = [vp, u16, i64, ctypes.c_uint64, ctypes.POINTER(ShrinkReport)]
    L.rl_route_partition_skip_device.argtypes = [vp, sz, vp, vp, u32, vp, vp, sz, vp]
    L.rl_route_fold_ops.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.rl_route_unfold_ops.argtypes = [vp, sz, vp, vp, vp, vp]
    L.rl_route_unpack_wait.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp]
    L.rl_router_execute.argtypes = [vp, sz] + [vp] * 8
    L.rl_router_retry_after.argtypes = [vp, sz] + [vp] * 7
    L.rl_key_hash.argtypes = [vp, sz]
    L.rl_key_hash.restype = ctypes.c_uint64
    L.rl_hash_keys_device.argtypes = [vp, sz, vp, sz, vp, vp, vp, vp]
    L.rl_hash_keys.argtypes = [vp, sz, vp, sz, vp, vp]
    L.rl_execute_batch_keys.argtypes = [vp, sz, vp, sz] + [vp] * 9
    L.rl_tally_batch.argtypes = [vp, sz] + [vp] * 6 + [u32]
    L.rl_tally_batch_device.argtypes = [vp, sz] + [vp] * 6 + [u32, vp]
    L.rl_top_denied.argtypes = [vp, sz] + [vp] * 6 + [u16, u32, ctypes.c_uint64, vp, vp, ctypes.POINTER(sz),
                                                      ctypes.POINTER(ctypes.c_uint64),
                                                      ctypes.POINTER(ctypes.c_uint64)]
    L.rl_top_denied_device.argtypes = [vp, sz] + [vp] * 6 + [u16, u32, ctypes.c_uint64, vp, vp, vp, vp]
    L.rl_check_limiter.argtypes = [vp, u16, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(CheckReport)]
    L.rl_check_limiter_device.argtypes = [vp, u16, ctypes.c_uint64, ctypes.c_uint64, vp, vp]
    L.rl_check_table_device.argtypes = [vp, u16, vp, vp, u32, vp, vp]
    L.rl_check_images.argtypes = [vp, sz, vp, ctypes.POINTER(CheckReport)]
    L.rl_check_images_device.argtypes = [vp, sz, vp, vp, vp]
    L.rl_debug_alloc_fill.argtypes = [ctypes.c_int]
    _lib = L
    return L


def strerror(status: int) -> str:
    return lib().rl_strerror(int(status)).decode()


def debug_alloc_fill(byte):
    """Test hook (rl_debug_alloc_fill), process-wide: fill every device allocation the library
    makes from now on with `byte` (0..255) before it is used; None turns the fill off."""
    st = lib().rl_debug_alloc_fill(-1 if byte is None else int(byte))
    if st != RL_OK:
        raise RlError(st, "rl_debug_alloc_fill")


def _p(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data_as(ctypes.c_void_p)
    if hasattr(a, "data_ptr"):          # torch tensor (device memory)
        assert a.is_contiguous()
        return ctypes.c_void_p(a.data_ptr())
    return ctypes.c_void_p(int(a))


def mix64(x):
    """splitmix64 finaliser (the engine's key mixer), numpy uint64 vectorised."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x


def _rotl64(x, r):
    return (x << np.uint64(r)) | (x >> np.uint64(64 - r))


def digest_model(entries, cache_entries, shard_count, bucket_bits):
    """rl_limiter_digest restated in numpy from its definition in include/rl_engine.h, for one
    limiter: `entries` are tuples in PyOracle.keyspace() order (limiter, key_hash, kind,
    window_start, count, tokens, last_refill, expire_at) - the limiter field is ignored -,
    `cache_entries` are (key_hash, x) pairs of the cache words that reject. Returns a
    DIGEST_DTYPE array of 2^bucket_bits buckets. Not used by the engine."""
    entries, cache_entries = list(entries), list(cache_entries)
    n, m = len(entries), len(cache_entries)
    key = np.zeros(n + m, np.uint64)
    kind = np.zeros(n + m, np.int64)
    f = np.zeros((3, n + m), np.uint64)
    u64 = lambda v: int(v) & 0xFFFFFFFFFFFFFFFF  # noqa: E731
    for i, (_, kh, kd, w0, cnt, tok, last, exp) in enumerate(entries):
        key[i], kind[i] = u64(kh), 1 if kd else 0
        if kd:
            f[0, i] = int(np.array([tok], "<f8").view("<u8")[0])
            f[1, i] = u64(last)
        else:
            f[0, i], f[1, i] = u64(w0), u64(cnt)
        f[2, i] = u64(exp)
    for i, (kh, x) in enumerate(cache_entries):
        key[n + i], kind[n + i], f[0, n + i] = u64(kh), 2, u64(x)
    tag = mix64(key)
    with np.errstate(over="ignore"):
        u = tag + np.array(DIGEST_K, np.uint64)[kind]
        u = (u ^ f[0]) * np.uint64(DIGEST_C1)
        u = (u ^ _rotl64(f[1], 23)) * np.uint64(DIGEST_C2)
        u = u ^ _rotl64(f[2], 47)
        h = mix64(u)
    s = int(shard_count).bit_length() - 1 if shard_count > 1 else 0
    g = int(bucket_bits)
    bucket = ((tag << np.uint64(s)) >> np.uint64(64 - g)).astype(np.int64) if g else np.zeros(n + m, np.int64)
    out = np.zeros(1 << g, DIGEST_DTYPE)
    with np.errstate(over="ignore"):
        np.add.at(out["entries"], bucket, np.uint64(1))
        np.add.at(out["sum"], bucket, h)
        np.bitwise_xor.at(out["xr"], bucket, h)
    return out


def key_hash(key) -> int:
    """Key bytes (or a str, taken as its UTF-8 bytes) -> the 64-bit key hash: rl_key_hash of
    include/rl_engine.h, the one definition the C++ host API and the device kernel share.
    Host code: no GPU is touched."""
    b = key.encode("utf-8") if isinstance(key, str) else bytes(key)
    return int(lib().rl_key_hash(b, len(b)))


def key_hash_model(key) -> int:
    """rl_key_hash restated in Python from its definition in include/rl_engine.h (FNV-1a 64
    over the bytes, each taken as unsigned, then the splitmix64 finaliser), for tests. Not used
    by the engine."""
    b = key.encode("utf-8") if isinstance(key, str) else bytes(key)
    h = 0xCBF29CE484222325
    for c in b:
        h = ((h ^ c) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return int(mix64(np.uint64(h)))


def pack_keys(keys, first_offset: int = 0):
    """A list of keys (bytes, or str taken as UTF-8) in the layout of rl_hash_keys /
    rl_execute_batch_keys: (blob uint8 array, off uint64 array of len(keys) + 1). The blob
    starts with first_offset filler bytes, so off[0] = first_offset."""
    parts = [k.encode("utf-8") if isinstance(k, str) else bytes(k) for k in keys]
    blob = np.frombuffer(b"\xa5" * int(first_offset) + b"".join(parts), np.uint8).copy()
    off = np.zeros(len(parts) + 1, np.uint64)
    off[0] = first_offset
    if parts:
        off[1:] = np.uint64(first_offset) + np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return blob, off


def owner_of(keys, shard_count: int):
    if shard_count <= 1:
        return np.zeros(np.shape(keys), np.uint32)
    s = int(shard_count).bit_length() - 1
    return (mix64(keys) >> np.uint64(64 - s)).astype(np.uint32)


class Engine:
    """One engine = one GPU's state table + stream (rl_create)."""

    def __init__(self, device: int = 0, max_batch: int = 1 << 22, capacity: int = 1 << 20,
                 stage_timing: bool = False, shard_index: int = 0, shard_count: int = 1,
                 max_skew_ms: int = 0, pipeline: bool = False, fixed_capacity: bool = False):
        self._L = lib()
        o = Opts(device=device, flags=(OPT_STAGE_TIMING if stage_timing else 0) |
                 (OPT_PIPELINE if pipeline else 0) | (OPT_FIXED_CAPACITY if fixed_capacity else 0),
                 max_batch=max_batch, default_capacity=capacity, shard_index=shard_index,
                 shard_count=shard_count, max_skew_ms=max_skew_ms)
        h = ctypes.c_void_p()
        st = self._L.rl_create(ctypes.byref(o), ctypes.byref(h))
        if st != RL_OK:
            raise RlError(st, "rl_create")
        self._h = h
        self.limiters = []
        # RL_TUNE="key=value,...": engine knobs for every engine of the process (A/B and
        # diagnostics runs of the test suite; every setting gives the same decisions)
        for kv in filter(None, os.environ.get("RL_TUNE", "").split(",")):
            k, v = kv.split("=")
            self.tune(k.strip(), int(v))

    def close(self):
        if getattr(self, "_h", None):
            self._L.rl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    def add_limiter(self, algo, max_permits, window_ms, refill_per_s=0.0, capacity=0,
                    local_cache_ttl_ms=0) -> int:
        """local_cache_ttl_ms > 0: the sliding window's Caffeine local cache (parity mode,
        the default, has it off as the reference's own test does)."""
        c = LimiterConfig(algo=int(algo), flags=LIM_LOCAL_CACHE if local_cache_ttl_ms else 0,
                          max_permits=int(max_permits), window_ms=int(window_ms),
                          refill_per_s=float(refill_per_s), capacity=int(capacity),
                          local_cache_ttl_ms=int(local_cache_ttl_ms))
        lid = ctypes.c_uint16()
        st = self._L.rl_add_limiter_ex(self._h, ctypes.byref(c), ctypes.byref(lid))
        if st != RL_OK:
            raise RlError(st, "rl_add_limiter")
        self.limiters.append((algo, max_permits, window_ms, refill_per_s))
        return lid.value

    def execute(self, keys, permits, now_ns, limiter=None, ops=None, want_tokens=True):
        """Host-buffer batch. Returns (allowed u8, remaining i64, tokens f64|None, status)."""
        keys = np.ascontiguousarray(keys, np.uint64)
        permits = np.ascontiguousarray(permits, np.int32)
        now_ns = np.ascontiguousarray(now_ns, np.int64)
        limiter = None if limiter is None else np.ascontiguousarray(limiter, np.uint16)
        ops = None if ops is None else np.ascontiguousarray(ops, np.uint8)
        n = keys.shape[0]
        allowed = np.zeros(n, np.uint8)
        remaining = np.zeros(n, np.int64)
        tokens = np.zeros(n, np.float64) if want_tokens else None
        st = self._L.rl_execute_batch(self._h, n, _p(keys), _p(permits), _p(now_ns), _p(limiter),
                                      _p(ops), _p(allowed), _p(remaining), _p(tokens))
        if st in (RL_E_DEVICE, RL_E_NOMEM, RL_E_TOO_LARGE):
            raise RlError(st, "rl_execute_batch")
        return allowed, remaining, tokens, st

    def hash_keys(self, blob, off):
        """rl_hash_keys on a host key batch (pack_keys): the keys' hashes, computed on the
        device, as a uint64 array. Read-only. Raises RlError(RL_E_INVALID_ARG) for a malformed
        offset."""
        blob = np.ascontiguousarray(blob, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        n = max(off.shape[0] - 1, 0)
        out = np.zeros(n, np.uint64)
        st = self._L.rl_hash_keys(self._h, n, _p(blob) if blob.shape[0] else None, blob.shape[0],
                                  _p(off), _p(out) if n else None)
        if st != RL_OK:
            raise RlError(st, "rl_hash_keys")
        return out

    def hash_keys_device(self, n, key_bytes, key_bytes_len, key_off, key_hash, hdr, stream=None):
        """rl_hash_keys_device on device buffers (torch tensors or raw pointers): key_hash[i] =
        the hash of the bytes [key_off[i], key_off[i + 1]) of key_bytes, 0 for a malformed key;
        hdr (2 x 8 bytes) = {malformed keys, n}. Asynchronous."""
        st = self._L.rl_hash_keys_device(self._h, int(n), _p(key_bytes), int(key_bytes_len),
                                         _p(key_off), _p(key_hash), _p(hdr), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_hash_keys_device")

    def execute_batch_keys(self, blob, off, permits, now_ns, limiter=None, ops=None, want_tokens=True,
                           want_hashes=True):
        """rl_execute_batch_keys: execute() on a host key batch (pack_keys), hashed on the
        device. Returns (allowed u8, remaining i64, tokens f64|None, status, hashes u64|None)."""
        blob = np.ascontiguousarray(blob, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        permits = np.ascontiguousarray(permits, np.int32)
        now_ns = np.ascontiguousarray(now_ns, np.int64)
        limiter = None if limiter is None else np.ascontiguousarray(limiter, np.uint16)
        ops = None if ops is None else np.ascontiguousarray(ops, np.uint8)
        n = max(off.shape[0] - 1, 0)
        allowed = np.zeros(n, np.uint8)
        remaining = np.zeros(n, np.int64)
        tokens = np.zeros(n, np.float64) if want_tokens else None
        hashes = np.zeros(n, np.uint64) if want_hashes else None
        st = self._L.rl_execute_batch_keys(self._h, n, _p(blob) if blob.shape[0] else None,
                                           blob.shape[0], _p(off), _p(permits), _p(now_ns),
                                           _p(limiter), _p(ops), _p(allowed), _p(remaining),
                                           _p(tokens), _p(hashes))
        if st in (RL_E_DEVICE, RL_E_NOMEM, RL_E_TOO_LARGE, RL_E_INVALID_ARG):
            raise RlError(st, "rl_execute_batch_keys")
        return allowed, remaining, tokens, st, hashes

    def grow_limiter(self, limiter: int, min_keys: int) -> None:
        st = self._L.rl_grow_limiter(self._h, limiter, min_keys)
        if st != RL_OK:
            raise RlError(st, "rl_grow_limiter")

    def limiter_slots(self, limiter: int) -> int:
        v = ctypes.c_uint64()
        st = self._L.rl_limiter_slots(self._h, limiter, ctypes.byref(v))
        if st != RL_OK:
            raise RlError(st, "rl_limiter_slots")
        return v.value

    def pin_host(self, arr) -> int:
        """rl_pin_host on a numpy array reused across host batches (status code)."""
        return self._L.rl_pin_host(self._h, _p(arr), arr.nbytes)

    def unpin_host(self, arr) -> int:
        return self._L.rl_unpin_host(self._h, _p(arr))

    def try_acquire_batch(self, keys, permits, now_ns, limiter=None):
        a, r, _, st = self.execute(keys, permits, now_ns, limiter, None, want_tokens=False)
        return a, r, st

    def execute_device(self, n, keys, permits, now_ns, limiter, ops, allowed, remaining,
                       tokens=None, stream=None):
        """Device-resident batch (torch tensors or raw device pointers); asynchronous."""
        st = self._L.rl_execute_batch_device(self._h, n, _p(keys), _p(permits), _p(now_ns),
                                             _p(limiter), _p(ops), _p(allowed), _p(remaining),
                                             _p(tokens), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_execute_batch_device")

    def last_status(self) -> int:
        return self._L.rl_last_status(self._h)

    def small_batches(self):
        """rl_small_batches: (taken, declined) of the small-batch path (tune("small_batch", v))."""
        taken, declined = ctypes.c_uint64(), ctypes.c_uint64()
        st = self._L.rl_small_batches(self._h, ctypes.byref(taken), ctypes.byref(declined))
        if st != RL_OK:
            raise RlError(st, "rl_small_batches")
        return taken.value, declined.value

    def available(self, limiter, keys, now_ns):
        keys = np.ascontiguousarray(keys, np.uint64)
        now_ns = np.ascontiguousarray(now_ns, np.int64)
        out = np.zeros(keys.shape[0], np.int64)
        st = self._L.rl_available(self._h, int(limiter), keys.shape[0], _p(keys), _p(now_ns),
                                  _p(out))
        return out, st

    def reset(self, limiter, keys, now_ns):
        keys = np.ascontiguousarray(keys, np.uint64)
        now_ns = np.ascontiguousarray(now_ns, np.int64)
        return self._L.rl_reset(self._h, int(limiter), keys.shape[0], _p(keys), _p(now_ns))

    def retry_after(self, limiter, keys, permits, now_ns, skip=None):
        """Milliseconds until an acquire of permits[i] on keys[i] would be allowed, from now_ns[i]
        (rl_retry_after): 0 = now, RETRY_NEVER, RETRY_INVALID. `limiter` is one id or an array;
        permits and now_ns broadcast; skip[i] != 0 answers 0 without a lookup (a batch's
        `allowed`). Read-only. Returns (wait_ms int64 array, status)."""
        keys = np.ascontiguousarray(keys, np.uint64)
        n = keys.shape[0]
        permits = np.ascontiguousarray(np.broadcast_to(np.asarray(permits, np.int32), (n,)))
        now_ns = np.ascontiguousarray(np.broadcast_to(np.asarray(now_ns, np.int64), (n,)))
        limiter = np.ascontiguousarray(np.broadcast_to(np.asarray(limiter, np.uint16), (n,)))
        skip = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        wait = np.zeros(n, np.int64)
        st = self._L.rl_retry_after(self._h, n, _p(keys), _p(permits), _p(now_ns), _p(limiter),
                                    _p(skip), _p(wait))
        if st not in (RL_OK, RL_E_INVALID_REQUEST):
            raise RlError(st, "rl_retry_after")
        return wait, st

    def retry_after_device(self, n, keys, permits, now_ns, limiter, skip, wait, stream=None):
        """rl_retry_after_device on device buffers (torch tensors or raw pointers; limiter and
        skip may be None); asynchronous, ordered behind the batches submitted before it."""
        st = self._L.rl_retry_after_device(self._h, n, _p(keys), _p(permits), _p(now_ns),
                                           _p(limiter), _p(skip), _p(wait), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_retry_after_device")

    def quota(self, limiter, keys, now_ns, permits=None, skip=None):
        """The rate-limit header numbers of keys[i] at now_ns[i] from one lookup per key (rl_quota):
        remaining = what available() reads, reset_ms = milliseconds until it reads maxPermits
        again (0: now), and with `permits` retry_ms = what retry_after() answers (skip[i] != 0: 0
        without a search). QUOTA_INVALID in every output of an invalid query. `limiter` is one id
        or an array; permits and now_ns broadcast. Read-only.
        Returns (remaining, reset_ms, retry_ms | None, status)."""
        keys = np.ascontiguousarray(keys, np.uint64)
        n = keys.shape[0]
        now_ns = np.ascontiguousarray(np.broadcast_to(np.asarray(now_ns, np.int64), (n,)))
        limiter = np.ascontiguousarray(np.broadcast_to(np.asarray(limiter, np.uint16), (n,)))
        if permits is not None:
            permits = np.ascontiguousarray(np.broadcast_to(np.asarray(permits, np.int32), (n,)))
        skip = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        remaining = np.zeros(n, np.int64)
        reset = np.zeros(n, np.int64)
        retry = None if permits is None else np.zeros(n, np.int64)
        st = self._L.rl_quota(self._h, n, _p(keys), _p(now_ns), _p(limiter), _p(permits), _p(skip),
                              _p(remaining), _p(reset), _p(retry))
        if st not in (RL_OK, RL_E_INVALID_REQUEST):
            raise RlError(st, "rl_quota")
        return remaining, reset, retry, st

    def quota_device(self, n, keys, now_ns, limiter, permits, skip, remaining, reset, retry,
                     stream=None):
        """rl_quota_device on device buffers (torch tensors or raw pointers; limiter, skip, and
        permits together with retry may be None); asynchronous, ordered behind the batches
        submitted before it."""
        st = self._L.rl_quota_device(self._h, n, _p(keys), _p(now_ns), _p(limiter), _p(permits),
                                     _p(skip), _p(remaining), _p(reset), _p(retry), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_quota_device")

    def top_keys(self, keys, k, min_count):
        """The keys of a host array that occur at least min_count times, the k most frequent
        first (count descending, key ascending), exact (rl_top_keys). Returns (keys uint64,
        counts uint64, n_heavy); raises RlError(RL_E_CAPACITY) when the sample overflows."""
        keys = np.ascontiguousarray(keys, np.uint64)
        k = int(k)
        top = np.zeros(max(min(k, TOP_KEYS_MAX), 0), np.uint64)
        cnt = np.zeros_like(top)
        n_out = ctypes.c_size_t(0)
        n_heavy = ctypes.c_uint64(0)
        st = self._L.rl_top_keys(self._h, keys.shape[0], _p(keys) if keys.shape[0] else None, k,
                                 int(min_count), _p(top), _p(cnt), ctypes.byref(n_out),
                                 ctypes.byref(n_heavy))
        if st != RL_OK:
            raise RlError(st, "rl_top_keys")
        return top[:n_out.value], cnt[:n_out.value], n_heavy.value

    def top_keys_device(self, keys, k, min_count, stream=None):
        """rl_top_keys_device on a device tensor of key hashes (8-byte integers). Returns
        (keys, counts, n_heavy): two device tensors of n_out 64-bit words holding unsigned
        values (torch.uint64 views) and an int; reads the header back, so it synchronises.
        Raises RlError(RL_E_CAPACITY) when the sample overflows."""
        import torch
        assert keys.element_size() == 8 and keys.is_contiguous()
        k = int(k)
        top = torch.zeros(max(min(k, TOP_KEYS_MAX), 1), dtype=torch.int64, device=keys.device)
        cnt = torch.zeros_like(top)
        hdr = torch.zeros(4, dtype=torch.int64, device=keys.device)
        st = self._L.rl_top_keys_device(self._h, keys.numel(), _p(keys) if keys.numel() else None, k,
                                        int(min_count), _p(top), _p(cnt), _p(hdr), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_top_keys_device")
        self.sync()
        n_out, n_heavy, overflow, _ = (int(x) for x in hdr.cpu())
        if overflow:
            raise RlError(RL_E_CAPACITY, "rl_top_keys_device")
        return top[:n_out].view(torch.uint64), cnt[:n_out].view(torch.uint64), n_heavy

    def tally_batch(self, permits, limiter, ops, allowed, remaining, out=None):
        """Per-limiter counts of a finished host batch (rl_tally_batch): a TALLY_DTYPE array of
        TALLY_ROWS rows, row = limiter id, TALLY_UNKNOWN for ids the engine does not know.
        `limiter` and `ops` may be None. With `out` (such an array) the counts are added to it
        (RL_TALLY_ACCUMULATE) and it is returned. Read-only."""
        permits = np.ascontiguousarray(permits, np.int32)
        limiter = None if limiter is None else np.ascontiguousarray(limiter, np.uint16)
        ops = None if ops is None else np.ascontiguousarray(ops, np.uint8)
        allowed = np.ascontiguousarray(allowed, np.uint8)
        remaining = np.ascontiguousarray(remaining, np.int64)
        flags = 0 if out is None else TALLY_ACCUMULATE
        if out is None:
            out = np.zeros(TALLY_ROWS, TALLY_DTYPE)
        assert out.dtype == TALLY_DTYPE and out.shape == (TALLY_ROWS,)
        st = self._L.rl_tally_batch(self._h, permits.shape[0], _p(permits), _p(limiter), _p(ops),
                                    _p(allowed), _p(remaining), _p(out), flags)
        if st != RL_OK:
            raise RlError(st, "rl_tally_batch")
        return out

    def tally_batch_device(self, n, permits, limiter, ops, allowed, remaining, out, accumulate=False,
                           stream=None):
        """rl_tally_batch_device on device buffers (torch tensors or raw pointers; limiter and ops
        may be None); `out` is a device buffer of TALLY_ROWS x 96 bytes, 8-byte aligned.
        Asynchronous, ordered behind the batches submitted before it."""
        st = self._L.rl_tally_batch_device(self._h, int(n), _p(permits), _p(limiter), _p(ops), _p(allowed),
                                           _p(remaining), _p(out), TALLY_ACCUMULATE if accumulate else 0,
                                           _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_tally_batch_device")

    def top_denied(self, keys, permits, limiter, ops, allowed, remaining, sel_limiter, k, min_count):
        """The keys of a finished host batch denied at least min_count times under limiter
        sel_limiter, the k most often denied first (rl_top_denied; order as top_keys). Returns
        (keys uint64, counts uint64, n_heavy, n_denied); raises RlError(RL_E_CAPACITY) when the
        denied keys overflow the candidate store. Read-only."""
        keys = np.ascontiguousarray(keys, np.uint64)
        permits = np.ascontiguousarray(permits, np.int32)
        limiter = None if limiter is None else np.ascontiguousarray(limiter, np.uint16)
        ops = None if ops is None else np.ascontiguousarray(ops, np.uint8)
        allowed = np.ascontiguousarray(allowed, np.uint8)
        remaining = np.ascontiguousarray(remaining, np.int64)
        k, n = int(k), keys.shape[0]
        top = np.zeros(max(min(k, TOP_KEYS_MAX), 0), np.uint64)
        cnt = np.zeros_like(top)
        n_out = ctypes.c_size_t(0)
        n_heavy, n_denied = ctypes.c_uint64(0), ctypes.c_uint64(0)
        st = self._L.rl_top_denied(self._h, n, _p(keys) if n else None, _p(permits), _p(limiter), _p(ops),
                                   _p(allowed), _p(remaining), int(sel_limiter), k, int(min_count),
                                   _p(top), _p(cnt), ctypes.byref(n_out), ctypes.byref(n_heavy),
                                   ctypes.byref(n_denied))
        if st != RL_OK:
            raise RlError(st, "rl_top_denied")
        return top[:n_out.value], cnt[:n_out.value], n_heavy.value, n_denied.value

    def top_denied_device(self, n, keys, permits, limiter, ops, allowed, remaining, sel_limiter, k,
                          min_count, stream=None):
        """rl_top_denied_device on device tensors (limiter and ops may be None). Returns (keys,
        counts, n_heavy, n_denied) as top_keys_device does: two device tensors of n_out 64-bit
        words (torch.uint64 views) and two ints; reads the header back, so it synchronises.
        Raises RlError(RL_E_CAPACITY) on overflow."""
        import torch
        k = int(k)
        dev = allowed.device
        top = torch.zeros(max(min(k, TOP_KEYS_MAX), 1), dtype=torch.int64, device=dev)
        cnt = torch.zeros_like(top)
        hdr = torch.zeros(4, dtype=torch.int64, device=dev)
        st = self._L.rl_top_denied_device(self._h, int(n), _p(keys) if n else None, _p(permits),
                                          _p(limiter), _p(ops), _p(allowed), _p(remaining),
                                          int(sel_limiter), k, int(min_count), _p(top), _p(cnt), _p(hdr),
                                          _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_top_denied_device")
        self.sync()
        n_out, n_heavy, overflow, n_denied = (int(x) for x in hdr.cpu())
        if overflow:
            raise RlError(RL_E_CAPACITY, "rl_top_denied_device")
        return top[:n_out].view(torch.uint64), cnt[:n_out].view(torch.uint64), n_heavy, n_denied

    def limiter_usage(self, limiter, now_ns) -> dict:
        """Census of one limiter's table at now_ns (rl_limiter_usage): a dict of the rl_usage
        fields, `hist` as a list of USAGE_BINS counts. Read-only."""
        u = Usage()
        st = self._L.rl_limiter_usage(self._h, int(limiter), int(now_ns), ctypes.byref(u))
        if st != RL_OK:
            raise RlError(st, "rl_limiter_usage")
        d = {f: getattr(u, f) for f, _ in Usage._fields_ if f != "hist"}
        d["hist"] = list(u.hist)
        return d

    def top_consumers(self, limiter, now_ns, k, min_used=1):
        """The live keys of a limiter that have used at least min_used permits at now_ns, the k
        heaviest first (used descending, key hash ascending), exact however many tie
        (rl_top_consumers). Returns (key hashes uint64, used int64, n_match). Read-only."""
        k = int(k)
        keys = np.zeros(max(min(k, TOP_KEYS_MAX), 0), np.uint64)
        used = np.zeros(keys.shape[0], np.int64)
        n_out = ctypes.c_size_t(0)
        n_match = ctypes.c_uint64(0)
        st = self._L.rl_top_consumers(self._h, int(limiter), int(now_ns), k, int(min_used),
                                      _p(keys), _p(used), ctypes.byref(n_out),
                                      ctypes.byref(n_match))
        if st != RL_OK:
            raise RlError(st, "rl_top_consumers")
        return keys[:n_out.value], used[:n_out.value], n_match.value

    def limiter_digest(self, limiter, now_ns, bucket_bits, cache=True):
        """Per-bucket fingerprints of a limiter's live state at now_ns (rl_limiter_digest), with
        the rejecting local-cache entries unless `cache` is false. Returns (a DIGEST_DTYPE array
        of 2^bucket_bits buckets, the total over them as an (entries, sum, xr) tuple). Read-only."""
        bits, slots = int(bucket_bits), ctypes.c_uint64(0)
        known = self._L.rl_limiter_slots(self._h, int(limiter), ctypes.byref(slots)) == RL_OK
        fits = known and 0 <= bits < 64 and (slots.value // REGION_SLOTS) >> bits   # (else: refused below)
        out = np.zeros(1 << bits if fits else 1, DIGEST_DTYPE)
        tot = BucketDigest()
        st = self._L.rl_limiter_digest(self._h, int(limiter), int(now_ns), int(bucket_bits),
                                       DIGEST_CACHE if cache else 0, _p(out), ctypes.byref(tot))
        if st != RL_OK:
            raise RlError(st, "rl_limiter_digest")
        return out, (tot.entries, tot.sum, tot.xr)

    def limiter_digest_device(self, limiter, now_ns, bucket_bits, out, cache=True, stream=None):
        """rl_limiter_digest_device: `out` is a device buffer of 2^bucket_bits x 24 bytes (a torch
        tensor or a raw pointer, 8-byte aligned); asynchronous, ordered behind the batches
        submitted before it."""
        st = self._L.rl_limiter_digest_device(self._h, int(limiter), int(now_ns), int(bucket_bits),
                                              DIGEST_CACHE if cache else 0, _p(out), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_limiter_digest_device")

    def check_limiter(self, limiter, region_begin=0, region_count=1 << 62) -> dict:
        """Check the slot invariants of a limiter's table (rl_check_limiter) over the regions
        [region_begin, region_begin + region_count), clipped to the table: a dict of the
        rl_check_report fields (check_dict). bad_slots == 0: the range is sound. Read-only."""
        r = CheckReport()
        st = self._L.rl_check_limiter(self._h, int(limiter), int(region_begin), int(region_count),
                                      ctypes.byref(r))
        if st != RL_OK:
            raise RlError(st, "rl_check_limiter")
        return check_dict(r)

    def check_limiter_device(self, limiter, region_begin, region_count, out, stream=None):
        """rl_check_limiter_device: `out` is a device buffer of CHECK_WORDS x 8 bytes (a torch
        tensor or a raw pointer, 8-byte aligned); asynchronous, ordered behind the batches
        submitted before it."""
        st = self._L.rl_check_limiter_device(self._h, int(limiter), int(region_begin),
                                             int(region_count), _p(out), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_check_limiter_device")

    def check_table_device(self, limiter, slots, cache_words, region_bits, out, stream=None):
        """rl_check_table_device: the same check over a caller-held device array of 2^region_bits
        regions of 256 slots of 32 bytes (`cache_words`: one uint64 per slot, or None), with the
        limiter's constants; asynchronous, `out` as for check_limiter_device."""
        st = self._L.rl_check_table_device(self._h, int(limiter), _p(slots), _p(cache_words),
                                           int(region_bits), _p(out), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_check_table_device")

    def check_images(self, images) -> dict:
        """The value classes over host KEY_IMAGE_DTYPE images (rl_check_images): a dict as
        check_limiter's, `first` holding image indices."""
        images = np.ascontiguousarray(images, KEY_IMAGE_DTYPE)
        r = CheckReport()
        st = self._L.rl_check_images(self._h, images.shape[0], _p(images) if images.shape[0] else None,
                                     ctypes.byref(r))
        if st != RL_OK:
            raise RlError(st, "rl_check_images")
        return check_dict(r)

    def check_images_device(self, n, images, out, stream=None):
        """rl_check_images_device: n device images (16-byte aligned), `out` as for
        check_limiter_device; asynchronous."""
        st = self._L.rl_check_images_device(self._h, int(n), _p(images), _p(out), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_check_images_device")

    def export_state(self, now_ns):
        """Live state at now_ns in the Redis layout: a STATE_DTYPE array (rl_export_state)."""
        n = ctypes.c_size_t(0)
        st = self._L.rl_export_state(self._h, int(now_ns), None, 0, ctypes.byref(n))
        while True:
            if st == RL_OK and n.value == 0:
                return np.zeros(0, STATE_DTYPE)
            if st not in (RL_OK, RL_E_TOO_LARGE):
                raise RlError(st, "rl_export_state")
            out = np.zeros(n.value + 1024, STATE_DTYPE)   # state may grow between calls
            st = self._L.rl_export_state(self._h, int(now_ns), _p(out), out.shape[0], ctypes.byref(n))
            if st == RL_OK:
                return out[:n.value]

    def import_state(self, entries):
        """Load STATE_DTYPE entries (rl_import_state). Returns (status, entries taken)."""
        entries = np.ascontiguousarray(entries, STATE_DTYPE)
        n = ctypes.c_size_t(0)
        st = self._L.rl_import_state(self._h, _p(entries) if entries.shape[0] else None,
                                     entries.shape[0], ctypes.byref(n))
        return st, n.value

    def copy_keys(self, keys, cap=None):
        """Images of the listed keys' state under every limiter (rl_copy_keys): a
        KEY_IMAGE_DTYPE array sorted by (limiter, key_hash). Read-only. With `cap` the call is
        made once with a buffer of that many images and returns (images, status, n_out)."""
        keys = np.ascontiguousarray(keys, np.uint64)
        n = ctypes.c_size_t(0)
        kp = _p(keys) if keys.shape[0] else None
        if cap is not None:
            out = np.zeros(int(cap), KEY_IMAGE_DTYPE)
            st = self._L.rl_copy_keys(self._h, keys.shape[0], kp, _p(out) if cap else None, int(cap),
                                      ctypes.byref(n))
            return out, st, n.value
        out = np.zeros(keys.shape[0] * max(len(self.limiters), 1), KEY_IMAGE_DTYPE)
        st = self._L.rl_copy_keys(self._h, keys.shape[0], kp, _p(out) if out.shape[0] else None,
                                  out.shape[0], ctypes.byref(n))
        if st != RL_OK:
            raise RlError(st, "rl_copy_keys")
        return out[:n.value]

    def drop_keys(self, keys) -> int:
        """Turn the listed keys' slots into tombstones (rl_drop_keys); returns the slots dropped."""
        keys = np.ascontiguousarray(keys, np.uint64)
        n = ctypes.c_uint64(0)
        st = self._L.rl_drop_keys(self._h, keys.shape[0], _p(keys) if keys.shape[0] else None,
                                  ctypes.byref(n))
        if st != RL_OK:
            raise RlError(st, "rl_drop_keys")
        return n.value

    def put_keys(self, images):
        """Insert KEY_IMAGE_DTYPE images (rl_put_keys). Returns (status, images put); the status
        is RL_OK or RL_E_CAPACITY, anything else raises."""
        images = np.ascontiguousarray(images, KEY_IMAGE_DTYPE)
        n = ctypes.c_size_t(0)
        st = self._L.rl_put_keys(self._h, images.shape[0], _p(images) if images.shape[0] else None,
                                 ctypes.byref(n))
        if st not in (RL_OK, RL_E_CAPACITY):
            raise RlError(st, "rl_put_keys")
        return st, n.value

    def snapshot_keys(self, limiter, region_begin, region_count, cap, out=None):
        """One chunk of a limiter's table as images (rl_snapshot_keys): the regions
        [region_begin, region_begin + region_count), whole regions only, in (region, slot) order.
        Returns (images, status, n_out, regions_done, regions_total): `images` is the buffer of
        `cap` entries (`out`, or a zeroed KEY_IMAGE_DTYPE array) of which the first n_out are
        written; status is RL_OK or RL_E_TOO_LARGE (n_out = the first region's count), anything
        else raises. Read-only."""
        cap = int(cap)
        if out is None:
            out = np.zeros(cap, KEY_IMAGE_DTYPE)
        assert out.dtype == KEY_IMAGE_DTYPE and out.shape[0] >= cap
        n, done, total = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        st = self._L.rl_snapshot_keys(self._h, int(limiter), int(region_begin), int(region_count),
                                      _p(out) if cap else None, cap, ctypes.byref(n),
                                      ctypes.byref(done), ctypes.byref(total))
        if st not in (RL_OK, RL_E_TOO_LARGE):
            raise RlError(st, "rl_snapshot_keys")
        return out, st, n.value, done.value, total.value

    def snapshot(self, limiter, chunk=1 << 20):
        """Generator over a limiter's whole table in chunks of at most `chunk` images (at least
        SNAPSHOT_MIN_CAP): yields KEY_IMAGE_DTYPE arrays whose concatenation is the table in
        (region, slot) order. No batch may run between the chunks of a point-in-time snapshot;
        raises RuntimeError if the table grew meanwhile."""
        chunk = max(int(chunk), SNAPSHOT_MIN_CAP)
        at, total0 = 0, None
        while True:
            out, st, n, done, total = self.snapshot_keys(limiter, at, 1 << 62, chunk)
            if st != RL_OK:
                raise RlError(st, "rl_snapshot_keys")
            if total0 is not None and total != total0:
                raise RuntimeError("the table grew between two snapshot chunks: start over")
            total0 = total
            if n:
                yield out[:n]
            at += done
            if at >= total:
                return

    def snapshot_keys_device(self, limiter, region_begin, region_count, out, cap, hdr, stream=None):
        """rl_snapshot_keys_device: `out` (48-byte images) and `hdr` (4 x 8 bytes) are device
        buffers (torch tensors or raw pointers); asynchronous, hdr = {n_out, regions_done,
        regions_total, 0}."""
        st = self._L.rl_snapshot_keys_device(self._h, int(limiter), int(region_begin),
                                             int(region_count), _p(out), int(cap), _p(hdr), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_snapshot_keys_device")

    def put_keys_device(self, n, images, hdr, stream=None):
        """rl_put_keys_device: n device images in ordered form (a snapshot's order); asynchronous,
        hdr (device, 4 x 8 bytes) = {n_put, n_failed, rejected, n}."""
        st = self._L.rl_put_keys_device(self._h, int(n), _p(images), _p(hdr), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_put_keys_device")

    def restore_keys(self, images):
        """Insert host KEY_IMAGE_DTYPE images of any order and number (rl_restore_keys). Returns
        (status, images put) as put_keys does."""
        images = np.ascontiguousarray(images, KEY_IMAGE_DTYPE)
        n = ctypes.c_size_t(0)
        st = self._L.rl_restore_keys(self._h, images.shape[0], _p(images) if images.shape[0] else None,
                                     ctypes.byref(n))
        if st not in (RL_OK, RL_E_CAPACITY):
            raise RlError(st, "rl_restore_keys")
        return st, n.value

    def sweep_expired(self, now_ns) -> int:
        """Free every slot with no bucket live at now_ns (rl_sweep_expired); returns the count."""
        n = ctypes.c_uint64(0)
        st = self._L.rl_sweep_expired(self._h, int(now_ns), ctypes.byref(n))
        if st != RL_OK:
            raise RlError(st, "rl_sweep_expired")
        return n.value

    @staticmethod
    def _shrink_dict(r) -> dict:
        d = {f: getattr(r, f) for f, _ in ShrinkReport._fields_ if f != "fullest"}
        d["fullest"] = list(r.fullest)[:r.levels]
        return d

    def shrink_plan(self, limiter, now_ns, min_keys=0) -> dict:
        """What shrink_limiter would do at now_ns (rl_shrink_plan): a dict of the rl_shrink_report
        fields, `fullest` as a list of `levels` counts. Read-only."""
        r = ShrinkReport()
        st = self._L.rl_shrink_plan(self._h, int(limiter), int(now_ns), int(min_keys), ctypes.byref(r))
        if st != RL_OK:
            raise RlError(st, "rl_shrink_plan")
        return self._shrink_dict(r)

    def shrink_limiter(self, limiter, now_ns, min_keys=0) -> dict:
        """Halve the limiter's region count as often as its live keys at now_ns allow
        (rl_shrink_limiter), keeping room for min_keys keys; dead slots are not carried. Returns
        the plan acted on (halvings == 0: the table was left alone)."""
        r = ShrinkReport()
        st = self._L.rl_shrink_limiter(self._h, int(limiter), int(now_ns), int(min_keys), ctypes.byref(r))
        if st != RL_OK:
            raise RlError(st, "rl_shrink_limiter")
        return self._shrink_dict(r)

    def stats(self) -> dict:
        s = BatchStats()
        self._L.rl_batch_stats_get(self._h, ctypes.byref(s))
        return {f: getattr(s, f) for f, _ in BatchStats._fields_}

    def stage_times(self) -> dict:
        names = (ctypes.c_char_p * 16)()
        ms = (ctypes.c_float * 16)()
        k = self._L.rl_stage_times(self._h, names, ms, 16)
        return {names[i].decode(): float(ms[i]) for i in range(k)}

    def tune(self, key: str, value: int):
        st = self._L.rl_tune(self._h, key.encode(), int(value))
        if st != RL_OK:
            raise RlError(st, "rl_tune")

    def debug_region_times(self, n_bins):
        """Per-bin {t_start, t_end, records, rounds} of the last batch (rl_tune debug_regions)."""
        out = np.zeros((n_bins, 28), np.uint64)     # kDbgWords
        k = self._L.rl_debug_fetch(self._h, b"region_times", _p(out), out.nbytes)
        if k < 0:
            raise RlError(k, "rl_debug_fetch")
        return out[:k]

    def debug_bin_totals(self):
        """The last batch's pass-0 bin sizes (2^kMaxDigitBits entries; beyond the batch's own bins
        zero, or an earlier, wider batch's)."""
        out = np.zeros(1 << 13, np.uint32)
        k = self._L.rl_debug_fetch(self._h, b"bin_totals", _p(out), out.nbytes)
        if k < 0:
            raise RlError(k, "rl_debug_fetch")
        return out[:k]

    def debug_alloc_probe(self, nbytes=4096):
        """A fresh device allocation of nbytes as the library's allocator hands it out
        (rl_debug_fetch "alloc_probe"): with debug_alloc_fill on, every byte is the fill."""
        out = np.zeros(int(nbytes), np.uint8)
        k = self._L.rl_debug_fetch(self._h, b"alloc_probe", _p(out), out.nbytes)
        if k < 0:
            raise RlError(k, "rl_debug_fetch")
        return out[:k]

    def sync(self):
        st = self._L.rl_sync(self._h)
        if st != RL_OK:
            raise RlError(st, "rl_sync")

    def route_partition(self, n, keys_dev, perm_dev, shard_count, stream=None):
        counts = np.zeros(shard_count, np.uint64)
        st = self._L.rl_route_partition(self._h, n, _p(keys_dev), None, shard_count,
                                        _p(perm_dev), _p(counts), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_partition")
        return counts

    def route_pack(self, n, perm, key, permits, now, limiter, key_o, permits_o, now_o, limiter_o,
                   stream=None):
        st = self._L.rl_route_pack(self._h, n, _p(perm), _p(key), _p(permits), _p(now),
                                   _p(limiter), _p(key_o), _p(permits_o), _p(now_o),
                                   _p(limiter_o), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_pack")

    def route_fold(self, n, allowed, remaining, packed, stream=None):
        st = self._L.rl_route_fold(self._h, n, _p(allowed), _p(remaining), _p(packed), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_fold")

    def route_unpack(self, n, perm, packed, allowed, remaining, stream=None):
        st = self._L.rl_route_unpack(self._h, n, _p(perm), _p(packed), _p(allowed), _p(remaining),
                                     _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_unpack")

    def route_pack_wire(self, n, perm, key, permits, now, limiter, wire_o, limiter_o, hdr,
                        stream=None):
        st = self._L.rl_route_pack_wire(self._h, n, _p(perm), _p(key), _p(permits), _p(now),
                                        _p(limiter), _p(wire_o), _p(limiter_o), _p(hdr),
                                        _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_pack_wire")

    def route_unwire(self, m, wire, src_base, src_count, key_o, permits_o, now_o, stream=None):
        base = np.ascontiguousarray(src_base, dtype=np.int64)
        cnt = np.ascontiguousarray(src_count, dtype=np.uint64)
        st = self._L.rl_route_unwire(self._h, m, _p(wire), len(base), base.ctypes.data,
                                     cnt.ctypes.data, _p(key_o), _p(permits_o), _p(now_o),
                                     _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_unwire")

    def result_width(self):
        w = self._L.rl_result_width(self._h)
        if w < 0:
            raise RlError(w, "rl_result_width")
        return w

    def route_fold_packed(self, n, allowed, remaining, packed, width, stream=None):
        st = self._L.rl_route_fold_packed(self._h, n, _p(allowed), _p(remaining), _p(packed),
                                          width, _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_fold_packed")

    def route_unpack_packed(self, n, perm, packed, width, allowed, remaining, stream=None):
        st = self._L.rl_route_unpack_packed(self._h, n, _p(perm), _p(packed), width, _p(allowed),
                                            _p(remaining), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_unpack_packed")

    def route_return_bytes(self, seg_counts, width, exc_cap):
        c = np.ascontiguousarray(seg_counts, dtype=np.uint64)
        return int(self._L.rl_route_return_bytes(len(c), c.ctypes.data, width, exc_cap))

    def route_fold_return(self, m, allowed, remaining, out, width, seg_counts, exc_cap,
                          stream=None):
        c = np.ascontiguousarray(seg_counts, dtype=np.uint64)
        st = self._L.rl_route_fold_return(self._h, m, _p(allowed), _p(remaining), _p(out), width,
                                          len(c), c.ctypes.data, exc_cap, _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_fold_return")

    def route_unpack_return(self, n, perm, inp, width, seg_counts, exc_cap, allowed, remaining,
                            lost, stream=None):
        c = np.ascontiguousarray(seg_counts, dtype=np.uint64)
        st = self._L.rl_route_unpack_return(self._h, n, _p(perm), _p(inp), width, len(c),
                                            c.ctypes.data, exc_cap, _p(allowed), _p(remaining),
                                            _p(lost), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_unpack_return")

    def set_owner_directory(self, keys, owners):
        k = np.ascontiguousarray(keys, np.uint64)
        o = np.ascontiguousarray(owners, np.uint32)
        st = self._L.rl_set_owner_directory(self._h, len(k), _p(k) if len(k) else None,
                                            _p(o) if len(o) else None)
        if st != RL_OK:
            raise RlError(st, "rl_set_owner_directory")

    def owner_of(self, key_hash) -> int:
        return int(self._L.rl_owner_of_engine(self._h, int(key_hash)))

    def route_partition_device(self, n, keys_dev, perm_dev, shard_count, counts_dev, stride,
                               stream=None):
        st = self._L.rl_route_partition_device(self._h, n, _p(keys_dev), shard_count, _p(perm_dev),
                                               _p(counts_dev), stride, _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_partition_device")

    def route_partition_skip_device(self, n, keys_dev, skip_dev, perm_dev, shard_count, counts_dev,
                                    stride, stream=None):
        """rl_route_partition_skip_device: the owner partition of the requests with skip == 0
        (skip_dev None: all of them); the live counts land in counts_dev[s * stride]."""
        st = self._L.rl_route_partition_skip_device(self._h, n, _p(keys_dev), _p(skip_dev),
                                                    shard_count, _p(perm_dev), _p(counts_dev),
                                                    stride, _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_partition_skip_device")

    def route_fold_ops(self, n, perm, limiter, op, col, stream=None):
        """col[j] = min(limiter[perm[j]], 0x3FFF) | min(op[perm[j]], 3) << 14 (either None: 0)."""
        st = self._L.rl_route_fold_ops(self._h, n, _p(perm), _p(limiter), _p(op), _p(col), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_fold_ops")

    def route_unfold_ops(self, m, col, limiter_o, op_o, stream=None):
        """limiter_o[j] = col[j] & 0x3FFF, op_o[j] = col[j] >> 14 (limiter_o may be col)."""
        st = self._L.rl_route_unfold_ops(self._h, m, _p(col), _p(limiter_o), _p(op_o), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_unfold_ops")

    def route_unpack_wait(self, n, n_live, perm, back, skip, wait, stream=None):
        """wait[i] = 0 where skip[i] != 0; wait[perm[j]] = back[j] for j < n_live."""
        st = self._L.rl_route_unpack_wait(self._h, n, n_live, _p(perm), _p(back), _p(skip), _p(wait),
                                          _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_route_unpack_wait")

    def synth_trace(self, n, keys, permits, now_ns, limiter, *, seed, n_keys, dist=DIST_UNIFORM,
                    zipf_s=1.1, permits_max=4, t0_ns=1_700_000_000_000 * 1_000_000,
                    span_ns=2_000_000_000, index_base=0, n_total=None, n_limiters=1,
                    stream=None):
        spec = TraceSpec(seed=seed, n_keys=n_keys, dist=dist, permits_max=permits_max,
                         zipf_s=zipf_s, t0_ns=t0_ns, span_ns=span_ns, index_base=index_base,
                         n_total=n_total or n, n_limiters=n_limiters)
        st = self._L.rl_synth_trace_device(self._h, ctypes.byref(spec), n, _p(keys), _p(permits),
                                           _p(now_ns), _p(limiter), _p(stream))
        if st != RL_OK:
            raise RlError(st, "rl_synth_trace_device")
