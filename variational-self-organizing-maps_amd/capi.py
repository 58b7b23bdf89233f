"""ctypes binding of libvsom_hip.so (include/vsom_hip.h).

This is the product path: it loads the in-tree HIP library and fails loudly when the
library or a gfx950 device is missing -- there is no CPU fallback and nothing here touches
oracle/.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# the in-tree library; VSOM_LIB names another BUILD OF THE SAME LIBRARY (the -DVSOM_DEVELOPMENT build of tools/exp/,
# which times variant code objects) without overwriting the shipped file
_INTREE = os.path.join(_HERE, "libvsom_hip.so")
LIB_PATH = os.environ.get("VSOM_LIB") or _INTREE

STANDARD, MEDIAN, CLR = 0, 1, 2
CUSTOM = -1        # a caller-defined transformation from device source (vsom_create_custom)
CUSTOM_MAX_DEPTH = 5120     # VSOM_CUSTOM_MAX_DEPTH
EXPONENTIAL, INVERSE_PROPORTIONAL, BATCHMAP = 0, 1, 2
BMU_AUTO, BMU_EXACT, BMU_SHORTLIST = 0, 1, 2
UPDATE_STRICT, UPDATE_FMA, UPDATE_FMA_SIGMA = 0, 1, 2
SIGMA_AUTO, SIGMA_EAGER, SIGMA_LAZY = 0, 1, 2
BUF_MAP, BUF_SIGMA, BUF_S, BUF_WEIGHT, BUF_HITS, BUF_LASTBMU, BUF_SQRES, BUF_CHUNK, BUF_UMATRIX = range(9)
T_STAGE, T_BMU, T_FINISH, T_CW, T_UPDATE, T_ONLINE, T_SIGMA, T_COUNT = range(8)
TIMER_NAMES = ["stage", "bmu", "finish", "cw", "update", "online", "sigma"]
SIGMA_AS_WRITTEN, SIGMA_FLOOR = 0, 1       # vsom_sigma_rule
GENERATE_AS_WRITTEN, GENERATE_PER_ROW = 0, 1   # vsom_generate_rule
NO_UNIT = 2 ** 64 - 1      # the unit of a row without mass (UINT64_MAX)

# every symbol include/vsom_hip.h declares (tests/test_capi_symbols.py checks the header too)
SYMBOLS = [
    "vsom_last_error", "vsom_device_count", "vsom_create", "vsom_destroy", "vsom_set_stream",
    "vsom_synchronize", "vsom_set_bmu_mode", "vsom_set_update_mode", "vsom_set_column_compaction", "vsom_set_row_dedupe", "vsom_get_shortlist_stats", "vsom_depth", "vsom_nodes", "vsom_set_state",
    "vsom_get_state", "vsom_upload_chunk", "vsom_set_chunk_device", "vsom_host_alloc", "vsom_host_free",
    "vsom_prefetch_chunk", "vsom_prefetch_wait", "vsom_commit_chunk", "vsom_stage_next_device", "vsom_get_last_bmu",
    "vsom_set_last_bmu", "vsom_get_sqres", "vsom_bmu_batch", "vsom_find_bmu", "vsom_dist_single", "vsom_find_local_bmu", "vsom_find_restricted_bmu", "vsom_distances_single", "vsom_bmu_local_batch",
    "vsom_distances", "vsom_bmu_restricted_batch", "vsom_distances_row", "vsom_distances_raw", "vsom_bmd_batch", "vsom_bmu_topk_batch", "vsom_batch_phase1_async", "vsom_batch_finish_async",
    "vsom_batch_phase2_async", "vsom_batch_epoch_async", "vsom_batch_epoch", "vsom_get_mse",
    "vsom_residual_len", "vsom_train_single", "vsom_train_online_chunk", "vsom_train_online_chunk_acc", "vsom_train_online_chunk_fetch", "vsom_upload_chunk_async", "vsom_get_online_search_stats",
    "vsom_neighbourhood_weight", "vsom_device_ptr", "vsom_chunk_size", "vsom_pitch",
    "vsom_chunk_pitch", "vsom_small_map_chains", "vsom_enable_timing", "vsom_enable_timing_of", "vsom_get_timing",
    "vsom_group_create", "vsom_group_destroy", "vsom_group_size", "vsom_group_ctx", "vsom_group_transport",
    "vsom_group_synchronize", "vsom_group_set_state", "vsom_group_get_state", "vsom_group_set_update_mode",
    "vsom_group_set_bmu_mode", "vsom_group_upload_chunk", "vsom_group_prefetch_chunk", "vsom_group_prefetch_wait",
    "vsom_group_commit_chunk", "vsom_group_set_chunk_device", "vsom_group_set_last_bmu", "vsom_group_get_last_bmu",
    "vsom_group_batch_epoch_async", "vsom_group_batch_epoch", "vsom_group_get_mse",
    "vsom_create_custom", "vsom_custom_compile_check",
    "vsom_ensemble_create", "vsom_ensemble_destroy", "vsom_ensemble_size", "vsom_ensemble_train_online_chunk_fetch",
    "vsom_ensemble_batch_epoch", "vsom_ensemble_upload_chunks", "vsom_ensemble_bmu_batch",
    "vsom_umatrix", "vsom_get_umatrix", "vsom_ensemble_umatrix", "vsom_similarity_batch",
    "vsom_bmu_masked_batch", "vsom_evaluate_batch", "vsom_generate_batch", "vsom_decode_nodes",
    "vsom_batch_epoch_masked", "vsom_batch_schedule", "vsom_ensemble_batch_schedule",
    "vsom_set_sigma_mode", "vsom_sigma_flush", "vsom_sigma_stats",
    "vsom_batch_accum_begin", "vsom_batch_accum_chunk", "vsom_batch_accum_end", "vsom_batch_accum_abort",
    "vsom_batch_accum_chunk_masked", "vsom_train_online_chunk_masked",
    "vsom_similarity_masked_batch", "vsom_evaluate_masked_batch",
    "vsom_bmd_masked_batch", "vsom_generate_masked_batch",
    "vsom_set_column_weights", "vsom_set_chunk_validity", "vsom_find_bmu_valid", "vsom_find_local_bmu_valid",
    "vsom_dist_single_valid", "vsom_train_single_valid",
    "vsom_bmu_topk_masked_batch",
    "vsom_batch_schedule_masked", "vsom_ensemble_batch_epoch_masked", "vsom_ensemble_batch_schedule_masked",
    "vsom_masked_tiny_applies",
    "vsom_online_masked_tiny_applies", "vsom_ensemble_train_online_chunk_masked",
    "vsom_ensemble_bmu_masked_batch", "vsom_ensemble_similarity_masked_batch",
    "vsom_ensemble_bmu_topk_batch", "vsom_ensemble_bmu_topk_masked_batch", "vsom_ensemble_topk_applies",
    "vsom_ensemble_evaluate_batch", "vsom_ensemble_evaluate_masked_batch", "vsom_ensemble_evaluate_applies",
]
SCHEDULE_MAX_EPOCHS = 1024     # VSOM_SCHEDULE_MAX_EPOCHS: the epochs of one launch of a schedule call


class SimilarityOut(C.Structure):
    """vsom_similarity_out: host pointers, each may be NULL"""
    _fields_ = [("bmu", C.POINTER(C.c_uint64)), ("dist", C.POINTER(C.c_float)), ("dmax", C.POINTER(C.c_float)),
                ("dmax_col", C.POINTER(C.c_uint32)), ("first", C.POINTER(C.c_float)), ("amax", C.POINTER(C.c_float)),
                ("amax_col", C.POINTER(C.c_uint32)), ("outside", C.POINTER(C.c_uint32)), ("delta", C.POINTER(C.c_float))]


class MaskedOut(C.Structure):
    """vsom_masked_out: host pointers, each may be NULL"""
    _fields_ = [("bmu", C.POINTER(C.c_uint64)), ("dist", C.POINTER(C.c_float)), ("nvalid", C.POINTER(C.c_uint32)),
                ("fill", C.POINTER(C.c_float))]


class EvaluateOut(C.Structure):
    """vsom_evaluate_out: host pointers, each may be NULL"""
    _fields_ = [("bmu", C.POINTER(C.c_uint64)), ("dist", C.POINTER(C.c_float)), ("bsum", C.POINTER(C.c_float)),
                ("nrepl", C.POINTER(C.c_uint32)), ("error", C.POINTER(C.c_double))]


class SimilarityMaskedOut(C.Structure):
    """vsom_similarity_masked_out: vsom_similarity_out's fields and nvalid; host pointers, each may be NULL"""
    _fields_ = SimilarityOut._fields_ + [("nvalid", C.POINTER(C.c_uint32))]


class EvaluateMaskedOut(C.Structure):
    """vsom_evaluate_masked_out: vsom_evaluate_out's fields and nvalid; host pointers, each may be NULL"""
    _fields_ = EvaluateOut._fields_ + [("nvalid", C.POINTER(C.c_uint32))]


class TopkMaskedOut(C.Structure):
    """vsom_topk_masked_out: host pointers; idx is required, the others may be NULL"""
    _fields_ = [("idx", C.POINTER(C.c_uint64)), ("dist", C.POINTER(C.c_float)), ("count", C.POINTER(C.c_uint32)),
                ("nvalid", C.POINTER(C.c_uint32)), ("blend", C.POINTER(C.c_double))]


class EnsembleTopkOut(C.Structure):
    """vsom_ensemble_topk_out: one member's host pointers; idx is required for a covered member, the others may be NULL"""
    _fields_ = TopkMaskedOut._fields_[:4]


class GenerateOut(C.Structure):
    """vsom_generate_out: host pointers, each may be NULL"""
    _fields_ = [("unit", C.POINTER(C.c_uint64)), ("record", C.POINTER(C.c_double))]


class VsomError(RuntimeError):
    pass


def has_contracted(transform):
    """whether vsom_set_update_mode(VSOM_UPDATE_FMA) changes the chain arithmetic of this transformation
    (include/vsom_hip.h, vsom_update_mode)"""
    return int(transform) == STANDARD      # Median (exact fused operations) and CLR have one arithmetic


def build(force=False):
    """Compile libvsom_hip.so for gfx950 with csrc/build.sh (hipcc cross-compiles on CPU)."""
    script = os.path.join(_HERE, "csrc", "build.sh")
    if force:
        for f in os.listdir(os.path.join(_HERE, "csrc")):
            if f.endswith(".o"):
                os.remove(os.path.join(_HERE, "csrc", f))
    subprocess.check_call(["bash", script, _INTREE], stdout=subprocess.DEVNULL)
    return _INTREE


def hip_runtimes():
    """paths of the libamdhip64 copies mapped into this process (/proc/self/maps)"""
    found = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                at = line.find("/")
                if at >= 0 and "libamdhip64.so" in line:
                    found.add(line[at:].strip())
    except OSError:
        pass
    return sorted(found)


def assert_single_hip_runtime(what):
    """PyTorch's wheel bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Loaded FIRST, it is the one copy
    libvsom_hip.so binds to as well; loaded AFTER libvsom_hip.so has pulled in /opt/rocm's, the process holds two HIP
    runtimes: torch streams / tensors handed to the library belong to the other runtime, and RCCL initialises against
    a runtime that never came up ("no ROCm-capable device is detected" in ncclCommInitAll).  Everything that mixes
    the two -- dist.HipEngine, Group, bench.py -- calls this and fails with the cause instead."""
    libs = hip_runtimes()
    if len(libs) > 1:
        raise VsomError(f"{what}: two HIP runtimes are mapped into this process ({', '.join(libs)}). "
                        "Import torch BEFORE the first vsom_amd call (tests/conftest.py and bench.py do), "
                        "so that libvsom_hip.so binds to the copy torch brings.")


_lib = None


def lib():
    """Load the HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VsomError(f"{LIB_PATH} is missing: run __graft_entry__.build() "
                        "(variational-self-organizing-maps_amd/csrc/build.sh)")
    L = C.CDLL(LIB_PATH)
    vp, fp, u64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    L.vsom_last_error.restype = C.c_char_p
    L.vsom_device_count.restype = C.c_int
    L.vsom_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.vsom_create_custom.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_char_p]
    L.vsom_custom_compile_check.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32]
    L.vsom_destroy.argtypes = [vp]
    L.vsom_destroy.restype = None
    L.vsom_set_stream.argtypes = [vp, vp]
    L.vsom_synchronize.argtypes = [vp]
    L.vsom_set_bmu_mode.argtypes = [vp, C.c_int]
    L.vsom_set_update_mode.argtypes = [vp, C.c_int]
    L.vsom_set_sigma_mode.argtypes = [vp, C.c_int]
    L.vsom_sigma_flush.argtypes = [vp]
    L.vsom_sigma_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.vsom_set_column_compaction.argtypes = [vp, C.c_long]
    L.vsom_set_row_dedupe.argtypes = [vp, C.c_double]
    L.vsom_get_shortlist_stats.argtypes = [vp, C.POINTER(C.c_uint32)]
    for name in ("vsom_depth", "vsom_nodes", "vsom_residual_len", "vsom_pitch", "vsom_chunk_pitch"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = C.c_uint32
    L.vsom_chunk_size.argtypes = [vp]
    L.vsom_chunk_size.restype = C.c_size_t
    L.vsom_enable_timing_of.argtypes = [vp, C.c_uint32]
    L.vsom_small_map_chains.argtypes = [vp, C.c_size_t]
    L.vsom_small_map_chains.restype = C.c_int
    L.vsom_set_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_get_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_upload_chunk.argtypes = [vp, fp, C.c_size_t]
    L.vsom_upload_chunk_async.argtypes = [vp, fp, C.c_size_t]
    L.vsom_set_chunk_device.argtypes = [vp, vp, C.c_size_t]
    L.vsom_host_alloc.argtypes = [C.POINTER(vp), C.c_size_t]
    L.vsom_host_free.argtypes = [vp]
    L.vsom_prefetch_chunk.argtypes = [vp, fp, C.c_size_t]
    L.vsom_prefetch_wait.argtypes = [vp]
    L.vsom_commit_chunk.argtypes = [vp]
    L.vsom_stage_next_device.argtypes = [vp, vp, C.c_size_t]
    L.vsom_get_last_bmu.argtypes = [vp, u64p]
    L.vsom_set_last_bmu.argtypes = [vp, u64p]
    L.vsom_get_sqres.argtypes = [vp, fp]
    L.vsom_bmu_batch.argtypes = [vp, u64p, fp]
    L.vsom_find_bmu.argtypes = [vp, fp, u64p, fp]
    L.vsom_bmu_local_batch.argtypes = [vp, u64p, fp]
    L.vsom_distances.argtypes = [vp, u64p, u64p, C.c_size_t, fp]
    L.vsom_bmu_restricted_batch.argtypes = [vp, C.c_uint64, u64p, fp]
    L.vsom_distances_row.argtypes = [vp, C.c_size_t, fp]
    dp = C.POINTER(C.c_double)
    L.vsom_bmd_batch.argtypes = [vp, C.c_uint64, C.c_size_t, C.c_size_t, dp, u64p, dp, dp]
    L.vsom_bmu_topk_batch.argtypes = [vp, C.c_uint32, C.c_size_t, C.c_size_t, u64p, fp]
    L.vsom_distances_raw.argtypes = [vp, u64p, u64p, C.c_size_t, C.c_int, fp]
    L.vsom_batch_phase1_async.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int]
    L.vsom_batch_finish_async.argtypes = [vp]
    L.vsom_batch_phase2_async.argtypes = [vp, C.c_double, C.c_size_t, C.c_size_t]
    L.vsom_batch_epoch_async.argtypes = [vp, C.c_double, C.c_int]
    L.vsom_batch_epoch.argtypes = [vp, C.c_double, C.c_int, fp]
    L.vsom_get_mse.argtypes = [vp, fp]
    L.vsom_train_single.argtypes = [vp, fp, C.c_double, C.c_double, u64p, C.c_int, fp, fp, u64p]
    L.vsom_get_online_search_stats.argtypes = [vp, u64p, C.c_int]
    L.vsom_dist_single.argtypes = [vp, fp, C.c_uint64, fp]
    L.vsom_find_local_bmu.argtypes = [vp, fp, C.c_uint64, u64p, fp]
    L.vsom_find_restricted_bmu.argtypes = [vp, fp, C.c_uint64, u64p, fp]
    L.vsom_distances_single.argtypes = [vp, fp, fp]
    L.vsom_train_online_chunk.argtypes = [vp, C.c_double, C.c_double, C.c_int, fp]
    L.vsom_train_online_chunk_acc.argtypes = [vp, C.c_double, C.c_double, C.c_int, C.c_int, fp]
    L.vsom_train_online_chunk_fetch.argtypes = [vp, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_uint64), fp]
    L.vsom_neighbourhood_weight.argtypes = [C.c_size_t] * 4 + [C.c_double]
    L.vsom_neighbourhood_weight.restype = C.c_double
    L.vsom_device_ptr.argtypes = [vp, C.c_int]
    L.vsom_device_ptr.restype = vp
    L.vsom_enable_timing.argtypes = [vp, C.c_int]
    L.vsom_get_timing.argtypes = [vp, fp, C.POINTER(C.c_uint32), C.c_int]
    L.vsom_group_create.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.vsom_group_destroy.argtypes = [vp]
    L.vsom_group_destroy.restype = None
    L.vsom_group_size.argtypes = [vp]
    L.vsom_group_ctx.argtypes = [vp, C.c_int]
    L.vsom_group_ctx.restype = vp
    L.vsom_group_transport.argtypes = [vp]
    L.vsom_group_transport.restype = C.c_char_p
    L.vsom_group_synchronize.argtypes = [vp]
    L.vsom_group_set_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_group_get_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_group_set_update_mode.argtypes = [vp, C.c_int]
    L.vsom_group_set_bmu_mode.argtypes = [vp, C.c_int]
    L.vsom_group_upload_chunk.argtypes = [vp, fp, C.c_size_t]
    L.vsom_group_prefetch_chunk.argtypes = [vp, fp, C.c_size_t]
    L.vsom_group_prefetch_wait.argtypes = [vp]
    L.vsom_group_commit_chunk.argtypes = [vp]
    L.vsom_group_set_chunk_device.argtypes = [vp, C.POINTER(vp), C.c_size_t]
    L.vsom_group_set_last_bmu.argtypes = [vp, u64p]
    L.vsom_group_get_last_bmu.argtypes = [vp, u64p]
    L.vsom_group_batch_epoch_async.argtypes = [vp, C.c_double, C.c_int]
    L.vsom_group_batch_epoch.argtypes = [vp, C.c_double, C.c_int, fp]
    L.vsom_group_get_mse.argtypes = [vp, fp]
    L.vsom_ensemble_create.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_size_t]
    L.vsom_ensemble_destroy.argtypes = [vp]
    L.vsom_ensemble_destroy.restype = None
    L.vsom_ensemble_size.argtypes = [vp]
    L.vsom_ensemble_size.restype = C.c_size_t
    L.vsom_ensemble_train_online_chunk_fetch.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                         C.POINTER(C.c_int), C.c_int, C.POINTER(u64p), fp]
    L.vsom_ensemble_batch_epoch.argtypes = [vp, C.POINTER(C.c_double), C.c_int, fp]
    L.vsom_ensemble_upload_chunks.argtypes = [vp, fp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_int]
    L.vsom_ensemble_bmu_batch.argtypes = [vp, C.POINTER(u64p), C.POINTER(fp)]
    L.vsom_umatrix.argtypes = [vp, dp]
    L.vsom_get_umatrix.argtypes = [vp, dp]
    L.vsom_ensemble_umatrix.argtypes = [vp, C.POINTER(dp)]
    if hasattr(L, "vsom_similarity_batch"):     # (VSOM_LIB may name an older build: tools/similarity_bench.py --route parent)
        L.vsom_similarity_batch.argtypes = [vp, C.c_uint64, C.c_int, C.c_int, C.c_size_t, C.c_size_t,
                                            C.POINTER(C.c_uint8), C.POINTER(SimilarityOut)]
    L.vsom_bmu_masked_batch.argtypes = [vp, C.c_uint64, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint8), C.c_int,
                                        C.POINTER(MaskedOut)]
    L.vsom_evaluate_batch.argtypes = [vp, C.c_size_t, C.c_size_t, fp, fp, C.POINTER(C.c_uint8), C.POINTER(EvaluateOut)]
    if hasattr(L, "vsom_generate_batch"):       # (VSOM_LIB may name an older build: tools/generate_bench.py --route parent)
        L.vsom_generate_batch.argtypes = [vp, C.c_uint64, C.c_int, C.c_size_t, C.c_size_t, dp, dp, C.POINTER(GenerateOut)]
        L.vsom_decode_nodes.argtypes = [vp, u64p, C.c_size_t, dp, dp]
    if hasattr(L, "vsom_batch_epoch_masked"):   # (VSOM_LIB may name an older build)
        L.vsom_batch_epoch_masked.argtypes = [vp, C.c_double, C.c_int, C.POINTER(C.c_uint8), C.c_int, fp]
    if hasattr(L, "vsom_batch_schedule"):
        L.vsom_batch_schedule.argtypes = [vp, dp, C.c_size_t, C.c_int, fp]
        L.vsom_ensemble_batch_schedule.argtypes = [vp, C.POINTER(dp), C.POINTER(C.c_size_t), C.c_int, C.POINTER(fp)]
    if hasattr(L, "vsom_batch_schedule_masked"):        # (VSOM_LIB may name an older build: tools/tiny_masked_bench.py --lib)
        u8p = C.POINTER(C.c_uint8)
        L.vsom_batch_schedule_masked.argtypes = [vp, dp, C.c_size_t, C.c_int, u8p, C.c_int, fp]
        L.vsom_ensemble_batch_epoch_masked.argtypes = [vp, dp, C.c_int, C.POINTER(u8p), C.POINTER(C.c_int), fp]
        L.vsom_ensemble_batch_schedule_masked.argtypes = [vp, C.POINTER(dp), C.POINTER(C.c_size_t), C.c_int, C.POINTER(u8p),
                                                          C.POINTER(C.c_int), C.POINTER(fp)]
        L.vsom_masked_tiny_applies.argtypes = [vp, C.c_int]
    if hasattr(L, "vsom_batch_accum_begin"):    # (VSOM_LIB may name an older build: tools/accum_bench.py --lib)
        L.vsom_batch_accum_begin.argtypes = [vp, C.c_double, C.c_int, C.c_size_t]
        L.vsom_batch_accum_chunk.argtypes = [vp]
        L.vsom_batch_accum_end.argtypes = [vp, fp]
        L.vsom_batch_accum_abort.argtypes = [vp]
    if hasattr(L, "vsom_train_online_chunk_masked"):    # (VSOM_LIB may name an older build: tools/online_masked_bench.py --lib)
        L.vsom_train_online_chunk_masked.argtypes = [vp, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int,
                                                     C.POINTER(C.c_uint64), fp]
    if hasattr(L, "vsom_online_masked_tiny_applies"):   # (VSOM_LIB may name an older build: tools/online_tiny_masked_bench.py --lib)
        u8p = C.POINTER(C.c_uint8)
        L.vsom_online_masked_tiny_applies.argtypes = [vp, C.c_double, C.c_int]
        L.vsom_ensemble_train_online_chunk_masked.argtypes = [vp, dp, dp, C.POINTER(C.c_int), C.c_int, C.POINTER(u8p),
                                                              C.POINTER(C.c_int), C.POINTER(u64p), fp]
    if hasattr(L, "vsom_batch_accum_chunk_masked"):     # (VSOM_LIB may name an older build: tools/accum_masked_bench.py --lib)
        L.vsom_batch_accum_chunk_masked.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int]
    if hasattr(L, "vsom_similarity_masked_batch"):      # (VSOM_LIB may name an older build: tools/masked_score_bench.py --lib)
        L.vsom_similarity_masked_batch.argtypes = [vp, C.c_uint64, C.c_int, C.c_int, C.c_size_t, C.c_size_t,
                                                   C.POINTER(C.c_uint8), C.c_int, C.POINTER(SimilarityMaskedOut)]
        L.vsom_evaluate_masked_batch.argtypes = [vp, C.c_uint64, C.c_size_t, C.c_size_t, fp, fp, C.POINTER(C.c_uint8), C.c_int,
                                                 C.POINTER(EvaluateMaskedOut)]
    if hasattr(L, "vsom_bmd_masked_batch"):             # (VSOM_LIB may name an older build: tools/bmd_masked_bench.py --lib)
        L.vsom_bmd_masked_batch.argtypes = [vp, C.c_uint64, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint8), C.c_int, dp, u64p,
                                            dp, dp]
        L.vsom_generate_masked_batch.argtypes = [vp, C.c_uint64, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint8), C.c_int,
                                                 C.c_uint32, C.c_int, dp, dp, C.POINTER(GenerateOut)]
    if hasattr(L, "vsom_set_chunk_validity"):           # (VSOM_LIB may name an older build: tools/custom_validity_bench.py --lib)
        u8p = C.POINTER(C.c_uint8)
        L.vsom_set_column_weights.argtypes = [vp, fp]
        L.vsom_set_chunk_validity.argtypes = [vp, u8p, C.c_int]
        L.vsom_find_bmu_valid.argtypes = [vp, fp, u8p, u64p, fp]
        L.vsom_find_local_bmu_valid.argtypes = [vp, fp, u8p, C.c_uint64, u64p, fp]
        L.vsom_dist_single_valid.argtypes = [vp, fp, u8p, C.c_uint64, fp]
        L.vsom_train_single_valid.argtypes = [vp, fp, u8p, C.c_double, C.c_double, u64p, C.c_int, fp, fp, u64p]
    if hasattr(L, "vsom_bmu_topk_masked_batch"):        # (VSOM_LIB may name an older build: tools/topk_masked_bench.py --lib)
        L.vsom_bmu_topk_masked_batch.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint8),
                                                 C.c_int, C.POINTER(TopkMaskedOut)]
    if hasattr(L, "vsom_ensemble_bmu_masked_batch"):    # (VSOM_LIB may name an older build: tools/ensemble_masked_query_bench.py --lib)
        u8p = C.POINTER(C.c_uint8)
        L.vsom_ensemble_bmu_masked_batch.argtypes = [vp, u64p, C.POINTER(u8p), C.POINTER(C.c_int), C.POINTER(MaskedOut)]
        L.vsom_ensemble_similarity_masked_batch.argtypes = [vp, u64p, C.POINTER(C.c_int), C.c_int, C.POINTER(u8p),
                                                            C.POINTER(C.c_int), C.POINTER(SimilarityMaskedOut)]
    if hasattr(L, "vsom_ensemble_bmu_topk_batch"):      # (VSOM_LIB may name an older build: tools/ensemble_topk_bench.py --lib)
        u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
        L.vsom_ensemble_bmu_topk_batch.argtypes = [vp, u32p, C.POINTER(EnsembleTopkOut)]
        L.vsom_ensemble_bmu_topk_masked_batch.argtypes = [vp, u32p, u64p, C.POINTER(u8p), C.POINTER(C.c_int),
                                                          C.POINTER(EnsembleTopkOut)]
        L.vsom_ensemble_topk_applies.argtypes = [vp, C.c_size_t, C.c_uint32, C.c_int]
    if hasattr(L, "vsom_ensemble_evaluate_batch"):      # (VSOM_LIB may name an older build: tools/ensemble_evaluate_bench.py --lib)
        u8p = C.POINTER(C.c_uint8)
        L.vsom_ensemble_evaluate_batch.argtypes = [vp, C.POINTER(fp), C.POINTER(fp), C.POINTER(u8p), C.POINTER(EvaluateOut)]
        L.vsom_ensemble_evaluate_masked_batch.argtypes = [vp, u64p, C.POINTER(fp), C.POINTER(fp), C.POINTER(u8p),
                                                          C.POINTER(C.c_int), C.POINTER(EvaluateMaskedOut)]
        L.vsom_ensemble_evaluate_applies.argtypes = [vp, C.c_size_t, C.c_int]
    _lib = L
    return L


def _f(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _u(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint64))


def check(rc):
    if rc != 0:
        raise VsomError(f"libvsom_hip error {rc}: {lib().vsom_last_error().decode(errors='replace')}")


def device_count():
    return int(lib().vsom_device_count())


def custom_compile_check(source, depth, residual_len):
    """compile a hook source (include/vsom_hip.h, vsom_create_custom) for gfx950 without opening a device; raises
    VsomError with the hipRTC log when it does not compile"""
    check(lib().vsom_custom_compile_check(source.encode(), int(depth), int(residual_len)))


def model_length(transform, in_len):
    """Transformation::Length (Transformation.cpp:33-36,71-74,162-165): J, or J(J-1) for CLR."""
    return int(in_len) * (int(in_len) - 1) if int(transform) == CLR else int(in_len)


def neighbourhood_weight(cx, cy, bx, by, sigma):
    return float(lib().vsom_neighbourhood_weight(cx, cy, bx, by, float(sigma)))


class PinnedBuffer:
    """Pinned host memory (vsom_host_alloc) exposed as a numpy float32 array."""

    def __init__(self, shape):
        self.shape = tuple(int(v) for v in shape)
        n = int(np.prod(self.shape))
        self._p = C.c_void_p()
        check(lib().vsom_host_alloc(C.byref(self._p), max(n, 1) * 4))
        buf = (C.c_float * max(n, 1)).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=np.float32, count=n).reshape(self.shape)

    def free(self):
        if self._p:
            self.array = None
            lib().vsom_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """RAII wrapper of a vsom_ctx (one per GPU)."""

    def __init__(self, width, height, in_len, transform=STANDARD, device=0, _borrowed=None, source=None, depth=None,
                 residual_len=None):
        """transform=CUSTOM: `source` defines vsom_compare / vsom_step, `depth` and `residual_len` their lengths"""
        self._owned = _borrowed is None
        if _borrowed is None:
            self._h = C.c_void_p()
            if int(transform) == CUSTOM:
                check(lib().vsom_create_custom(C.byref(self._h), int(device), int(width), int(height), int(in_len),
                                               int(depth), int(residual_len), source.encode()))
            else:
                check(lib().vsom_create(C.byref(self._h), int(device), int(width), int(height), int(in_len),
                                        int(transform)))
        else:
            self._h = C.c_void_p(_borrowed)       # a member of a Group: the group owns it
        self.width, self.height, self.in_len = int(width), int(height), int(in_len)
        self.transform, self.device = int(transform), int(device)
        self.depth = int(lib().vsom_depth(self._h))
        self.n_nodes = int(lib().vsom_nodes(self._h))
        self.residual_len = int(lib().vsom_residual_len(self._h))
        self.pitch = int(lib().vsom_pitch(self._h))

    def close(self):
        if self._h:
            if self._owned:
                lib().vsom_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- plumbing ------------------------------------------------------
    def set_stream(self, hip_stream_ptr):
        check(lib().vsom_set_stream(self._h, C.c_void_p(hip_stream_ptr or 0)))

    def synchronize(self):
        check(lib().vsom_synchronize(self._h))

    def set_bmu_mode(self, mode):
        check(lib().vsom_set_bmu_mode(self._h, int(mode)))

    def set_update_mode(self, mode):
        check(lib().vsom_set_update_mode(self._h, int(mode)))

    def set_sigma_mode(self, mode):
        """SIGMA_AUTO / SIGMA_EAGER / SIGMA_LAZY: when a whole-map batch epoch writes sigmaMap (vsom_set_sigma_mode)"""
        check(lib().vsom_set_sigma_mode(self._h, int(mode)))

    def sigma_flush(self):
        check(lib().vsom_sigma_flush(self._h))

    def sigma_stats(self):
        out = (C.c_uint64 * 4)()
        check(lib().vsom_sigma_stats(self._h, out))
        return {"deferred": int(out[0]), "dropped": int(out[1]), "materialised": int(out[2]), "pending": bool(out[3])}

    def set_row_dedupe(self, min_work):
        """exact searches of at least min_work (sample, node, value) triples evaluate one representative per class of
        bit-identical model rows (default 2e10; 0: always; < 0: never)"""
        check(lib().vsom_set_row_dedupe(self._h, float(min_work)))

    def set_column_compaction(self, min_rows):
        """chunks of at least min_rows rows retire their all-zero columns (default 1024; < 0: off)"""
        check(lib().vsom_set_column_compaction(self._h, int(min_rows)))

    def shortlist_stats(self):
        out = (C.c_uint32 * 4)()
        check(lib().vsom_get_shortlist_stats(self._h, out))
        return {"redo_samples": int(out[0]), "candidates": int(out[1]), "samples": int(out[2]),
                "searches": int(out[3])}

    def device_ptr(self, which):
        return int(lib().vsom_device_ptr(self._h, int(which)) or 0)

    @property
    def chunk_size(self):
        return int(lib().vsom_chunk_size(self._h))

    # ---- state ---------------------------------------------------------
    def set_state(self, map=None, sigma=None, S=None, weight=None, hits=None):
        n, d = self.n_nodes, self.depth

        def f2(a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32)
            assert a.size == int(np.prod(shape)), (a.shape, shape)
            return a

        m, s, ss, w = f2(map, (n, d)), f2(sigma, (n, d)), f2(S, (n, d)), f2(weight, (n,))
        h = None if hits is None else np.ascontiguousarray(hits, dtype=np.uint64)
        check(lib().vsom_set_state(self._h, _f(m), _f(s), _f(ss), _f(w), _u(h)))

    def get_state(self, map=True, sigma=True, S=True, weight=True, hits=True):
        n, d = self.n_nodes, self.depth
        m = np.empty((n, d), np.float32) if map else None
        s = np.empty((n, d), np.float32) if sigma else None
        ss = np.empty((n, d), np.float32) if S else None
        w = np.empty(n, np.float32) if weight else None
        h = np.empty(n, np.uint64) if hits else None
        check(lib().vsom_get_state(self._h, _f(m), _f(s), _f(ss), _f(w), _u(h)))
        return {"map": m, "sigma": s, "S": ss, "weight": w, "hits": h}

    # ---- chunk ---------------------------------------------------------
    def upload_chunk(self, X):
        X = np.ascontiguousarray(X, dtype=np.float32)
        assert X.ndim == 2 and X.shape[1] == self.in_len, (X.shape, self.in_len)
        check(lib().vsom_upload_chunk(self._h, _f(X), X.shape[0]))

    def upload_chunk_async(self, X_pinned):
        """copy + staging enqueued, no wait: X_pinned (a PinnedBuffer's array) must stay unchanged until a synchronising call"""
        assert X_pinned.ndim == 2 and X_pinned.shape[1] == self.in_len and X_pinned.dtype == np.float32
        check(lib().vsom_upload_chunk_async(self._h, _f(X_pinned), X_pinned.shape[0]))

    def set_chunk_device(self, dev_ptr, B):
        check(lib().vsom_set_chunk_device(self._h, C.c_void_p(int(dev_ptr)), int(B)))

    def prefetch_chunk(self, X):
        """Start the H2D copy of the NEXT chunk (async when X lives in pinned memory, see
        pinned_array); the current chunk keeps training."""
        assert X.dtype == np.float32 and X.flags.c_contiguous and X.ndim == 2 and X.shape[1] == self.in_len
        check(lib().vsom_prefetch_chunk(self._h, _f(X), X.shape[0]))

    def prefetch_wait(self):
        check(lib().vsom_prefetch_wait(self._h))

    def commit_chunk(self):
        check(lib().vsom_commit_chunk(self._h))

    def stage_next_device(self, dev_ptr, n_rows):
        """a next chunk that already lives in HBM: staged beside the running epoch when possible, adopted by
        commit_chunk (the rows must stay valid until then)"""
        check(lib().vsom_stage_next_device(self._h, C.c_void_p(int(dev_ptr) or None), int(n_rows)))

    def get_last_bmu(self):
        out = np.empty(self.chunk_size, np.uint64)
        check(lib().vsom_get_last_bmu(self._h, _u(out)))
        return out

    def set_last_bmu(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        assert idx.size == self.chunk_size
        check(lib().vsom_set_last_bmu(self._h, _u(idx)))

    def get_sqres(self):
        out = np.empty(self.chunk_size, np.float32)
        check(lib().vsom_get_sqres(self._h, _f(out)))
        return out

    # ---- search --------------------------------------------------------
    def bmu_batch(self):
        B = self.chunk_size
        idx, dist = np.empty(B, np.uint64), np.empty(B, np.float32)
        check(lib().vsom_bmu_batch(self._h, _u(idx), _f(dist)))
        return idx, dist

    def set_column_weights(self, w):
        """custom contexts: the column weights of the hooks' value_weight (None = all 1); they hold until set again"""
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float32)
            if w.shape != (self.in_len,):
                raise ValueError(f"weights have shape {w.shape}, not ({self.in_len},)")
        check(lib().vsom_set_column_weights(self._h, _f(w)))

    def set_chunk_validity(self, valid, one_mask=False):
        """custom contexts: the loaded chunk's validity for the hooks' value_weight -- B x J (nonzero = valid), or J values
        for every row with one_mask; None = all valid.  The next chunk resets it."""
        if valid is None:
            check(lib().vsom_set_chunk_validity(self._h, None, 0))
            return
        vb = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
        want = (self.in_len,) if one_mask else (self.chunk_size, self.in_len)
        if vb.shape != want:
            raise ValueError(f"valid has shape {vb.shape}, not {want}")
        check(lib().vsom_set_chunk_validity(self._h, vb.ctypes.data_as(C.POINTER(C.c_uint8)), 1 if one_mask else 0))

    def _vector_valid(self, valid):
        vb = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
        if vb.shape != (self.in_len,):
            raise ValueError(f"valid has shape {vb.shape}, not ({self.in_len},)")
        return vb, vb.ctypes.data_as(C.POINTER(C.c_uint8))

    def dist_single(self, v, node, valid=None):
        """Som::euclidianWeightedDist(node, v) of one host vector (does not disturb the staged chunk); valid= (custom
        contexts): the vector's validity for the hooks' value_weight."""
        v = np.ascontiguousarray(v, dtype=np.float32)
        assert v.shape == (self.in_len,)
        d = C.c_float()
        if valid is not None:
            vb, vp = self._vector_valid(valid)
            check(lib().vsom_dist_single_valid(self._h, _f(v), vp, int(node), C.byref(d)))
        else:
            check(lib().vsom_dist_single(self._h, _f(v), int(node), C.byref(d)))
        return np.float32(d.value)

    def find_local_bmu(self, v, last_bmu, valid=None):
        """Som::findLocalBmu of one host vector from `last_bmu`: (index, distance); valid= as in dist_single."""
        v = np.ascontiguousarray(v, dtype=np.float32)
        assert v.shape == (self.in_len,)
        idx, d = C.c_uint64(), C.c_float()
        if valid is not None:
            vb, vp = self._vector_valid(valid)
            check(lib().vsom_find_local_bmu_valid(self._h, _f(v), vp, int(last_bmu), C.byref(idx), C.byref(d)))
        else:
            check(lib().vsom_find_local_bmu(self._h, _f(v), int(last_bmu), C.byref(idx), C.byref(d)))
        return int(idx.value), np.float32(d.value)

    def find_restricted_bmu(self, v, min_hits):
        """Som::findRestrictedBmu of one host vector: (index, distance)."""
        v = np.ascontiguousarray(v, dtype=np.float32)
        assert v.shape == (self.in_len,)
        idx, d = C.c_uint64(), C.c_float()
        check(lib().vsom_find_restricted_bmu(self._h, _f(v), int(min_hits), C.byref(idx), C.byref(d)))
        return int(idx.value), np.float32(d.value)

    def distances_single(self, v):
        """euclidianWeightedDist(i, v) of one host vector to every node."""
        v = np.ascontiguousarray(v, dtype=np.float32)
        assert v.shape == (self.in_len,)
        out = np.empty(self.n_nodes, np.float32)
        check(lib().vsom_distances_single(self._h, _f(v), _f(out)))
        return out

    def find_bmu(self, v, valid=None):
        """Som::findBmu of one host vector (does not disturb the staged chunk); valid= as in dist_single."""
        v = np.ascontiguousarray(v, dtype=np.float32)
        assert v.size == self.in_len
        idx, dist = C.c_uint64(), C.c_float()
        if valid is not None:
            vb, vp = self._vector_valid(valid)
            check(lib().vsom_find_bmu_valid(self._h, _f(v), vp, C.byref(idx), C.byref(dist)))
        else:
            check(lib().vsom_find_bmu(self._h, _f(v), C.byref(idx), C.byref(dist)))
        return int(idx.value), np.float32(dist.value)

    def bmu_local_batch(self):
        B = self.chunk_size
        idx, dist = np.empty(B, np.uint64), np.empty(B, np.float32)
        check(lib().vsom_bmu_local_batch(self._h, _u(idx), _f(dist)))
        return idx, dist

    def distances(self, nodes, rows):
        nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        assert nodes.size == rows.size
        out = np.empty(nodes.size, np.float32)
        check(lib().vsom_distances(self._h, _u(nodes), _u(rows), nodes.size, _f(out)))
        return out

    def bmu_restricted_batch(self, min_hits):
        B = self.chunk_size
        idx, dist = np.empty(B, np.uint64), np.empty(B, np.float32)
        check(lib().vsom_bmu_restricted_batch(self._h, int(min_hits), _u(idx), _f(dist)))
        return idx, dist

    def restricted_bmd(self, min_hits, r0=0, r1=None, u=None, probs=False):
        """Som::findRestrictedBmd of chunk rows [r0, r1) in one call (vsom_bmd_batch): {"norm": C per row (float64),
        "draw": the node drawn with uniform u[r] per row (uint64, UINT64_MAX = no mass; None without u), "prob":
        float64[rows, N] (None unless probs)}.  Reads nothing but the map, the hits and the staged rows."""
        r1 = self.chunk_size if r1 is None else int(r1)
        n = max(r1 - int(r0), 0)
        norm = np.empty(n, np.float64)
        draw = prob = None
        up = None
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64)
            assert u.shape == (n,), (u.shape, n)
            up = u.ctypes.data_as(C.POINTER(C.c_double))
            draw = np.empty(n, np.uint64)
        if probs:
            prob = np.empty((n, self.n_nodes), np.float64)
        dp = C.POINTER(C.c_double)
        check(lib().vsom_bmd_batch(self._h, int(min_hits), int(r0), r1, up, _u(draw), norm.ctypes.data_as(dp),
                                   None if prob is None else prob.ctypes.data_as(dp)))
        return {"norm": norm, "draw": draw, "prob": prob}

    def bmu_topk(self, k, r0=0, r1=None, dist=True):
        """The k best matching units of chunk rows [r0, r1) in one call (vsom_bmu_topk_batch): (idx uint64[n, k],
        dist float32[n, k] or None).  Entry 0 is vsom_bmu_batch's BMU; the others follow in (distance, index) order.
        Read-only."""
        k = int(k)
        B = self.chunk_size
        r0 = int(r0)
        r1 = B if r1 is None else int(r1)
        if not 1 <= k <= min(64, self.n_nodes):
            raise ValueError(f"k = {k} is not in [1, min(64, N = {self.n_nodes})]")
        if r0 < 0 or r0 > r1 or r1 > B:
            raise ValueError(f"row range [{r0}, {r1}) is not within the chunk's {B} rows")
        n = r1 - r0
        idx = np.empty((n, k), np.uint64)
        d = np.empty((n, k), np.float32) if dist else None
        check(lib().vsom_bmu_topk_batch(self._h, k, r0, r1, _u(idx), None if d is None else _f(d)))
        return idx, d

    def similarity(self, min_hits, num_sigmas, sigma_rule=SIGMA_FLOOR, r0=0, r1=None, valid=None, delta=False):
        """Som::measureSimilarity's per-row report of chunk rows [r0, r1) in one call (vsom_similarity_batch): every row
        searched (findRestrictedBmu; findBmu's path when min_hits is 0) and scored against its BMU.  A dict of arrays
        with one entry per row: bmu (uint64), dist, dmax, first, amax (float32), dmax_col, amax_col, outside (uint32),
        and delta (float32[rows, min(J, D)], None unless delta=True).  valid: None, or rows x J, nonzero = the column
        counts for amax / outside.  Overwrites the chunk's lastBMU / sqres like bmu_restricted_batch."""
        B = self.chunk_size
        r0 = int(r0)
        r1 = B if r1 is None else int(r1)
        if int(sigma_rule) not in (SIGMA_AS_WRITTEN, SIGMA_FLOOR):
            raise ValueError(f"sigma_rule = {sigma_rule} is neither SIGMA_AS_WRITTEN nor SIGMA_FLOOR")
        if int(min_hits) < 0:
            raise ValueError("min_hits must be >= 0")
        if not -2 ** 31 <= int(num_sigmas) < 2 ** 31:
            raise ValueError("num_sigmas must fit an int")
        if r0 < 0 or r0 > r1 or r1 > B:
            raise ValueError(f"row range [{r0}, {r1}) is not within the chunk's {B} rows")
        n = r1 - r0
        vb = None
        if valid is not None:
            vb = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
            if vb.shape != (n, self.in_len):
                raise ValueError(f"valid has shape {vb.shape}, not ({n}, {self.in_len})")
        cols = min(self.in_len, self.depth)
        res = {"bmu": np.empty(n, np.uint64), "dist": np.empty(n, np.float32), "dmax": np.empty(n, np.float32),
               "dmax_col": np.empty(n, np.uint32), "first": np.empty(n, np.float32), "amax": np.empty(n, np.float32),
               "amax_col": np.empty(n, np.uint32), "outside": np.empty(n, np.uint32),
               "delta": np.empty((n, cols), np.float32) if delta else None}
        out = SimilarityOut()
        for name, ctype in SimilarityOut._fields_:
            if res[name] is not None:
                setattr(out, name, res[name].ctypes.data_as(ctype))
        check(lib().vsom_similarity_batch(self._h, int(min_hits), int(num_sigmas), int(sigma_rule), r0, r1,
                                          None if vb is None else vb.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(out)))
        return res

    def evaluate(self, binary, continuous, valid=None, r0=0, r1=None):
        """Som::evaluate of chunk rows [r0, r1) in one call (vsom_evaluate_batch): every row searched (findBmu, as
        bmu_batch) and its binary error scored against its BMU.  binary, continuous: J column factors each.  valid: None,
        or rows x J, nonzero = valid.  A dict: bmu (uint64), dist, bsum (float32), nrepl (uint32) with one entry per row,
        and error (float), the running mean of dist + sqrt(bsum) over the rows.  Overwrites the chunk's lastBMU / sqres
        like bmu_batch."""
        B = self.chunk_size
        r0 = int(r0)
        r1 = B if r1 is None else int(r1)
        if r0 < 0 or r0 > r1 or r1 > B:
            raise ValueError(f"row range [{r0}, {r1}) is not within the chunk's {B} rows")
        n = r1 - r0
        cols = []
        for name, a in (("binary", binary), ("continuous", continuous)):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != (self.in_len,):
                raise ValueError(f"{name} has shape {a.shape}, not ({self.in_len},)")
            cols.append(a)
        vb = None
        if valid is not None:
            vb = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
            if vb.shape != (n, self.in_len):
                raise ValueError(f"valid has shape {vb.shape}, not ({n}, {self.in_len})")
        res = {"bmu": np.empty(n, np.uint64), "dist": np.empty(n, np.float32), "bsum": np.empty(n, np.float32),
               "nrepl": np.empty(n, np.uint32), "error": np.zeros(1, np.float64)}
        out = EvaluateOut()
        for name, ctype in EvaluateOut._fields_:
            setattr(out, name, res[name].ctypes.data_as(ctype))
        check(lib().vsom_evaluate_batch(self._h, r0, r1, _f(cols[0]), _f(cols[1]),
                                        None if vb is None else vb.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(out)))
        res["error"] = float(res["error"][0])
        return res

    def _logits(self, l, n):
        cols = min(self.in_len, self.depth)
        if cols == 0:
            raise ValueError("the records have no columns")
        l = np.ascontiguousarray(l, dtype=np.float64)
        if l.shape != (n, cols):
            raise ValueError(f"l has shape {l.shape}, not ({n}, {cols})")
        return l, cols

    def generate(self, min_hits, u, l, rule=GENERATE_PER_ROW, r0=0, r1=None):
        """Som::autoEncoder's records of chunk rows [r0, r1) in one call (vsom_generate_batch): a unit per row drawn from a
        restricted best matching distribution with the uniform u[r] in [0, 1) -- the row's own (GENERATE_PER_ROW:
        restricted_bmd's draw) or that of the chunk's last row (GENERATE_AS_WRITTEN, what the reference does) -- and every
        column sampled as log(l / (1 - l)) / 1.6 * sigma + mean around that unit, l: float64[rows, min(J, D)].  A dict:
        unit (uint64, NO_UNIT = no mass) and record (float64[rows, min(J, D)], NaN in a row without mass).  Read-only."""
        B = self.chunk_size
        r0 = int(r0)
        r1 = B if r1 is None else int(r1)
        if int(rule) not in (GENERATE_AS_WRITTEN, GENERATE_PER_ROW):
            raise ValueError(f"rule = {rule} is neither GENERATE_AS_WRITTEN nor GENERATE_PER_ROW")
        if int(min_hits) < 0:
            raise ValueError("min_hits must be >= 0")
        if r0 < 0 or r0 > r1 or r1 > B:
            raise ValueError(f"row range [{r0}, {r1}) is not within the chunk's {B} rows")
        n = r1 - r0
        u = np.ascontiguousarray(u, dtype=np.float64)
        if u.shape != (n,):
            raise ValueError(f"u has shape {u.shape}, not ({n},)")
        if not ((u >= 0.0) & (u < 1.0)).all():
            raise ValueError("every uniform must lie in [0, 1)")
        l, cols = self._logits(l, n)
        res = {"unit": np.empty(n, np.uint64), "record": np.empty((n, cols), np.float64)}
        out = GenerateOut()
        for name, ctype in GenerateOut._fields_:
            setattr(out, name, res[name].ctypes.data_as(ctype))
        dp = C.POINTER(C.c_double)
        check(lib().vsom_generate_batch(self._h, int(min_hits), int(rule), r0, r1, u.ctypes.data_as(dp), l.ctypes.data_as(dp),
                                        C.byref(out)))
        return res

    def decode_nodes(self, nodes, l):
        """generate's decode for given units (vsom_decode_nodes): float64[len(nodes), min(J, D)], row i sampled around unit
        nodes[i] with l[i].  Needs no chunk.  Read-only."""
        a = np.asarray(nodes)
        if a.ndim != 1:
            raise ValueError(f"nodes has shape {a.shape}, not one dimension")
        if a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) >= self.n_nodes):
            raise ValueError(f"every node must be an integer in [0, {self.n_nodes})")
        a = np.ascontiguousarray(a, dtype=np.uint64)
        l, cols = self._logits(l, a.size)
        rec = np.empty((a.size, cols), np.float64)
        dp = C.POINTER(C.c_double)
        check(lib().vsom_decode_nodes(self._h, _u(a), a.size, l.ctypes.data_as(dp), rec.ctypes.data_as(dp)))
        return rec

    def bmu_masked(self, valid, r0=0, r1=None, min_hits=0, fill=False):
        """The best matching unit of chunk rows [r0, r1) over their valid columns only (vsom_bmu_masked_batch; Standard /
        Median): findRestrictedBmu on the distance whose residual is +0 at invalid columns.  valid: rows x J (nonzero =
        valid), or a 1-D column mask of J entries applied to every row.  A dict of arrays with one entry per row: bmu
        (uint64), dist (float32), nvalid (uint32), and fill (float32[rows, J]: x where valid, the unit's value where not;
        None unless fill=True).  Read-only."""
        B = self.chunk_size
        r0 = int(r0)
        r1 = B if r1 is None else int(r1)
        if int(min_hits) < 0:
            raise ValueError("min_hits must be >= 0")
        if r0 < 0 or r0 > r1 or r1 > B:
            raise ValueError(f"row range [{r0}, {r1}) is not within the chunk's {B} rows")
        n = r1 - r0
        vb = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
        one = vb.ndim == 1
        if vb.shape != ((self.in_len,) if one else (n, self.in_len)):
            raise ValueError(f"valid has shape {vb.shape}, neither ({self.in_len},) nor ({n}, {self.in_len})")
        res = {"bmu": np.empty(n, np.uint64), "dist": np.empty(n, np.float32), "nvalid": np.empty(n, np.uint32),
               "fill": np.empty((n, self.in_len), np.float32) if fill else None}
        out = MaskedOut()
        for name, ctype in MaskedOut._fields_:
            if res[name] is not None:
                setattr(out, name, res[name].ctypes.data_as(ctype))
        check(lib().vsom_bmu_masked_batch(self._h, int(min_hits), r0, r1, vb.ctypes.data_as(C.POINTER(C.c_uint8)), int(one),
                                          C.byref(out)))
        return res

    def bmu_topk_masked(self, k, valid, r0=0, r1=None, min_hits=0, dist=True, blend=False):
        """The k best matching units of chunk rows [r0, r1) over their valid columns only (vsom_bmu_topk_masked_batch;
        Standard / Median): bmu_topk on bmu_masked's distance, over findRestrictedBmu's candidates (node 0, and the nodes
        with at least min_hits hits).  valid: rows x J (nonzero = valid), or a 1-D column mask of J entries applied to every
        row.  A dict of arrays: idx (uint64[n, k]; entry 0 is bmu_masked's unit), dist (float32[n, k], None unless dist),
        count (uint32[n]: the real entries of the row -- a row with fewer than k candidates is padded with idx = NO_UNIT,
        dist = NaN), nvalid (uint32[n]) and blend (float64[n, J]: x where valid, elsewhere the k units' values weighted as
        the BMD weights units; None unless blend).  Read-only."""
        k = int(k)
        B = self.chunk_size
        r0 = int(r0)
        r1 = B if r1 is None else int(r1)
        if not 1 <= k <= min(64, self.n_nodes):
            raise ValueError(f"k = {k} is not in [1, min(64, N = {self.n_nodes})]")
        if int(min_hits) < 0:
            raise ValueError("min_hits must be >= 0")
        if r0 < 0 or r0 > r1 or r1 > B:
            raise ValueError(f"row range [{r0}, {r1}) is not within the chunk's {B} rows")
        n = r1 - r0
        vb, one = self._mask_bytes(valid, n)
        res = {"idx": np.empty((n, k), np.uint64), "dist": np.empty((n, k), np.float32) if dist else None,
               "count": np.empty(n, np.uint32), "nvalid": np.empty(n, np.uint32),
               "blend": np.empty((n, self.in_len), np.float64) if blend else None}
        out = TopkMaskedOut()
        for name, ctype in TopkMaskedOut._fields_:
            if res[name] is not None:
                setattr(out, name, res[name].ctypes.data_as(ctype))
        check(lib().vsom_bmu_topk_masked_batch(self._h, k, int(min_hits), r0, r1, vb.ctypes.data_as(C.POINTER(C.c_uint8)),
                                               int(one), C.byref(out)))
        return res

    def _mask_bytes(self, valid, n):
        """valid as the masked calls take it: (bytes, one_mask) from rows x J (nonzero = valid) or a 1-D column mask"""
        vb = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
        one = vb.ndim == 1
        if vb.shape != ((self.in_len,) if one else (n, self.in_len)):
            raise ValueError(f"valid has shape {vb.shape}, neither ({self.in_len},) nor ({n}, {self.in_len})")
        return vb, one

    def similarity_masked(self, valid, min_hits, num_sigmas, sigma_rule=SIGMA_FLOOR, r0=0, r1=None, delta=False):
        """similarity for records with missing fields (vsom_similarity_masked_batch; Standard / Median): chunk rows
        [r0, r1) searched over their valid columns only, as bmu_masked, and scored against that unit in those columns.
        valid: rows x J (nonzero = valid), or a 1-D column mask of J entries applied to every row.  similarity's dict
        (dmax / first over the valid columns only, delta 0 at invalid ones) and nvalid (uint32).  Read-only: lastBMU and
        sqres stay."""
        B = self.chunk_size
        r0 = int(r0)
        r1 = B if r1 is None else int(r1)
        if int(sigma_rule) not in (SIGMA_AS_WRITTEN, SIGMA_FLOOR):
            raise ValueError(f"sigma_rule = {sigma_rule} is neither SIGMA_AS_WRITTEN nor SIGMA_FLOOR")
        if int(min_hits) < 0:
            raise ValueError("min_hits must be >= 0")
        if not -2 ** 31 <= int(num_sigmas) < 2 ** 31:
            raise ValueError("num_sigmas must fit an int")
        if r0 < 0 or r0 > r1 or r1 > B:
            raise ValueError(f"row range [{r0}, {r1}) is not within the chunk's {B} rows")
        n = r1 - r0
        vb, one = self._mask_bytes(valid, n)
        res = {"bmu": np.empty(n, np.uint64), "dist": np.empty(n, np.float32), "dmax": np.empty(n, np.float32),
               "dmax_col": np.empty(n, np.uint32), "first": np.empty(n, np.float32), "amax": np.empty(n, np.float32),
               "amax_col": np.empty(n, np.uint32), "outside": np.empty(n, np.uint32),
               "delta": np.empty((n, self.in_len), np.float32) if delta else None, "nvalid": np.empty(n, np.uint32)}
        out = SimilarityMaskedOut()
        for name, ctype in SimilarityMaskedOut._fields_:
            if res[name] is not None:
                setattr(out, name, res[name].ctypes.data_as(ctype))
        check(lib().vsom_similarity_masked_batch(self._h, int(min_hits), int(num_sigmas), int(sigma_rule), r0, r1,
                                                 vb.ctypes.data_as(C.POINTER(C.c_uint8)), int(one), C.byref(out)))
        return res

    def evaluate_masked(self, valid, binary, continuous, min_hits=0, r0=0, r1=None):
        """evaluate for records with missing fields (vsom_evaluate_masked_batch; Standard / Median): chunk rows [r0, r1)
        searched over their valid columns only, as bmu_masked, and the binary error summed over those columns (an invalid
        column's term is +0 by select).  valid as in similarity_masked.  evaluate's dict, error the running mean of the
        masked dist + sqrt(bsum), and nvalid (uint32).  Read-only: lastBMU and sqres stay."""
        B = self.chunk_size
        r0 = int(r0)
        r1 = B if r1 is None else int(r1)
        if int(min_hits) < 0:
            raise ValueError("min_hits must be >= 0")
        if r0 < 0 or r0 > r1 or r1 > B:
            raise ValueError(f"row range [{r0}, {r1}) is not within the chunk's {B} rows")
        n = r1 - r0
        cols = []
        for name, a in (("binary", binary), ("continuous", continuous)):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != (self.in_len,):
                raise ValueError(f"{name} has shape {a.shape}, not ({self.in_len},)")
            cols.append(a)
        vb, one = self._mask_bytes(valid, n)
        res = {"bmu": np.empty(n, np.uint64), "dist": np.empty(n, np.float32), "bsum": np.empty(n, np.float32),
               "nrepl": np.empty(n, np.uint32), "error": np.zeros(1, np.float64), "nvalid": np.empty(n, np.uint32)}
        out = EvaluateMaskedOut()
        for name, ctype in EvaluateMaskedOut._fields_:
            setattr(out, name, res[name].ctypes.data_as(ctype))
        check(lib().vsom_evaluate_masked_batch(self._h, int(min_hits), r0, r1, _f(cols[0]), _f(cols[1]),
                                               vb.ctypes.data_as(C.POINTER(C.c_uint8)), int(one), C.byref(out)))
        res["error"] = float(res["error"][0])
        return res

    def restricted_bmd_masked(self, valid, min_hits, r0=0, r1=None, u=None, probs=False):
        """restricted_bmd for records with missing fields (vsom_bmd_masked_batch; Standard / Median): the distribution of
        chunk rows [r0, r1) over the units from the distance over their valid columns only, as bmu_masked's.  valid: rows x J
        (nonzero = valid), or a 1-D column mask of J entries applied to every row.  restricted_bmd's dict.  Read-only."""
        B = self.chunk_size
        r0 = int(r0)
        r1 = B if r1 is None else int(r1)
        if int(min_hits) < 0:
            raise ValueError("min_hits must be >= 0")
        if r0 < 0 or r0 > r1 or r1 > B:
            raise ValueError(f"row range [{r0}, {r1}) is not within the chunk's {B} rows")
        n = r1 - r0
        vb, one = self._mask_bytes(valid, n)
        dp = C.POINTER(C.c_double)
        norm = np.empty(n, np.float64)
        draw = prob = up = None
        if u is not None:
            u = self._uniforms(u, (n,))
            up = u.ctypes.data_as(dp)
            draw = np.empty(n, np.uint64)
        if probs:
            prob = np.empty((n, self.n_nodes), np.float64)
        check(lib().vsom_bmd_masked_batch(self._h, int(min_hits), r0, r1, vb.ctypes.data_as(C.POINTER(C.c_uint8)), int(one), up,
                                          _u(draw), norm.ctypes.data_as(dp), None if prob is None else prob.ctypes.data_as(dp)))
        return {"norm": norm, "draw": draw, "prob": prob}

    @staticmethod
    def _uniforms(u, shape):
        u = np.ascontiguousarray(u, dtype=np.float64)
        if u.shape != shape:
            raise ValueError(f"u has shape {u.shape}, not {shape}")
        if not ((u >= 0.0) & (u < 1.0)).all():
            raise ValueError("every uniform must lie in [0, 1)")
        return u

    def generate_masked(self, valid, min_hits, u, l, draws=1, keep_observed=True, r0=0, r1=None):
        """Sampled imputation of chunk rows [r0, r1) in one call (vsom_generate_masked_batch; Standard / Median): draws = K
        units per row, drawn with the uniforms u[r, k] from the row's distribution over its valid columns
        (restricted_bmd_masked's draw), and around each unit a record whose valid columns are the row's own values
        (keep_observed) and whose other columns are sampled as generate does, l: float64[rows, K, J].  valid as in
        restricted_bmd_masked.  A dict: unit (uint64[rows, K], NO_UNIT = no mass) and record (float64[rows, K, J], NaN
        throughout for a draw without mass).  u and l may also come as [rows] and [rows, J] when draws is 1.  Read-only."""
        B = self.chunk_size
        r0 = int(r0)
        r1 = B if r1 is None else int(r1)
        K = int(draws)
        if not 1 <= K <= 65535:
            raise ValueError(f"draws = {draws} is not in [1, 65535]")
        if int(min_hits) < 0:
            raise ValueError("min_hits must be >= 0")
        if r0 < 0 or r0 > r1 or r1 > B:
            raise ValueError(f"row range [{r0}, {r1}) is not within the chunk's {B} rows")
        n = r1 - r0
        J = self.in_len
        vb, one = self._mask_bytes(valid, n)
        u = np.asarray(u, dtype=np.float64)
        l = np.asarray(l, dtype=np.float64)
        if K == 1 and u.shape == (n,):
            u = u.reshape(n, 1)
        if K == 1 and l.shape == (n, J):
            l = l.reshape(n, 1, J)
        u = self._uniforms(u, (n, K))
        l = np.ascontiguousarray(l)
        if l.shape != (n, K, J):
            raise ValueError(f"l has shape {l.shape}, not ({n}, {K}, {J})")
        res = {"unit": np.empty((n, K), np.uint64), "record": np.empty((n, K, J), np.float64)}
        out = GenerateOut()
        for name, ctype in GenerateOut._fields_:
            setattr(out, name, res[name].ctypes.data_as(ctype))
        dp = C.POINTER(C.c_double)
        check(lib().vsom_generate_masked_batch(self._h, int(min_hits), r0, r1, vb.ctypes.data_as(C.POINTER(C.c_uint8)), int(one),
                                               K, int(bool(keep_observed)), u.ctypes.data_as(dp), l.ctypes.data_as(dp),
                                               C.byref(out)))
        return res

    def distances_row(self, row):
        out = np.empty(self.n_nodes, np.float32)
        check(lib().vsom_distances_row(self._h, int(row), _f(out)))
        return out

    def distances_raw(self, nodes, vrows, from_map):
        nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
        vrows = np.ascontiguousarray(vrows, dtype=np.uint64)
        out = np.empty(nodes.size, np.float32)
        check(lib().vsom_distances_raw(self._h, _u(nodes), _u(vrows), nodes.size, int(bool(from_map)), _f(out)))
        return out

    def _umatrix_shape_check(self):
        if self.width < 2 or self.height < 2:
            raise ValueError(f"the U-matrix needs width >= 2 and height >= 2, not {self.width} x {self.height}")

    def umatrix(self, fetch=True):
        """Som::updateUMatrix of the current map and sigmaMap in one launch (vsom_umatrix): float64[N], or None with
        fetch=False (only enqueued: get_umatrix() returns it later, as of the state at this call).  Read-only."""
        self._umatrix_shape_check()
        if not fetch:
            check(lib().vsom_umatrix(self._h, None))
            return None
        out = np.empty(self.n_nodes, np.float64)
        check(lib().vsom_umatrix(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def get_umatrix(self):
        """the matrix of the last umatrix() call (synchronises)"""
        self._umatrix_shape_check()
        out = np.empty(self.n_nodes, np.float64)
        check(lib().vsom_get_umatrix(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    # ---- batch epoch ---------------------------------------------------
    def batch_phase1_async(self, s0, s1, is_first):
        check(lib().vsom_batch_phase1_async(self._h, int(s0), int(s1), int(bool(is_first))))

    def batch_finish_async(self):
        check(lib().vsom_batch_finish_async(self._h))

    def batch_phase2_async(self, sigma, n0, n1):
        check(lib().vsom_batch_phase2_async(self._h, float(sigma), int(n0), int(n1)))

    def batch_epoch_async(self, sigma, is_first):
        check(lib().vsom_batch_epoch_async(self._h, float(sigma), int(bool(is_first))))

    def batch_epoch(self, sigma, is_first):
        mse = C.c_float()
        check(lib().vsom_batch_epoch(self._h, float(sigma), int(bool(is_first)), C.byref(mse)))
        return np.float32(mse.value)

    def get_mse(self):
        mse = C.c_float()
        check(lib().vsom_get_mse(self._h, C.byref(mse)))
        return np.float32(mse.value)

    def batch_schedule(self, sigmas, reset_bmu=True):
        """A whole batch schedule on the loaded chunk in one call (vsom_batch_schedule): epoch 0 with the exact search,
        the later ones with the local walk -- from unit 0 (reset_bmu, the reference's per-epoch reload) or from the
        previous epoch's BMU.  sigmas: one value per epoch.  Returns every epoch's MSE [float32 array]."""
        sg = _schedule(sigmas)
        mse = np.zeros(sg.size, np.float32)
        check(lib().vsom_batch_schedule(self._h, sg.ctypes.data_as(C.POINTER(C.c_double)), sg.size, int(bool(reset_bmu)),
                                        _f(mse)))
        return mse

    def _validity(self, valid):
        """valid as contiguous bytes and its one_mask flag; ValueError for a shape that is neither (J,) nor (B, J)"""
        B = self.chunk_size
        vb = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
        one = vb.ndim == 1
        if vb.shape != ((self.in_len,) if one else (B, self.in_len)):
            raise ValueError(f"valid has shape {vb.shape}, neither ({self.in_len},) nor ({B}, {self.in_len})")
        return vb, one

    def batch_schedule_masked(self, sigmas, valid, reset_bmu=True):
        """batch_schedule over the valid entries of the chunk only (vsom_batch_schedule_masked): bit for bit the loop of
        batch_epoch_masked calls with the same validity in every epoch; one launch for a tiny map (masked_tiny_applies).
        valid: B x J (nonzero = valid), or a 1-D column mask of J entries applied to every row; ValueError for another
        shape, before any call into the library.  Returns every epoch's MSE [float32 array]."""
        vb, one = self._validity(valid)
        sg = _schedule(sigmas)
        mse = np.zeros(sg.size, np.float32)
        check(lib().vsom_batch_schedule_masked(self._h, sg.ctypes.data_as(C.POINTER(C.c_double)), sg.size,
                                               int(bool(reset_bmu)), vb.ctypes.data_as(C.POINTER(C.c_uint8)), int(one),
                                               _f(mse)))
        return mse

    def masked_tiny_applies(self, one_mask=False):
        """would batch_schedule_masked on the loaded chunk take the one-workgroup masked kernel (finite sigmas given)?"""
        return bool(lib().vsom_masked_tiny_applies(self._h, int(bool(one_mask))))

    def batch_accum_begin(self, sigma, is_first, total_rows):
        """Open a batch epoch over a data set that loads in several chunks (vsom_batch_accum_begin): total_rows is the sum
        of the rows of the chunks that batch_accum_chunk will be called on.  ValueError for a negative or non-integral
        total_rows or a non-finite sigma, before any call into the library."""
        sigma = float(sigma)
        if not np.isfinite(sigma):
            raise ValueError(f"sigma must be finite, got {sigma}")
        if isinstance(total_rows, (bool, np.bool_)) or int(total_rows) != total_rows:
            raise ValueError(f"total_rows must be a whole number, got {total_rows!r}")
        if int(total_rows) < 0:
            raise ValueError(f"total_rows must be >= 0, got {total_rows}")
        check(lib().vsom_batch_accum_begin(self._h, sigma, int(bool(is_first)), int(total_rows)))

    def batch_accum_chunk(self):
        """the chunk currently loaded into the open epoch: search against the epoch-start map, then every node's chains
        continue over its rows (enqueues, does not block)"""
        check(lib().vsom_batch_accum_chunk(self._h))

    def batch_accum_chunk_masked(self, valid):
        """batch_accum_chunk over the valid entries of the chunk only (vsom_batch_accum_chunk_masked): the search on the
        masked distance, and per column the carried chain over the rows valid at that column.  valid: B x J (nonzero =
        valid), or a 1-D column mask of J entries applied to every row; ValueError for another shape, before any call
        into the library.  The array is not read after the call returns (enqueues, does not block)."""
        vb, one = self._validity(valid)
        check(lib().vsom_batch_accum_chunk_masked(self._h, vb.ctypes.data_as(C.POINTER(C.c_uint8)), int(one)))

    def batch_accum_end(self):
        """map, sigmaMap and weightMap of the whole epoch; returns its MSE (blocks)"""
        mse = C.c_float()
        check(lib().vsom_batch_accum_end(self._h, C.byref(mse)))
        return np.float32(mse.value)

    def batch_accum_abort(self):
        """close the open epoch: map, sigmaMap, weightMap and S stay what they were at batch_accum_begin"""
        check(lib().vsom_batch_accum_abort(self._h))

    def batch_epoch_masked(self, sigma, is_first, valid):
        """One batch epoch over the valid entries of the chunk only (vsom_batch_epoch_masked; Standard / Median, strict
        update mode): the search on the masked distance, and per column the chain over the rows valid at that column.
        valid: B x J (nonzero = valid), or a 1-D column mask of J entries applied to every row.  Returns the MSE."""
        vb, one = self._validity(valid)
        mse = C.c_float()
        check(lib().vsom_batch_epoch_masked(self._h, float(sigma), int(bool(is_first)),
                                            vb.ctypes.data_as(C.POINTER(C.c_uint8)), int(one), C.byref(mse)))
        return np.float32(mse.value)

    # ---- online --------------------------------------------------------
    def train_single(self, v, eta, sigma, last_bmu, decay_fn, valid=None):
        """Som::trainSingle of one host vector; valid= (custom contexts): the vector's validity for the hooks' value_weight"""
        v = np.ascontiguousarray(v, dtype=np.float32)
        assert v.size == self.in_len
        res = np.empty(self.residual_len, np.float32)
        lb, bmu, dist = C.c_uint64(int(last_bmu)), C.c_uint64(), C.c_float()
        if valid is not None:
            vb, vp = self._vector_valid(valid)
            check(lib().vsom_train_single_valid(self._h, _f(v), vp, float(eta), float(sigma), C.byref(lb),
                                                int(decay_fn), _f(res), C.byref(dist), C.byref(bmu)))
        else:
            check(lib().vsom_train_single(self._h, _f(v), float(eta), float(sigma), C.byref(lb),
                                          int(decay_fn), _f(res), C.byref(dist), C.byref(bmu)))
        return int(bmu.value), res, np.float32(dist.value), int(lb.value)

    def train_online_chunk(self, eta, sigma, decay_fn, first_chunk=True):
        """B sequential trainSingle steps on the staged chunk; returns the epoch's running MSE
        accumulator after it (first_chunk=False continues the previous chunk's value)."""
        mse = C.c_float()
        check(lib().vsom_train_online_chunk_acc(self._h, float(eta), float(sigma), int(decay_fn),
                                                int(bool(first_chunk)), C.byref(mse)))
        return np.float32(mse.value)

    def train_online_chunk_fetch(self, eta, sigma, decay_fn, first_chunk=True):
        """the same as one synchronising call that also hands back the chunk's lastBMU: (running MSE, lastBMU)"""
        mse = C.c_float()
        lb = np.zeros(self.chunk_size, np.uint64)
        check(lib().vsom_train_online_chunk_fetch(self._h, float(eta), float(sigma), int(decay_fn), int(bool(first_chunk)),
                                                  _u(lb), C.byref(mse)))
        return np.float32(mse.value), lb

    def train_online_chunk_masked(self, eta, sigma, decay_fn, valid, first_chunk=True):
        """train_online_chunk_fetch over the valid entries of the rows only (vsom_train_online_chunk_masked; Standard /
        Median): the search on the masked distance, and in every window node only the valid columns of map, SMap and
        sigmaMap are stepped.  valid: B x J (nonzero = valid), or a 1-D column mask of J entries applied to every row;
        ValueError for another shape, before any call into the library.  Returns (running MSE, lastBMU)."""
        B = self.chunk_size
        vb = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
        one = vb.ndim == 1
        if vb.shape != ((self.in_len,) if one else (B, self.in_len)):
            raise ValueError(f"valid has shape {vb.shape}, neither ({self.in_len},) nor ({B}, {self.in_len})")
        mse = C.c_float()
        lb = np.zeros(B, np.uint64)
        check(lib().vsom_train_online_chunk_masked(self._h, float(eta), float(sigma), int(decay_fn), int(bool(first_chunk)),
                                                   vb.ctypes.data_as(C.POINTER(C.c_uint8)), int(one), _u(lb), C.byref(mse)))
        return np.float32(mse.value), lb

    def online_masked_tiny_applies(self, sigma, one_mask=False):
        """would train_online_chunk_masked on the loaded chunk take the one-launch chunk of one workgroup
        (vsom_online_masked_tiny_applies)?"""
        return bool(lib().vsom_online_masked_tiny_applies(self._h, float(sigma), int(bool(one_mask))))

    def online_search_stats(self, reset=False):
        """image-bounded search of the online chunk loop: samples searched, nodes evaluated exactly, refinement workgroups
        with work (all zero while the exact scan is in use)"""
        out = np.zeros(4, np.uint64)
        check(lib().vsom_get_online_search_stats(self._h, _u(out), int(bool(reset))))
        return {"samples": int(out[0]), "exact_evaluations": int(out[1]), "refine_workgroups": int(out[2])}

    # ---- measurement ---------------------------------------------------
    def enable_timing(self, on=True, groups=None):
        """HIP-event timing of the kernel groups (TIMER_NAMES); groups = names to time only those (each timed group
        costs two event records between otherwise back-to-back kernels)"""
        if groups is None:
            check(lib().vsom_enable_timing(self._h, int(bool(on))))
        else:
            mask = 0
            for g in groups:
                mask |= 1 << TIMER_NAMES.index(g)
            check(lib().vsom_enable_timing_of(self._h, C.c_uint32(mask if on else 0)))

    def get_timing(self, reset=True):
        ms = (C.c_float * T_COUNT)()
        cnt = (C.c_uint32 * T_COUNT)()
        check(lib().vsom_get_timing(self._h, ms, cnt, int(bool(reset))))
        return {TIMER_NAMES[i]: (float(ms[i]), int(cnt[i])) for i in range(T_COUNT)}


class Group:
    """RAII wrapper of a vsom_group: Som::trainBatchSomEpoch over several GPUs from one process
    (include/vsom_hip.h, "multi-GPU batch epoch").  devices=None: devices 0..ndev-1; a list that repeats
    a device rehearses the N > 1 flow on one GPU (peer-copy transport)."""

    def __init__(self, width, height, in_len, transform=STANDARD, ndev=0, devices=None):
        self._h = C.c_void_p()
        self._members = []
        self.size = None
        devs = None
        if devices is not None:
            ndev = len(devices)
            devs = (C.c_int * ndev)(*[int(d) for d in devices])
        lib()
        assert_single_hip_runtime("vsom_group_create (RCCL)")
        check(lib().vsom_group_create(C.byref(self._h), int(ndev), devs, int(width), int(height), int(in_len),
                                      int(transform)))
        self.size = int(lib().vsom_group_size(self._h))
        self.transport = lib().vsom_group_transport(self._h).decode()
        self.width, self.height, self.in_len, self.transform = int(width), int(height), int(in_len), int(transform)
        c0 = self.member(0)
        self.depth, self.n_nodes = c0.depth, c0.n_nodes

    def member(self, rank):
        """Borrowed Context of one member for the single-context calls (searches, getters).  The group is
        synchronised first (include/vsom_hip.h requires it), the returned object keeps the group alive, and
        Group.close() invalidates it -- a call on it afterwards raises instead of touching freed memory."""
        if not self._h:
            raise VsomError("group is closed")
        h = lib().vsom_group_ctx(self._h, int(rank))
        if not h:
            raise VsomError("rank out of range")
        if getattr(self, "size", None) is not None:     # (not yet during __init__)
            check(lib().vsom_group_synchronize(self._h))
        c = Context(self.width, self.height, self.in_len, self.transform, _borrowed=h)
        c._group = self
        self._members.append(c)
        return c

    def close(self):
        if self._h:
            for c in self._members:
                c._h = C.c_void_p()                       # borrowed handles die with the group
            self._members = []
            lib().vsom_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(lib().vsom_group_synchronize(self._h))

    def set_update_mode(self, mode):
        check(lib().vsom_group_set_update_mode(self._h, int(mode)))

    def set_bmu_mode(self, mode):
        check(lib().vsom_group_set_bmu_mode(self._h, int(mode)))

    def set_state(self, map=None, sigma=None, S=None, weight=None, hits=None):
        n, d = self.n_nodes, self.depth

        def f2(a, size):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32)
            assert a.size == size, (a.shape, size)
            return a

        m, s, ss, w = f2(map, n * d), f2(sigma, n * d), f2(S, n * d), f2(weight, n)
        h = None if hits is None else np.ascontiguousarray(hits, dtype=np.uint64)
        check(lib().vsom_group_set_state(self._h, _f(m), _f(s), _f(ss), _f(w), _u(h)))

    def get_state(self):
        n, d = self.n_nodes, self.depth
        m, s, ss = (np.empty((n, d), np.float32) for _ in range(3))
        w, h = np.empty(n, np.float32), np.empty(n, np.uint64)
        check(lib().vsom_group_get_state(self._h, _f(m), _f(s), _f(ss), _f(w), _u(h)))
        return {"map": m, "sigma": s, "S": ss, "weight": w, "hits": h}

    def upload_chunk(self, X):
        X = np.ascontiguousarray(X, dtype=np.float32)
        assert X.ndim == 2 and X.shape[1] == self.in_len, (X.shape, self.in_len)
        self._B = X.shape[0]
        check(lib().vsom_group_upload_chunk(self._h, _f(X), X.shape[0]))

    def prefetch_chunk(self, X):
        """X must stay alive (and unchanged) until commit_chunk/prefetch_wait; pinned memory makes it asynchronous"""
        assert X.dtype == np.float32 and X.flags["C_CONTIGUOUS"] and X.shape[1] == self.in_len
        self._B = X.shape[0]
        check(lib().vsom_group_prefetch_chunk(self._h, _f(X), X.shape[0]))

    def prefetch_wait(self):
        check(lib().vsom_group_prefetch_wait(self._h))

    def commit_chunk(self):
        check(lib().vsom_group_commit_chunk(self._h))

    def set_chunk_device(self, rows_dev, B):
        """rows_dev[r] = device pointer (int) of member r's own rows [B*r/n, B*(r+1)/n) on its device"""
        assert len(rows_dev) == self.size
        arr = (C.c_void_p * self.size)(*[C.c_void_p(int(p) or None) for p in rows_dev])
        self._B = int(B)
        check(lib().vsom_group_set_chunk_device(self._h, arr, int(B)))

    def set_last_bmu(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        check(lib().vsom_group_set_last_bmu(self._h, _u(idx)))

    def get_last_bmu(self):
        out = np.empty(self._B, np.uint64)
        check(lib().vsom_group_get_last_bmu(self._h, _u(out)))
        return out

    def batch_epoch_async(self, sigma, is_first):
        check(lib().vsom_group_batch_epoch_async(self._h, float(sigma), int(bool(is_first))))

    def batch_epoch(self, sigma, is_first):
        mse = C.c_float()
        check(lib().vsom_group_batch_epoch(self._h, float(sigma), int(bool(is_first)), C.byref(mse)))
        return np.float32(mse.value)

    def get_mse(self):
        mse = C.c_float()
        check(lib().vsom_group_get_mse(self._h, C.byref(mse)))
        return np.float32(mse.value)


def _schedule(sigmas):
    """a schedule's sigma values as a contiguous 1-D float64 array (ValueError for any other shape)"""
    sg = np.asarray(sigmas, dtype=np.float64)
    if sg.ndim != 1:
        raise ValueError(f"a schedule is a 1-D sequence of sigma values, got shape {sg.shape}")
    return np.ascontiguousarray(sg)


def _is_nested(sigmas):
    """one schedule per member (a sequence of sequences) rather than one schedule of scalars"""
    if isinstance(sigmas, np.ndarray):
        return sigmas.ndim == 2 or sigmas.dtype == object
    return hasattr(sigmas, "__len__") and len(sigmas) > 0 and all(hasattr(v, "__len__") for v in sigmas)


class Ensemble:
    """A set of Contexts on one device trained by one call (include/vsom_hip.h, vsom_ensemble): the same results, bit for
    bit, as the single-context call on every member in turn.  Members stay ordinary Contexts (upload, state, checkpoints);
    close the ensemble before closing a member.  Parameters are scalars (every member) or one value per member."""

    def __init__(self, contexts):
        self.members = list(contexts)
        n = len(self.members)
        arr = (C.c_void_p * max(n, 1))(*[c._h.value if c is not None and c._h else None for c in self.members])
        self._h = C.c_void_p()
        check(lib().vsom_ensemble_create(C.byref(self._h), arr, n))
        self._pinned = None         # upload_chunks' packing buffer (grow-only)

    def __len__(self):
        return len(self.members)

    def close(self):
        if self._h:
            lib().vsom_ensemble_destroy(self._h)
            self._h = C.c_void_p()
        if getattr(self, "_pinned", None) is not None:
            self._pinned.free()
            self._pinned = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _per_member(self, v, ctype, conv):
        n = len(self.members)
        vals = [conv(x) for x in v] if np.ndim(v) else [conv(v)] * n
        if len(vals) != n:
            raise ValueError(f"{len(vals)} values for {n} members")
        return (ctype * n)(*vals)

    def train_online_chunk_fetch(self, eta, sigma, decay_fn, first_chunk=True):
        """one online chunk on every member: (running MSE per member [float32 array], lastBMU per member [list of
        uint64 arrays, each of that member's chunk size])"""
        n = len(self.members)
        lbs = [np.zeros(c.chunk_size, np.uint64) for c in self.members]
        ptrs = (C.POINTER(C.c_uint64) * n)(*[_u(a) for a in lbs])
        mse = np.zeros(n, np.float32)
        check(lib().vsom_ensemble_train_online_chunk_fetch(
            self._h, self._per_member(eta, C.c_double, float), self._per_member(sigma, C.c_double, float),
            self._per_member(decay_fn, C.c_int, int), int(bool(first_chunk)), ptrs, _f(mse)))
        return mse, lbs

    def train_online_chunk_masked(self, eta, sigma, decay_fn, valid, first_chunk=True):
        """train_online_chunk_fetch over the valid entries only for the members with a validity
        (vsom_ensemble_train_online_chunk_masked).  valid: as in batch_epoch_masked -- a list with one entry per member,
        None (a plain member), a B x J array, or a 1-D column mask of J entries; ValueError before any call into the
        library.  Returns (running MSE per member [float32 array], lastBMU per member [list of uint64 arrays])."""
        keep, vptrs, ones = self._validities(valid)
        n = len(self.members)
        lbs = [np.zeros(c.chunk_size, np.uint64) for c in self.members]
        ptrs = (C.POINTER(C.c_uint64) * n)(*[_u(a) for a in lbs])
        mse = np.zeros(n, np.float32)
        check(lib().vsom_ensemble_train_online_chunk_masked(
            self._h, self._per_member(eta, C.c_double, float), self._per_member(sigma, C.c_double, float),
            self._per_member(decay_fn, C.c_int, int), int(bool(first_chunk)), vptrs, ones, ptrs, _f(mse)))
        del keep
        return mse, lbs

    def batch_epoch(self, sigma, is_first):
        """one batch epoch on every member: the MSE per member [float32 array]"""
        mse = np.zeros(len(self.members), np.float32)
        check(lib().vsom_ensemble_batch_epoch(self._h, self._per_member(sigma, C.c_double, float), int(bool(is_first)),
                                              _f(mse)))
        return mse

    def batch_schedule(self, sigmas, reset_bmu=True):
        """a whole batch schedule on every member in one call (vsom_ensemble_batch_schedule).  sigmas: one sequence of
        values that every member runs, or one sequence per member (their lengths may differ, 0 included).  Returns each
        member's per-epoch MSE [list of float32 arrays]."""
        n = len(self.members)
        if _is_nested(sigmas):
            per = [_schedule(v) for v in sigmas]
            if len(per) != n:
                raise ValueError(f"{len(per)} schedules for {n} members")
        else:
            per = [_schedule(sigmas)] * n
        mses = [np.zeros(sg.size, np.float32) for sg in per]
        dp = C.POINTER(C.c_double)
        sig = (dp * max(n, 1))(*[sg.ctypes.data_as(dp) for sg in per])
        out = (C.POINTER(C.c_float) * max(n, 1))(*[_f(m) for m in mses])
        cnt = (C.c_size_t * max(n, 1))(*[sg.size for sg in per])
        check(lib().vsom_ensemble_batch_schedule(self._h, sig, cnt, int(bool(reset_bmu)), out))
        return mses

    def _validities(self, valid, none="a plain member"):
        """valid (one entry per member: None for a plain member -- in the masked queries a skipped one, `none` words the
        message -- else that member's B x J or 1-D J validity) as the arrays, the pointer array and the one_mask array of
        the masked calls; ValueError before any call into the library"""
        n = len(self.members)
        if isinstance(valid, np.ndarray) or not hasattr(valid, "__len__") or len(valid) != n:
            raise ValueError(f"valid must be a list of one entry per member ({n}), None for {none}")
        keep = [None if v is None else c._validity(v) for c, v in zip(self.members, valid)]
        u8p = C.POINTER(C.c_uint8)
        ptrs = (u8p * max(n, 1))(*[u8p() if kv is None else kv[0].ctypes.data_as(u8p) for kv in keep])
        ones = (C.c_int * max(n, 1))(*[0 if kv is None else int(kv[1]) for kv in keep])
        return keep, ptrs, ones

    def batch_epoch_masked(self, sigma, is_first, valid):
        """one batch epoch on every member, over the valid entries only for the members with a validity
        (vsom_ensemble_batch_epoch_masked).  valid: a list with one entry per member -- None (a plain member: batch_epoch),
        a B x J array, or a 1-D column mask of J entries.  Returns the MSE per member [float32 array]."""
        keep, ptrs, ones = self._validities(valid)
        mse = np.zeros(len(self.members), np.float32)
        check(lib().vsom_ensemble_batch_epoch_masked(self._h, self._per_member(sigma, C.c_double, float),
                                                     int(bool(is_first)), ptrs, ones, _f(mse)))
        del keep
        return mse

    def batch_schedule_masked(self, sigmas, valid, reset_bmu=True):
        """batch_schedule with each member's validity (vsom_ensemble_batch_schedule_masked); sigmas as in batch_schedule,
        valid as in batch_epoch_masked.  Returns each member's per-epoch MSE [list of float32 arrays]."""
        n = len(self.members)
        keep, ptrs, ones = self._validities(valid)
        if _is_nested(sigmas):
            per = [_schedule(v) for v in sigmas]
            if len(per) != n:
                raise ValueError(f"{len(per)} schedules for {n} members")
        else:
            per = [_schedule(sigmas)] * n
        mses = [np.zeros(sg.size, np.float32) for sg in per]
        dp = C.POINTER(C.c_double)
        sig = (dp * max(n, 1))(*[sg.ctypes.data_as(dp) for sg in per])
        out = (C.POINTER(C.c_float) * max(n, 1))(*[_f(m) for m in mses])
        cnt = (C.c_size_t * max(n, 1))(*[sg.size for sg in per])
        check(lib().vsom_ensemble_batch_schedule_masked(self._h, sig, cnt, int(bool(reset_bmu)), ptrs, ones, out))
        del keep
        return mses

    def upload_chunks(self, rows):
        """every member's chunk in one call (vsom_ensemble_upload_chunks, wait = 1): `rows` is a list of one 2-D float32
        array per member, or one 2-D array that every member gets.  The same array object given to several members is
        packed once and shared.  Bit for bit what Context.upload_chunk on every member gives."""
        n = len(self.members)
        if isinstance(rows, np.ndarray):
            rows = [rows] * n
        rows = list(rows)
        if len(rows) != n:
            raise ValueError(f"{len(rows)} chunks for {n} members")
        seen, parts, offsets, Bs, total = {}, [], [], [], 0
        for k, (X, c) in enumerate(zip(rows, self.members)):
            X = np.asarray(X)
            if X.ndim != 2 or X.shape[1] != c.in_len:
                raise ValueError(f"member {k}: rows of shape {X.shape}, the member reads rows of {c.in_len}")
            key = id(rows[k])
            if key not in seen:
                seen[key] = total
                parts.append((total, X))
                total += X.size
            offsets.append(seen[key])
            Bs.append(X.shape[0])
        if self._pinned is None or self._pinned.array.size < total:
            if self._pinned is not None:
                self._pinned.free()
            self._pinned = PinnedBuffer((max(total, 1),))
        buf = self._pinned.array
        for at, X in parts:
            buf[at:at + X.size] = X.reshape(-1)
        self._upload(buf, total, offsets, Bs, 1)

    def upload_chunks_async(self, pinned, offsets, B):
        """the low-level form (wait = 0): member k gets B[k] rows at pinned.flat[offsets[k]:] (a PinnedBuffer's float32
        array, which must stay unchanged until a call that synchronises the members has returned)"""
        a = pinned.array if isinstance(pinned, PinnedBuffer) else pinned
        assert a.dtype == np.float32 and a.flags.c_contiguous
        self._upload(a, a.size, offsets, B, 0)

    def _upload(self, a, n_floats, offsets, B, wait):
        n = len(self.members)
        if len(offsets) != n or len(B) != n:
            raise ValueError(f"{len(offsets)} offsets and {len(B)} chunk sizes for {n} members")
        off = (C.c_size_t * n)(*[int(v) for v in offsets])
        bs = (C.c_size_t * n)(*[int(v) for v in B])
        check(lib().vsom_ensemble_upload_chunks(self._h, _f(a), int(n_floats), off, bs, int(wait)))

    def bmu_batch(self):
        """Som::findBmu for every row of every member's chunk (vsom_ensemble_bmu_batch): (list of uint64 index arrays,
        list of float32 distance arrays), one array per member"""
        n = len(self.members)
        idx = [np.empty(c.chunk_size, np.uint64) for c in self.members]
        dist = [np.empty(c.chunk_size, np.float32) for c in self.members]
        ip = (C.POINTER(C.c_uint64) * n)(*[_u(a) for a in idx])
        dp = (C.POINTER(C.c_float) * n)(*[_f(a) for a in dist])
        check(lib().vsom_ensemble_bmu_batch(self._h, ip, dp))
        return idx, dist

    def _min_hits(self, min_hits):
        """min_hits (a scalar or one value per member) as the uint64 array of the masked queries; ValueError for a
        negative value or a wrong count"""
        n = len(self.members)
        vals = [int(v) for v in min_hits] if np.ndim(min_hits) else [int(min_hits)] * n
        if len(vals) != n:
            raise ValueError(f"{len(vals)} values of min_hits for {n} members")
        if any(v < 0 for v in vals):
            raise ValueError("min_hits must be >= 0")
        return (C.c_uint64 * max(n, 1))(*vals)

    def bmu_masked(self, valid, min_hits=0, fill=False):
        """Context.bmu_masked of every member's whole chunk in one call (vsom_ensemble_bmu_masked_batch).  valid: a list with
        one entry per member -- None (the member is skipped), a B x J array (nonzero = valid), or a 1-D column mask of J
        entries; min_hits: a scalar or one value per member.  A list with one entry per member: the dict Context.bmu_masked
        returns (bmu, dist, nvalid, and fill unless fill=False), or None for a skipped member.  ValueError before any call
        into the library.  Read-only."""
        keep, vptrs, ones = self._validities(valid, none="a skipped member")
        mh = self._min_hits(min_hits)
        n = len(self.members)
        res, outs = [], (MaskedOut * max(n, 1))()
        for k, (c, kv) in enumerate(zip(self.members, keep)):
            if kv is None:
                res.append(None)
                continue
            B, J = c.chunk_size, c.in_len
            r = {"bmu": np.empty(B, np.uint64), "dist": np.empty(B, np.float32), "nvalid": np.empty(B, np.uint32),
                 "fill": np.empty((B, J), np.float32) if fill else None}
            for name, ctype in MaskedOut._fields_:
                if r[name] is not None:
                    setattr(outs[k], name, r[name].ctypes.data_as(ctype))
            res.append(r)
        check(lib().vsom_ensemble_bmu_masked_batch(self._h, mh, vptrs, ones, outs))
        del keep
        return res

    def impute(self, valid, min_hits=0):
        """every member's rows with the missing fields taken from the row's masked BMU (bmu_masked's fill): a list of
        float32[B, J] arrays, None for a skipped member"""
        return [None if r is None else r["fill"] for r in self.bmu_masked(valid, min_hits=min_hits, fill=True)]

    def similarity_masked(self, valid, min_hits, num_sigmas, sigma_rule=SIGMA_FLOOR, delta=False):
        """Context.similarity_masked of every member's whole chunk in one call (vsom_ensemble_similarity_masked_batch).
        valid and min_hits as in bmu_masked; num_sigmas: a scalar or one value per member; sigma_rule applies to every
        member.  A list with one entry per member: the dict Context.similarity_masked returns, or None for a skipped
        member.  ValueError before any call into the library.  Read-only."""
        if int(sigma_rule) not in (SIGMA_AS_WRITTEN, SIGMA_FLOOR):
            raise ValueError(f"sigma_rule = {sigma_rule} is neither SIGMA_AS_WRITTEN nor SIGMA_FLOOR")
        keep, vptrs, ones = self._validities(valid, none="a skipped member")
        mh = self._min_hits(min_hits)
        n = len(self.members)
        ns = [int(v) for v in num_sigmas] if np.ndim(num_sigmas) else [int(num_sigmas)] * n
        if len(ns) != n:
            raise ValueError(f"{len(ns)} values of num_sigmas for {n} members")
        if any(not -2 ** 31 <= v < 2 ** 31 for v in ns):
            raise ValueError("num_sigmas must fit an int")
        res, outs = [], (SimilarityMaskedOut * max(n, 1))()
        for k, (c, kv) in enumerate(zip(self.members, keep)):
            if kv is None:
                res.append(None)
                continue
            B, J = c.chunk_size, c.in_len
            r = {"bmu": np.empty(B, np.uint64), "dist": np.empty(B, np.float32), "dmax": np.empty(B, np.float32),
                 "dmax_col": np.empty(B, np.uint32), "first": np.empty(B, np.float32), "amax": np.empty(B, np.float32),
                 "amax_col": np.empty(B, np.uint32), "outside": np.empty(B, np.uint32),
                 "delta": np.empty((B, J), np.float32) if delta else None, "nvalid": np.empty(B, np.uint32)}
            for name, ctype in SimilarityMaskedOut._fields_:
                if r[name] is not None:
                    setattr(outs[k], name, r[name].ctypes.data_as(ctype))
            res.append(r)
        check(lib().vsom_ensemble_similarity_masked_batch(self._h, mh, (C.c_int * max(n, 1))(*ns), int(sigma_rule), vptrs,
                                                          ones, outs))
        del keep
        return res

    def _ks(self, k):
        """k (an int or one value per member) as the uint32 array of the top-k calls and as a list; ValueError for a
        wrong count or a value outside [1, 64]"""
        n = len(self.members)
        vals = [int(v) for v in k] if np.ndim(k) else [int(k)] * n
        if len(vals) != n:
            raise ValueError(f"{len(vals)} values of k for {n} members")
        if any(not 1 <= v <= 64 for v in vals):
            raise ValueError("k must be in [1, 64]")
        return (C.c_uint32 * max(n, 1))(*vals), vals

    def _topk_outputs(self, ks, covered, dist, masked):
        """the result dicts (None for a member that is not covered) and the vsom_ensemble_topk_out array over them"""
        n = len(self.members)
        res, outs = [], (EnsembleTopkOut * max(n, 1))()
        for m, c in enumerate(self.members):
            if not covered[m]:
                res.append(None)
                continue
            B = c.chunk_size
            r = {"idx": np.empty((B, ks[m]), np.uint64), "dist": np.empty((B, ks[m]), np.float32) if dist else None}
            if masked:
                r.update(count=np.empty(B, np.uint32), nvalid=np.empty(B, np.uint32))
            for name, ctype in EnsembleTopkOut._fields_:
                if r.get(name) is not None:
                    setattr(outs[m], name, r[name].ctypes.data_as(ctype))
            res.append(r)
        return res, outs

    def bmu_topk(self, k, dist=True, members=None):
        """Context.bmu_topk of every member's whole chunk in one call (vsom_ensemble_bmu_topk_batch).  k: an int or one
        value per member; members: None (every member) or the indices of the members to cover, the others are skipped.
        A list with one entry per member: {"idx": uint64[B, k], "dist": float32[B, k] or None}, or None for a skipped
        member.  ValueError before any call into the library.  Read-only."""
        n = len(self.members)
        kp, ks = self._ks(k)
        covered = [True] * n
        if members is not None:
            chosen = [int(m) for m in members]
            if any(not 0 <= m < n for m in chosen):
                raise ValueError(f"members must be indices in [0, {n})")
            covered = [m in chosen for m in range(n)]
        res, outs = self._topk_outputs(ks, covered, dist, False)
        check(lib().vsom_ensemble_bmu_topk_batch(self._h, kp, outs))
        return res

    def bmu_topk_masked(self, k, valid, min_hits=0, dist=True):
        """Context.bmu_topk_masked (without blend) of every member's whole chunk in one call
        (vsom_ensemble_bmu_topk_masked_batch).  k: an int or one value per member; valid and min_hits as in bmu_masked.
        A list with one entry per member: {"idx": uint64[B, k], "dist": float32[B, k] or None, "count": uint32[B],
        "nvalid": uint32[B]}, or None for a skipped member.  ValueError before any call into the library.  Read-only."""
        kp, ks = self._ks(k)
        keep, vptrs, ones = self._validities(valid, none="a skipped member")
        mh = self._min_hits(min_hits)
        res, outs = self._topk_outputs(ks, [kv is not None for kv in keep], dist, True)
        check(lib().vsom_ensemble_bmu_topk_masked_batch(self._h, kp, mh, vptrs, ones, outs))
        del keep
        return res

    def topk_applies(self, member, k, masked=False):
        """would that member with that k run in the one-launch kernel of bmu_topk / bmu_topk_masked
        (vsom_ensemble_topk_applies)?"""
        rc = lib().vsom_ensemble_topk_applies(self._h, int(member), int(k), int(bool(masked)))
        if rc < 0:
            check(rc)
        return bool(rc)

    def _columns(self, name, a, covered):
        """the column factors `name` (one array of J entries for all members, when every covered J agrees, or a list with
        one array per member; an entry of a member that is not covered may be None) as the float32 arrays (None: not
        covered) and the pointer array of the evaluate calls; ValueError before any call into the library"""
        n = len(self.members)
        if isinstance(a, (list, tuple)) and (len(a) == 0 or a[0] is None or np.ndim(a[0]) > 0):
            if len(a) != n:
                raise ValueError(f"{name}: {len(a)} arrays for {n} members")
            per = list(a)
        else:
            per = [a] * n
        fp = C.POINTER(C.c_float)
        keep = []
        for m, c in enumerate(self.members):
            if not covered[m]:
                keep.append(None)
                continue
            if per[m] is None:
                raise ValueError(f"{name}: member {m} is covered and has no array")
            v = np.ascontiguousarray(per[m], dtype=np.float32)
            if v.shape != (c.in_len,):
                raise ValueError(f"{name}: member {m}: shape {v.shape}, not ({c.in_len},)")
            keep.append(v)
        return keep, (fp * max(n, 1))(*[fp() if v is None else _f(v) for v in keep])

    def _evaluate_outputs(self, covered, struct):
        """the result dicts (None for a member that is not covered) and the array of `struct` over them"""
        n = len(self.members)
        res, outs = [], (struct * max(n, 1))()
        for m, c in enumerate(self.members):
            if not covered[m]:
                res.append(None)
                continue
            B = c.chunk_size
            r = {"bmu": np.empty(B, np.uint64), "dist": np.empty(B, np.float32), "bsum": np.empty(B, np.float32),
                 "nrepl": np.empty(B, np.uint32), "error": np.zeros(1, np.float64)}
            if struct is EvaluateMaskedOut:
                r["nvalid"] = np.empty(B, np.uint32)
            for name, ctype in struct._fields_:
                setattr(outs[m], name, r[name].ctypes.data_as(ctype))
            res.append(r)
        return res, outs

    def evaluate(self, binary, continuous, valid=None, members=None):
        """Context.evaluate of every member's whole chunk in one call (vsom_ensemble_evaluate_batch): the validation loss a
        sweep is ranked by.  binary, continuous: one array of J column factors for all members (every covered J must
        agree) or a list with one array per member; valid: None, or a list with one entry per member -- None or that
        member's B x J validity (nonzero = valid); members: None (every member) or the indices of the members to cover,
        the others are skipped.  A list with one entry per member: the dict Context.evaluate returns (bmu, dist, bsum,
        nrepl, error), or None for a skipped member.  ValueError before any call into the library.  Overwrites the
        covered members' lastBMU / sqres like bmu_batch."""
        n = len(self.members)
        covered = [True] * n
        if members is not None:
            chosen = [int(m) for m in members]
            if any(not 0 <= m < n for m in chosen):
                raise ValueError(f"members must be indices in [0, {n})")
            covered = [m in chosen for m in range(n)]
        bkeep, bptrs = self._columns("binary", binary, covered)
        ckeep, cptrs = self._columns("continuous", continuous, covered)
        vkeep, vptrs = None, None
        if valid is not None:
            if isinstance(valid, np.ndarray) or not hasattr(valid, "__len__") or len(valid) != n:
                raise ValueError(f"valid must be None or a list of one entry per member ({n}), None for a member without one")
            u8p = C.POINTER(C.c_uint8)
            vkeep = []
            for m, (c, v) in enumerate(zip(self.members, valid)):
                if v is None or not covered[m]:
                    vkeep.append(None)
                    continue
                vb = np.ascontiguousarray(np.asarray(v) != 0, dtype=np.uint8)
                if vb.shape != (c.chunk_size, c.in_len):
                    raise ValueError(f"valid: member {m}: shape {vb.shape}, not ({c.chunk_size}, {c.in_len})")
                vkeep.append(vb)
            vptrs = (u8p * max(n, 1))(*[u8p() if v is None else v.ctypes.data_as(u8p) for v in vkeep])
        res, outs = self._evaluate_outputs(covered, EvaluateOut)
        check(lib().vsom_ensemble_evaluate_batch(self._h, bptrs, cptrs, vptrs, outs))
        del bkeep, ckeep, vkeep
        for r in res:
            if r is not None:
                r["error"] = float(r["error"][0])
        return res

    def evaluate_masked(self, valid, binary, continuous, min_hits=0):
        """Context.evaluate_masked of every member's whole chunk in one call (vsom_ensemble_evaluate_masked_batch).  valid
        and min_hits as in bmu_masked (a None entry skips the member); binary, continuous as in evaluate.  A list with one
        entry per member: evaluate's dict with nvalid added, or None for a skipped member.  ValueError before any call
        into the library.  Read-only."""
        keep, vptrs, ones = self._validities(valid, none="a skipped member")
        mh = self._min_hits(min_hits)
        covered = [kv is not None for kv in keep]
        bkeep, bptrs = self._columns("binary", binary, covered)
        ckeep, cptrs = self._columns("continuous", continuous, covered)
        res, outs = self._evaluate_outputs(covered, EvaluateMaskedOut)
        check(lib().vsom_ensemble_evaluate_masked_batch(self._h, mh, bptrs, cptrs, vptrs, ones, outs))
        del keep, bkeep, ckeep
        for r in res:
            if r is not None:
                r["error"] = float(r["error"][0])
        return res

    def evaluate_applies(self, member, masked=False):
        """would that member run in the one-launch kernel of evaluate / evaluate_masked (vsom_ensemble_evaluate_applies)?"""
        rc = lib().vsom_ensemble_evaluate_applies(self._h, int(member), int(bool(masked)))
        if rc < 0:
            check(rc)
        return bool(rc)

    def validation_errors(self, binary, continuous, valid=None, members=None, masked=False, min_hits=0):
        """the validation loss of every member on its chunk as one float64 array, NaN for a skipped member: what a sweep
        sorts by.  masked=False: evaluate(binary, continuous, valid, members); masked=True: evaluate_masked(valid, binary,
        continuous, min_hits), whose None entries of valid are the skipped members."""
        if masked:
            if members is not None:
                raise ValueError("masked=True: the members are chosen by the None entries of valid")
            got = self.evaluate_masked(valid, binary, continuous, min_hits=min_hits)
        else:
            got = self.evaluate(binary, continuous, valid=valid, members=members)
        return np.array([np.nan if r is None else r["error"] for r in got], np.float64)

    def _rankable(self):
        """the members a topographic error exists for: at least 2 nodes and a chunk with rows"""
        return [c.n_nodes >= 2 and c.chunk_size > 0 for c in self.members]

    def topographic_error(self):
        """the topographic error of every member on its chunk, from one bmu_topk call with k = 2: a float64 array, member
        m's value som.topographic_error(idx2, width) on its lists; NaN for a member with fewer than 2 nodes or no rows"""
        from .som import topographic_error
        ok = self._rankable()
        te = np.full(len(self.members), np.nan, np.float64)
        if any(ok):
            got = self.bmu_topk(2, dist=False, members=[m for m, v in enumerate(ok) if v])
            for m, c in enumerate(self.members):
                if ok[m]:
                    te[m] = topographic_error(got[m]["idx"], c.width)
        return te

    def topographic_error_masked(self, valid, min_hits=0):
        """the topographic error of every member over the valid columns, from one bmu_topk_masked call with k = 2:
        (errors float64[K], rows_counted int64[K]).  A member's rows count when they have a valid column and a second unit
        (nvalid >= 1 and count >= 2, the rule of Som.topographicErrorMasked); its error is som.topographic_error over
        them.  NaN and 0 for a member with fewer than 2 nodes, no rows or no validity (None)."""
        from .som import topographic_error
        n = len(self.members)
        if isinstance(valid, np.ndarray) or not hasattr(valid, "__len__") or len(valid) != n:
            raise ValueError(f"valid must be a list of one entry per member ({n}), None for a skipped member")
        ok = self._rankable()
        te = np.full(n, np.nan, np.float64)
        counted = np.zeros(n, np.int64)
        use = [v if ok[m] else None for m, v in enumerate(valid)]
        if any(v is not None for v in use):
            got = self.bmu_topk_masked(2, use, min_hits=min_hits, dist=False)
            for m, c in enumerate(self.members):
                if got[m] is not None:
                    keep = (got[m]["nvalid"] >= 1) & (got[m]["count"] >= 2)
                    te[m] = topographic_error(got[m]["idx"][keep], c.width)
                    counted[m] = int(keep.sum())
        return te, counted

    def umatrix(self):
        """Som::updateUMatrix of every member (vsom_ensemble_umatrix): a list of float64 arrays, one per member, each
        what Context.umatrix() of that member gives"""
        n = len(self.members)
        for k, c in enumerate(self.members):
            if c.width < 2 or c.height < 2:
                raise ValueError(f"member {k}: the U-matrix needs width >= 2 and height >= 2, not {c.width} x {c.height}")
        out = [np.empty(c.n_nodes, np.float64) for c in self.members]
        dp = C.POINTER(C.c_double)
        ptrs = (dp * max(n, 1))(*[a.ctypes.data_as(dp) for a in out])
        check(lib().vsom_ensemble_umatrix(self._h, ptrs))
        return out
