"""ctypes loader of csrc/libvlq_ivfpq.so (the C ABI of include/vlq_ivfpq.h)."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_SO = os.environ.get("VLQ_LIB_PATH") or os.path.join(_CSRC, "libvlq_ivfpq.so")   # override: A/B builds of the library

# every symbol include/vlq_ivfpq.h declares
SYMBOLS = [
    "vlq_version", "vlq_last_error", "vlq_device_count", "vlq_ivfpq_create", "vlq_ivfpq_destroy",
    "vlq_ivfpq_set_stream", "vlq_ivfpq_set_coarse_centroids", "vlq_ivfpq_set_imi_centroids",
    "vlq_ivfpq_set_pq_centroids",
    "vlq_ivfpq_set_search_options", "vlq_ivfpq_set_float16_tables", "vlq_ivfpq_set_scan_schedule", "vlq_ivfpq_set_coarse_screen", "vlq_ivfpq_coarse_screen_state", "vlq_ivfpq_set_scan_sums", "vlq_ivfpq_scan_sums_state", "vlq_ivfpq_set_lists", "vlq_ivfpq_add", "vlq_ivfpq_reserve_memory", "vlq_ivfpq_reclaim_memory", "vlq_ivfpq_encode", "vlq_ivfpq_encode_preassigned",
    "vlq_ivfpq_ntotal", "vlq_ivfpq_list_length", "vlq_ivfpq_get_list", "vlq_ivfpq_search",
    "vlq_ivfpq_search_preassigned", "vlq_ivfpq_coarse_search", "vlq_ivfpq_query_tables",
    "vlq_ivfpq_get_precomputed_table", "vlq_ivfpq_stats", "vlq_ivfpq_profile",
    "vlq_ivfpq_profile_read", "vlq_merge_topk", "vlq_ivfpq_last_scan_info", "vlq_ivfpq_reset_walk_state",
    "vlq_ivfpq_set_refine_pq", "vlq_ivfpq_set_refine_codes", "vlq_ivfpq_get_list_refine_codes", "vlq_ivfpq_refine",
    "vlq_ivfpq_search_refined", "vlq_ivfpq_search_refined_preassigned",
    "vlq_ivfpq_set_polysemous_ht", "vlq_ivfpq_query_codes", "vlq_ivfpq_polysemous_stats",
    "vlq_ivfpq_set_metric", "vlq_ivfpq_get_metric",
    # IVFFlat (vlq_ivfflat_t)
    "vlq_ivfflat_create", "vlq_ivfflat_destroy", "vlq_ivfflat_set_stream", "vlq_ivfflat_set_coarse_centroids",
    "vlq_ivfflat_set_lists", "vlq_ivfflat_add", "vlq_ivfflat_add_preassigned", "vlq_ivfflat_reserve_memory",
    "vlq_ivfflat_reclaim_memory", "vlq_ivfflat_ntotal", "vlq_ivfflat_list_length", "vlq_ivfflat_get_list", "vlq_ivfflat_reset",
    "vlq_ivfflat_coarse_search", "vlq_ivfflat_search", "vlq_ivfflat_search_preassigned", "vlq_ivfflat_stats",
    "vlq_ivfflat_last_scan_info",
    "vlq_ivfflat_range_search", "vlq_ivfflat_range_search_preassigned", "vlq_ivfflat_range_result",
    # IVF scalar quantizer (vlq_ivfsq_t)
    "vlq_ivfsq_create", "vlq_ivfsq_destroy", "vlq_ivfsq_set_stream", "vlq_ivfsq_set_coarse_centroids", "vlq_ivfsq_set_trained",
    "vlq_ivfsq_get_trained", "vlq_ivfsq_code_size", "vlq_ivfsq_set_lists", "vlq_ivfsq_add", "vlq_ivfsq_add_preassigned", "vlq_ivfsq_encode",
    "vlq_ivfsq_reserve_memory", "vlq_ivfsq_reclaim_memory", "vlq_ivfsq_ntotal", "vlq_ivfsq_list_length", "vlq_ivfsq_get_list",
    "vlq_ivfsq_reset", "vlq_ivfsq_coarse_search", "vlq_ivfsq_search", "vlq_ivfsq_search_preassigned", "vlq_ivfsq_last_scan_info",
    # flat PQ (vlq_pq_t)
    "vlq_pq_create", "vlq_pq_destroy", "vlq_pq_set_stream", "vlq_pq_set_centroids", "vlq_pq_set_codes", "vlq_pq_add", "vlq_pq_encode",
    "vlq_pq_get_codes", "vlq_pq_ntotal", "vlq_pq_reset", "vlq_pq_reserve_memory", "vlq_pq_set_search_type", "vlq_pq_search",
    "vlq_pq_query_tables", "vlq_pq_query_codes", "vlq_pq_stats", "vlq_pq_set_scan_split", "vlq_pq_last_scan_info",
    # flat scalar quantizer (vlq_sq_t)
    "vlq_sq_create", "vlq_sq_destroy", "vlq_sq_set_stream", "vlq_sq_set_trained", "vlq_sq_get_trained", "vlq_sq_code_size",
    "vlq_sq_set_codes", "vlq_sq_add", "vlq_sq_encode", "vlq_sq_get_codes", "vlq_sq_reconstruct", "vlq_sq_ntotal", "vlq_sq_reset",
    "vlq_sq_reserve_memory", "vlq_sq_search", "vlq_sq_set_scan_split", "vlq_sq_last_scan_info",
    # flat exact k-NN (vlq_flat_t)
    "vlq_flat_create", "vlq_flat_destroy", "vlq_flat_set_stream", "vlq_flat_add", "vlq_flat_ntotal", "vlq_flat_reset",
    "vlq_flat_reserve_memory", "vlq_flat_reconstruct_n", "vlq_flat_search", "vlq_flat_set_scan_split", "vlq_flat_last_scan_info",
    "vlq_flat_compute_distance_subset", "vlq_flat_refine", "vlq_flat_last_refine_info", "vlq_flat_range_search", "vlq_flat_range_result",
    # LSH: sign-bit codes and Hamming k-NN (vlq_lsh_t)
    "vlq_lsh_create", "vlq_lsh_destroy", "vlq_lsh_set_stream", "vlq_lsh_set_rotation", "vlq_lsh_set_thresholds", "vlq_lsh_apply",
    "vlq_lsh_encode", "vlq_lsh_add", "vlq_lsh_add_codes", "vlq_lsh_get_codes", "vlq_lsh_ntotal", "vlq_lsh_reset",
    "vlq_lsh_reserve_memory", "vlq_lsh_search", "vlq_lsh_search_codes", "vlq_lsh_set_scan_split", "vlq_lsh_last_scan_info",
    # include/vlq_line.h
    "vlq_line_set_float16_tables", "vlq_line_set_row_mode", "vlq_line_set_scan_parts", "vlq_line_create", "vlq_line_destroy", "vlq_line_set_stream", "vlq_line_set_coarse_centroids",
    "vlq_line_set_pq_centroids", "vlq_line_set_lambda_codebook", "vlq_line_set_graph",
    "vlq_line_build_graph", "vlq_line_assign", "vlq_line_residuals", "vlq_line_encode", "vlq_line_add",
    "vlq_line_set_lists", "vlq_line_ntotal", "vlq_line_list_length", "vlq_line_get_list",
    "vlq_line_search", "vlq_line_stats", "vlq_line_profile", "vlq_line_profile_read",
]


class VlqError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("vlq error %d: %s" % (code, msg))
        self.code = code


def library_path():
    return _SO


def build_library(force=False):
    """hipcc cross-compiles for gfx950 without a GPU present."""
    if force:
        subprocess.check_call(["make", "-s", "-C", _CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-C", _CSRC])
    return _SO


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own
    libamdhip64 (SONAME libamdhip64.so.7); if this library were loaded first it would
    pull the system copy and a later `import torch` would bring a second runtime
    that cannot open the device.  So when torch is installed but not yet imported,
    map torch's copy first: our NEEDED libamdhip64.so.7 then binds to it by SONAME."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise VlqError(-1, "HIP library %s is not built (run `make -C %s`); there is no "
                               "fallback path" % (_SO, _CSRC))
        _share_hip_runtime_with_torch()
        L = C.CDLL(_SO)
        L.vlq_last_error.restype = C.c_char_p
        L.vlq_ivfpq_ntotal.restype = C.c_int64
        L.vlq_ivfpq_destroy.restype = None
        L.vlq_ivfflat_ntotal.restype = C.c_int64
        L.vlq_ivfflat_destroy.restype = None
        L.vlq_ivfsq_ntotal.restype = C.c_int64
        L.vlq_ivfsq_destroy.restype = None
        L.vlq_pq_ntotal.restype = C.c_int64
        L.vlq_pq_destroy.restype = None
        L.vlq_sq_ntotal.restype = C.c_int64
        L.vlq_sq_destroy.restype = None
        L.vlq_flat_ntotal.restype = C.c_int64
        L.vlq_flat_destroy.restype = None
        L.vlq_lsh_ntotal.restype = C.c_int64
        L.vlq_lsh_destroy.restype = None
        L.vlq_line_ntotal.restype = C.c_int64
        L.vlq_line_destroy.restype = None
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise VlqError(rc, lib().vlq_last_error().decode(errors="replace"))


def device_count():
    return lib().vlq_device_count()
