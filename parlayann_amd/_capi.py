"""ctypes binding of the C-ABI in include/pann.h (libpann.so, built in-tree by csrc/Makefile).

The library is the product's only compute path: if it is missing, or no HIP device is visible,
callers get an exception -- there is no CPU fallback (DESIGN.md "No fallback").
"""
import ctypes as C
import os

# torch bundles its own libamdhip64.so; importing it first makes the dynamic loader resolve
# libpann.so's NEEDED libamdhip64.so.7 to that same copy, so tensors allocated by torch and kernels
# launched by libpann.so share ONE HIP runtime per process.
try:  # pragma: no cover - ordering shim only
    import torch  # noqa: F401
except Exception:  # torch is plumbing, not a requirement of the C-ABI
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpann.so")
if os.environ.get("PANN_LIBRARY"):      # A/B runs of diagnostic builds (tools/): same ABI, another file
    LIB_PATH = os.environ["PANN_LIBRARY"]

PANN_U8, PANN_I8, PANN_F32, PANN_F16, PANN_BF16, PANN_U4, PANN_I4 = 0, 1, 2, 3, 4, 5, 6
PANN_L2, PANN_MIPS = 0, 1
PANN_OK = 0
PANN_ERR_BAD_ARG, PANN_ERR_UNSUPPORTED = 1, 4
PANN_ERR_OVERFLOW = 5
PANN_ABI_VERSION = 3
PANN_STATUS_VISITED_OVERFLOW, PANN_STATUS_DROPPED_OVERFLOW, PANN_STATUS_SHORT_FRONTIER, PANN_STATUS_BAD_GROUP = 1, 2, 4, 8

u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
f32p = C.POINTER(C.c_float)


class QueryParams(C.Structure):
    """pann_query_params == QueryParams (algorithms/utils/types.h:218-231)."""
    _fields_ = [("k", C.c_int64), ("beam", C.c_int64), ("cut", C.c_double), ("limit", C.c_int64),
                ("degree_limit", C.c_int64), ("rerank_factor", C.c_int32), ("pad", C.c_float)]


class SearchOut(C.Structure):
    _fields_ = [("ids", C.c_void_p), ("dists", C.c_void_p), ("out_k", C.c_uint32),
                ("frontier_size", C.c_void_p), ("visited_count", C.c_void_p),
                ("dist_cmps", C.c_void_p), ("degree_sum", C.c_void_p),
                ("visited_ids", C.c_void_p), ("visited_dists", C.c_void_p),
                ("visited_cap", C.c_uint32), ("status", C.c_void_p)]


class RerankOut(C.Structure):
    """pann_rerank_out: outputs of pann_batch_search_rerank*; everything but ids and dists is optional."""
    _fields_ = [("ids", C.c_void_p), ("dists", C.c_void_p), ("frontier_size", C.c_void_p), ("visited_count", C.c_void_p),
                ("dist_cmps", C.c_void_p), ("pruned_cmps", C.c_void_p), ("status", C.c_void_p)]


class BuildStats(C.Structure):
    _fields_ = [("t_search_s", C.c_double), ("t_prune_s", C.c_double), ("t_bidirect_s", C.c_double),
                ("t_reprune_s", C.c_double), ("search_dist_cmps", C.c_uint64),
                ("prune_dist_cmps", C.c_uint64), ("visited_total", C.c_uint64),
                ("per_point_visited", C.c_void_p), ("per_point_dist_cmps", C.c_void_p)]


class DeleteStats(C.Structure):
    """pann_delete_stats: every field is added to by pann_vamana_delete_batch*"""
    _fields_ = [("t_expand_s", C.c_double), ("t_prune_s", C.c_double), ("deleted", C.c_uint64), ("affected", C.c_uint64),
                ("candidates", C.c_uint64), ("prune_dist_cmps", C.c_uint64), ("per_point_dist_cmps", C.c_void_p)]


class ReachStats(C.Structure):
    """pann_reach_stats: overwritten by pann_graph_reach*"""
    _fields_ = [("reached", C.c_uint64), ("unreached", C.c_uint64), ("max_frontier", C.c_uint64), ("levels", C.c_uint32),
                ("truncated", C.c_uint32), ("t_s", C.c_double)]


PANN_QUANT_EUCLID_U8, PANN_QUANT_MIPS_I8, PANN_QUANT_EUCLID_U4, PANN_QUANT_MIPS_I4 = 0, 1, 2, 3


class QuantParams(C.Structure):
    """pann_quant_params: Euclidian_Point<uint8_t>::parameters (slope, offset) / Quantized_Mips_Point<8>::parameters (max_val);
    the four-bit kinds use the same fields (range 15)."""
    _fields_ = [("kind", C.c_int32), ("dims", C.c_int32), ("slope", C.c_float), ("offset", C.c_int32),
                ("max_val", C.c_float), ("min_seen", C.c_float), ("max_seen", C.c_float)]

    @property
    def identity(self):
        return self.kind != PANN_QUANT_EUCLID_U4 and self.slope == 1.0 and self.offset == 0      # the 4-bit translate never casts


PANN_PRED_ANY, PANN_PRED_MATCH, PANN_PRED_RANGE = 0, 1, 2      # pann_label_pred kinds: two uint32 words (a, b) per predicate

PANN_SKETCH_EUCLID_BIT, PANN_SKETCH_MIPS_BIT, PANN_SKETCH_MIPS_2BIT = 0, 1, 2
PANN_SKETCH_MAX_DIMS = 2048


class SketchParams(C.Structure):
    """pann_sketch_params: Euclidean_Bit_Point::parameters (median) / Mips_2Bit_Point::parameters (cut); hamming_as_written
    selects the reference's one-bit distance loop as written (block 0 counted num_blocks times)."""
    _fields_ = [("kind", C.c_int32), ("dims", C.c_int32), ("median", C.c_int64), ("cut", C.c_float),
                ("hamming_as_written", C.c_uint32)]


# every symbol include/pann.h declares: (restype, argtypes)
SIGNATURES = {
    "pann_abi_version": (C.c_int, []),
    "pann_last_error": (C.c_char_p, []),
    "pann_device_count": (C.c_int, []),
    "pann_index_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.c_uint32, C.c_int,
                                    C.c_uint64, C.c_int, C.c_void_p, C.c_uint32, C.c_int]),
    "pann_index_create_empty": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_int]),
    "pann_index_upload_points": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]),
    "pann_index_destroy": (None, [C.c_void_p]),
    "pann_index_size": (C.c_uint64, [C.c_void_p]),
    "pann_index_dims": (C.c_uint32, [C.c_void_p]),
    "pann_index_max_degree": (C.c_uint32, [C.c_void_p]),
    "pann_index_device": (C.c_int, [C.c_void_p]),
    "pann_index_set_exact_float_order": (C.c_int, [C.c_void_p, C.c_int]),
    "pann_range_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                    C.c_int, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_index_reserve_dropped": (C.c_int, [C.c_void_p, C.c_uint32]),
    "pann_index_dropped_capacity": (C.c_uint32, [C.c_void_p]),
    "pann_index_set_graph": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pann_index_update_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "pann_index_get_graph": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pann_index_clear_graph": (C.c_int, [C.c_void_p]),
    "pann_index_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "pann_index_set_stream": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "pann_index_get_option": (C.c_int64, [C.c_void_p, C.c_char_p]),
    "pann_batch_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                    C.c_uint32, C.POINTER(QueryParams), C.POINTER(SearchOut)]),
    "pann_batch_search_per_query_starts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                                     C.c_void_p, C.c_uint32, C.POINTER(QueryParams), C.POINTER(SearchOut)]),
    "pann_batch_search_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                        C.c_uint32, C.POINTER(QueryParams), C.POINTER(SearchOut), C.c_void_p]),
    "pann_pair_distances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "pann_query_distances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                       C.c_void_p]),
    "pann_robust_prune_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_double, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]),
    "pann_vamana_insert_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_double, C.POINTER(BuildStats)]),
    "pann_vamana_build_single_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_uint32, C.c_uint64,
                                                 C.c_int, C.c_void_p]),
    "pann_vamana_build": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_uint64, C.c_int,
                                    C.POINTER(BuildStats)]),
    "pann_vamana_search_prune_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.c_double, C.c_void_p, C.POINTER(BuildStats)]),
    "pann_vamana_apply_rows_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_double,
                                             C.POINTER(BuildStats)]),
    "pann_vamana_sort_neighbors": (C.c_int, [C.c_void_p]),
    "pann_vamana_delete_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.POINTER(DeleteStats)]),
    "pann_vamana_delete_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_double,
                                               C.POINTER(DeleteStats)]),
    "pann_build_permutation": (None, [C.c_uint64, C.c_uint64, C.c_void_p]),
    "pann_vamana_batch_schedule": (C.c_uint64, [C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]),
    "pann_leaf_knn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pann_leaf_knn_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                      C.c_void_p]),
    "pann_rerank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                              C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]),
    "pann_pivot_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_hcnng_build": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p]),
    "pann_merge_topk_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_hcnng_build_trees_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                             C.c_void_p, C.c_uint32, C.c_void_p]),
    "pann_hcnng_assemble_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "pann_bruteforce_knn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p,
                                      C.c_void_p]),
    "pann_bruteforce_range": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_uint64]),
    "pann_range_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                   C.POINTER(QueryParams), C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "pann_index_normalize": (C.c_int, [C.c_void_p]),
    "pann_quantize_params": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(QuantParams)]),
    "pann_quantize_params_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int,
                                           C.POINTER(QuantParams), C.c_void_p]),
    "pann_index_create_quantized": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(QuantParams), C.c_int]),
    "pann_quantize_rows": (C.c_int, [C.POINTER(QuantParams), C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p,
                                     C.c_uint64, C.c_int]),
    "pann_quantize_rows_dev": (C.c_int, [C.POINTER(QuantParams), C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p,
                                         C.c_uint64, C.c_void_p]),
    "pann_index_download_points": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]),
    "pann_quantize_select_ranks": (None, [C.c_uint64, C.c_int, u64p, u64p]),
    "pann_sketch_params_generate": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(SketchParams)]),
    "pann_sketch_select_ranks": (None, [C.c_uint64, C.c_int, u64p, u64p]),
    "pann_index_attach_sketch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SketchParams)]),
    "pann_index_upload_sketch": (C.c_int, [C.c_void_p, C.POINTER(SketchParams), C.c_void_p, C.c_uint64]),
    "pann_index_drop_sketch": (C.c_int, [C.c_void_p]),
    "pann_index_sketch_kind": (C.c_int, [C.c_void_p]),
    "pann_index_download_sketch": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]),
    "pann_sketch_rows": (C.c_int, [C.POINTER(SketchParams), C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int]),
    "pann_sketch_rows_dev": (C.c_int, [C.POINTER(SketchParams), C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                       C.c_void_p]),
    "pann_batch_search_filtered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                             C.c_void_p, C.c_uint32, C.POINTER(QueryParams), C.POINTER(SearchOut), C.c_void_p]),
    "pann_batch_search_filtered_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                                 C.c_void_p, C.c_uint32, C.POINTER(QueryParams), C.POINTER(SearchOut), C.c_void_p,
                                                 C.c_void_p]),
    "pann_batch_search_masked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                           C.POINTER(QueryParams), C.c_void_p, C.c_uint64, C.POINTER(SearchOut), C.c_void_p, C.c_void_p]),
    "pann_batch_search_masked_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                               C.POINTER(QueryParams), C.c_void_p, C.c_uint64, C.POINTER(SearchOut), C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "pann_batch_search_rerank": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(QuantParams), C.c_void_p, C.c_uint64, C.c_uint64, C.c_int,
                                           C.c_int, C.c_void_p, C.c_uint32, C.POINTER(QueryParams), C.POINTER(RerankOut)]),
    "pann_batch_search_rerank_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(QuantParams), C.c_void_p, C.c_uint64, C.c_uint64,
                                               C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(QueryParams),
                                               C.POINTER(RerankOut), C.c_void_p]),
    "pann_batch_search_masked_rerank": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(QuantParams), C.c_void_p, C.c_uint64, C.c_uint64,
                                                  C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(QueryParams), C.c_void_p,
                                                  C.c_uint64, C.POINTER(RerankOut), C.c_void_p, C.c_void_p]),
    "pann_batch_search_masked_rerank_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(QuantParams), C.c_void_p, C.c_uint64,
                                                      C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(QueryParams),
                                                      C.c_void_p, C.c_uint64, C.POINTER(RerankOut), C.c_void_p, C.c_void_p,
                                                      C.c_void_p]),
    "pann_bruteforce_knn_masked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_bruteforce_knn_masked_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_allow_count_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "pann_index_set_labels": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "pann_index_set_labels_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "pann_index_get_labels": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "pann_index_drop_labels": (C.c_int, [C.c_void_p]),
    "pann_index_has_labels": (C.c_int, [C.c_void_p]),
    "pann_batch_search_labeled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                            C.POINTER(QueryParams), C.c_int, C.c_void_p, C.c_uint64, C.POINTER(SearchOut), C.c_void_p,
                                            C.c_void_p]),
    "pann_batch_search_labeled_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                                C.POINTER(QueryParams), C.c_int, C.c_void_p, C.c_uint64, C.POINTER(SearchOut),
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_batch_search_steered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                            C.POINTER(QueryParams), C.c_void_p, C.c_uint64, C.POINTER(SearchOut), C.c_void_p, C.c_void_p,
                                            C.c_uint32, C.c_void_p]),
    "pann_batch_search_steered_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                                C.POINTER(QueryParams), C.c_void_p, C.c_uint64, C.POINTER(SearchOut), C.c_void_p,
                                                C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pann_batch_search_steered_labeled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                                    C.POINTER(QueryParams), C.c_int, C.c_void_p, C.c_uint64, C.POINTER(SearchOut),
                                                    C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "pann_batch_search_steered_labeled_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                                        C.c_uint32, C.POINTER(QueryParams), C.c_int, C.c_void_p, C.c_uint64,
                                                        C.POINTER(SearchOut), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                        C.c_void_p]),
    "pann_batch_search_labeled_rerank": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(QuantParams), C.c_void_p, C.c_uint64, C.c_uint64,
                                                   C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(QueryParams), C.c_int,
                                                   C.c_void_p, C.c_uint64, C.POINTER(RerankOut), C.c_void_p, C.c_void_p]),
    "pann_batch_search_labeled_rerank_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(QuantParams), C.c_void_p, C.c_uint64,
                                                       C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(QueryParams),
                                                       C.c_int, C.c_void_p, C.c_uint64, C.POINTER(RerankOut), C.c_void_p, C.c_void_p,
                                                       C.c_void_p]),
    "pann_bruteforce_knn_labeled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p,
                                              C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_bruteforce_knn_labeled_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p,
                                                  C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_labels_to_allow_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "pann_label_count_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "pann_bruteforce_knn_labeled_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p,
                                                      C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_bruteforce_knn_labeled_grouped_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int,
                                                          C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_void_p]),
    "pann_bruteforce_knn_masked_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64,
                                                     C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_bruteforce_knn_masked_grouped_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p,
                                                         C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p]),
    "pann_batch_search_grouped_labeled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                                    C.c_uint64, C.POINTER(QueryParams), C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                                    C.POINTER(SearchOut), C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]),
    "pann_batch_search_grouped_labeled_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                                        C.c_uint32, C.c_uint64, C.POINTER(QueryParams), C.c_int, C.c_void_p, C.c_uint64,
                                                        C.c_void_p, C.POINTER(SearchOut), C.c_void_p, C.c_void_p, C.c_int, C.c_uint32,
                                                        C.c_void_p, C.c_void_p]),
    "pann_filter_medoids_labeled": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_filter_medoids_labeled_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_filter_medoids_masked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_filter_medoids_masked_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_index_create_subset_dev": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                                               C.c_uint64, C.c_void_p, u64p]),
    "pann_index_create_subset": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                                           C.c_uint64, C.c_void_p, u64p]),
    "pann_graph_reach_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_uint64, C.POINTER(ReachStats)]),
    "pann_graph_reach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_uint64, C.POINTER(ReachStats)]),
    "pann_graph_degrees_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pann_graph_degrees": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
}

_lib = None


class PannError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pann error {code}: {msg}")
        self.code = code


def load():
    """Load libpann.so and attach signatures.  Raises if the extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `make -C parlayann_amd/csrc` "
                          "(or __graft_entry__.build()); there is no fallback path")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != PANN_OK:
        raise PannError(rc, load().pann_last_error().decode("utf-8", "replace"))
