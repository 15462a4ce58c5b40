"""ctypes binding of the C-ABI declared in include/pgh.h (and the multi-seed loops of include/pgh_batch.h, the tuner's entries of
include/pgh_tune.h, the unsupervised measures' entries of include/pgh_measure.h, the supervised measures' entry of
include/pgh_supervised.h, the prior-editing entry of include/pgh_fair.h, the mixed batches of include/pgh_mixed.h, the locally fair PageRank's entries of
include/pgh_lfpr.h, the seed oversampling passes of include/pgh_oversample.h, the rank-based measures' entries of include/pgh_rank.h,
the Krylov-space filters' entries of include/pgh_krylov.h, the multi-group measures' entries of include/pgh_link.h, the Arnoldi
passes of include/pgh_arnoldi.h, the postprocessors' slab passes of include/pgh_post.h).

The product binds exactly one library: ``pygrank_amd/csrc/libpgh_hip.so`` (hand-written HIP for gfx950).
There is NO CPU fallback: if the library is missing, if it reports a runtime other than ``hip:*``, or if no MI355X is
visible when the engine is first used, an exception is raised.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libpgh_hip.so")

c_vec = C.c_void_p
c_mat = C.c_void_p
c_graph = C.c_void_p
c_timer = C.c_void_p
c_i64p = C.POINTER(C.c_int64)
c_i32p = C.POINTER(C.c_int32)
c_f32p = C.POINTER(C.c_float)
c_f64p = C.POINTER(C.c_double)


NORM_COL, NORM_SYMMETRIC, NORM_NONE, NORM_BOTH, NORM_LAPLACIAN = 0, 1, 2, 3, 4      # include/pgh.h PGH_NORM_*


class LoopCfg(C.Structure):
    _fields_ = [("alpha", C.c_double), ("use_quotient", C.c_int32), ("err_kind", C.c_int32), ("tol", C.c_double),
                ("max_iters", C.c_int32), ("end_modulo", C.c_int32), ("out_scale", C.c_double),
                ("in_norm", C.c_double), ("start_from_p", C.c_int32), ("reserved", C.c_int32)]


class LoopResult(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("spmv_count", C.c_int32),
                ("flags", C.c_int32), ("last_error", C.c_double), ("loop_ms", C.c_double), ("in_norm", C.c_double)]


class DistCfg(C.Structure):
    _fields_ = [("alpha", C.c_double), ("tol", C.c_double), ("n_global", C.c_int64), ("err_kind", C.c_int32), ("max_iters", C.c_int32),
                ("end_modulo", C.c_int32), ("use_quotient", C.c_int32), ("preserve_norm", C.c_int32), ("every_row", C.c_int32),
                ("deg_local", C.c_void_p), ("lam_local", C.c_void_p)]


class DistResult(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("spmv_count", C.c_int32), ("converged", C.c_int32), ("column_blocks", C.c_int32),
                ("split_regions", C.c_int32), ("flags", C.c_int32), ("last_error", C.c_double), ("loop_ms", C.c_double),
                ("exchange_bytes", C.c_int64), ("gather_slots", C.c_int64)]


COMM_ID_BYTES = 128
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p)
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64),
                           C.POINTER(C.c_int64), C.c_void_p)

# name -> (restype, argtypes); every symbol include/pgh.h declares
SIGNATURES = {
    "pgh_init": (C.c_int, [C.c_int]),
    "pgh_shutdown": (C.c_int, []),
    "pgh_last_error": (C.c_char_p, []),
    "pgh_runtime_name": (C.c_char_p, []),
    "pgh_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "pgh_device_name": (C.c_int, [C.c_char_p, C.c_int]),
    "pgh_mem_info": (C.c_int, [c_i64p, c_i64p]),
    "pgh_set_stream": (C.c_int, [C.c_void_p]),
    "pgh_sync": (C.c_int, []),
    "pgh_timer_create": (C.c_int, [C.POINTER(c_timer)]),
    "pgh_timer_destroy": (C.c_int, [c_timer]),
    "pgh_timer_start": (C.c_int, [c_timer]),
    "pgh_timer_stop": (C.c_int, [c_timer]),
    "pgh_timer_elapsed_ms": (C.c_int, [c_timer, c_f64p]),
    "pgh_profile_enable": (C.c_int, [C.c_int]),
    "pgh_profile_reset": (C.c_int, []),
    "pgh_profile_read": (C.c_int, [C.c_int, c_i64p, c_f64p]),
    "pgh_vec_alloc": (C.c_int, [C.c_int64, C.POINTER(c_vec)]),
    "pgh_vec_wrap": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(c_vec)]),
    "pgh_vec_free": (C.c_int, [c_vec]),
    "pgh_vec_len": (C.c_int64, [c_vec]),
    "pgh_vec_ptr": (C.c_void_p, [c_vec]),
    "pgh_vec_h2d_f32": (C.c_int, [c_vec, C.c_void_p, C.c_int64]),
    "pgh_vec_h2d_f64": (C.c_int, [c_vec, C.c_void_p, C.c_int64]),
    "pgh_vec_d2h_f32": (C.c_int, [c_vec, C.c_void_p, C.c_int64]),
    "pgh_vec_d2h_f64": (C.c_int, [c_vec, C.c_void_p, C.c_int64]),
    "pgh_vec_fill": (C.c_int, [c_vec, C.c_double]),
    "pgh_vec_copy": (C.c_int, [c_vec, c_vec]),
    "pgh_vec_get": (C.c_int, [c_vec, C.c_int64, c_f64p]),
    "pgh_vec_set": (C.c_int, [c_vec, C.c_int64, C.c_double]),
    "pgh_vec_scatter_set": (C.c_int, [c_vec, C.c_void_p, C.c_void_p, C.c_int64]),
    "pgh_ewise_vv": (C.c_int, [C.c_int, c_vec, c_vec, c_vec]),
    "pgh_ewise_vs": (C.c_int, [C.c_int, c_vec, C.c_double, C.c_int, c_vec]),
    "pgh_ewise_unary": (C.c_int, [C.c_int, c_vec, c_vec]),
    "pgh_axpby": (C.c_int, [C.c_double, c_vec, C.c_double, c_vec, c_vec]),
    "pgh_filter_out": (C.c_int, [c_vec, c_vec, c_vec, c_i64p]),
    "pgh_vec_ordinals": (C.c_int, [c_vec, c_vec]),
    "pgh_vec_kth_largest": (C.c_int, [c_vec, C.c_int64, c_f64p]),
    "pgh_auc": (C.c_int, [c_vec, c_vec, c_f64p, c_i64p]),
    "pgh_vec_gap_threshold": (C.c_int, [c_vec, c_f64p]),
    "pgh_reduce": (C.c_int, [C.c_int, c_vec, c_f64p]),
    "pgh_dot": (C.c_int, [c_vec, c_vec, c_f64p]),
    "pgh_residual": (C.c_int, [C.c_int, c_vec, c_vec, c_f64p]),
    "pgh_mat_alloc": (C.c_int, [C.c_int64, C.c_int32, C.POINTER(c_mat)]),
    "pgh_mat_free": (C.c_int, [c_mat]),
    "pgh_mat_shape": (C.c_int, [c_mat, c_i64p, c_i32p]),
    "pgh_mat_ptr": (C.c_void_p, [c_mat]),
    "pgh_mat_h2d_f64": (C.c_int, [c_mat, C.c_void_p]),
    "pgh_mat_d2h_f64": (C.c_int, [c_mat, C.c_void_p]),
    "pgh_mat_set_col": (C.c_int, [c_mat, C.c_int32, c_vec]),
    "pgh_mat_col_abssum": (C.c_int, [c_mat, C.c_void_p]),
    "pgh_mat_div_cols": (C.c_int, [c_mat, C.c_void_p, c_mat]),
    "pgh_mat_gemv": (C.c_int, [c_mat, C.c_void_p, C.c_int32, c_vec]),
    "pgh_mat_gemm": (C.c_int, [c_mat, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_mat]),
    "pgh_mat_get_cols": (C.c_int, [c_mat, C.c_int32, c_mat]),
    "pgh_mat_set_cols": (C.c_int, [c_mat, C.c_int32, c_mat]),
    "pgh_mat_get_col": (C.c_int, [c_mat, C.c_int32, c_vec]),
    "pgh_graph_from_csr": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.POINTER(c_graph)]),
    "pgh_graph_from_csr_part": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                          C.c_void_p, C.POINTER(c_graph)]),
    "pgh_graph_from_factored_csr": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_int, C.POINTER(c_graph)]),
    "pgh_graph_from_adjacency": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
                                           C.POINTER(c_graph)]),
    "pgh_graph_from_adjacency_ex": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double,
                                              C.c_int, C.POINTER(c_graph)]),
    "pgh_graph_destroy": (C.c_int, [c_graph]),
    "pgh_graph_info": (C.c_int, [c_graph, c_i64p, c_i64p, c_i64p, c_i64p]),
    "pgh_graph_format": (C.c_int, [c_graph, C.c_char_p, C.c_int]),
    "pgh_last_build_profile": (C.c_int, [C.c_char_p, C.c_int]),
    "pgh_graph_degrees": (C.c_int, [c_graph, c_vec]),
    "pgh_graph_degrees_dropout": (C.c_int, [c_graph, C.c_double, C.c_uint64, c_vec]),
    "pgh_graph_download": (C.c_int, [c_graph, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgh_spmv": (C.c_int, [c_graph, c_vec, c_vec]),
    "pgh_spmv_dropout": (C.c_int, [c_graph, c_vec, c_vec, C.c_double, C.c_uint64]),
    "pgh_ppr_step": (C.c_int, [c_graph, c_vec, C.c_double, c_vec, C.c_double, c_vec, c_f64p]),
    "pgh_absorb_step": (C.c_int, [c_graph, c_vec, C.c_double, c_vec, c_vec, c_vec, c_vec, c_f64p]),
    "pgh_poly_step": (C.c_int, [c_graph, c_vec, c_vec, C.c_double, C.c_double, c_vec, C.c_double, C.c_int, c_f64p]),
    "pgh_scaled_residual": (C.c_int, [C.c_int, c_vec, C.c_double, c_vec, C.c_double, c_f64p]),
    "pgh_graph_resident_len": (C.c_int, [c_graph, c_i64p, c_i64p]),
    "pgh_resident_in": (C.c_int, [c_graph, c_vec, C.c_double, c_vec, c_vec]),
    "pgh_resident_gather": (C.c_int, [c_graph, c_vec, c_vec]),
    "pgh_resident_out": (C.c_int, [c_graph, c_vec, C.c_double, c_vec]),
    "pgh_resident_step": (C.c_int, [c_graph, C.c_int32, c_vec, c_vec, C.c_double, c_vec, C.c_double, c_vec, c_vec, c_vec, c_vec, c_f64p]),
    "pgh_ppr_run": (C.c_int, [c_graph, c_vec, c_vec, C.POINTER(LoopCfg), C.POINTER(LoopResult)]),
    "pgh_ppr_run_f64": (C.c_int, [c_graph, c_vec, c_vec, C.POINTER(LoopCfg), C.POINTER(LoopResult)]),
    "pgh_absorb_run_f64": (C.c_int, [c_graph, c_vec, c_vec, c_vec, C.POINTER(LoopCfg), C.POINTER(LoopResult)]),
    "pgh_sarw_run_f64": (C.c_int, [c_graph, c_vec, c_vec, C.POINTER(LoopCfg), C.POINTER(LoopResult)]),
    "pgh_ppr_run_dropout": (C.c_int, [c_graph, c_vec, c_vec, C.POINTER(LoopCfg), C.c_double, C.c_uint64, C.POINTER(LoopResult)]),
    "pgh_absorb_run": (C.c_int, [c_graph, c_vec, c_vec, c_vec, C.POINTER(LoopCfg), C.POINTER(LoopResult)]),
    "pgh_sarw_run": (C.c_int, [c_graph, c_vec, c_vec, C.POINTER(LoopCfg), C.POINTER(LoopResult)]),
    "pgh_poly_run": (C.c_int, [c_graph, c_vec, C.c_void_p, C.c_int32, C.c_int32, c_vec, C.POINTER(LoopCfg),
                               C.POINTER(LoopResult)]),
    "pgh_poly_terms": (C.c_int, [c_graph, c_vec, C.c_int32, C.c_int32, C.c_int32, c_mat, C.c_int32]),
    "pgh_spmm": (C.c_int, [c_graph, c_mat, c_mat]),
    "pgh_ppr_run_batch": (C.c_int, [c_graph, c_mat, c_mat, C.POINTER(LoopCfg), C.c_void_p, C.POINTER(LoopResult)]),
    "pgh_spmm_dropout": (C.c_int, [c_graph, c_mat, c_mat, C.c_double, C.c_uint64]),
    "pgh_ppr_run_batch_dropout": (C.c_int, [c_graph, c_mat, c_mat, C.POINTER(LoopCfg), C.c_void_p, C.c_double, C.c_uint64,
                                            C.POINTER(LoopResult)]),
    "pgh_ppr_step_dist": (C.c_int, [c_graph, c_vec, C.c_double, c_vec, C.c_double, c_vec, c_vec, c_f64p]),
    "pgh_graph_gather_layout": (C.c_int, [c_graph, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_void_p]),
    "pgh_graph_set_gather_bases": (C.c_int, [c_graph, C.c_void_p]),
    "pgh_dist_state_init": (C.c_int, [C.c_void_p]),
    "pgh_dist_partial": (C.c_int, [c_graph, c_vec, C.c_void_p]),
    "pgh_dist_partial_stage": (C.c_int, [c_graph, c_vec, C.c_void_p, C.c_int32]),
    "pgh_graph_hot_prefix": (C.c_int, [c_graph, C.POINTER(C.c_int32)]),
    "pgh_dist_combine": (C.c_int, [c_graph, c_vec, C.c_double, c_vec, c_vec, C.c_void_p]),
    "pgh_dist_combine_absorb": (C.c_int, [c_graph, c_vec, c_vec, c_vec, c_vec, c_vec, C.c_void_p]),
    "pgh_dist_combine_poly": (C.c_int, [c_graph, c_vec, c_vec, C.c_double, C.c_double, c_vec, C.c_double, C.c_int32, c_vec, C.c_void_p]),
    "pgh_dist_close_sum": (C.c_int, [C.c_void_p, C.c_int32]),
    "pgh_dist_watch_isolated": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgh_dist_release_isolated": (C.c_int, [C.c_void_p]),
    "pgh_dist_residual": (C.c_int, [C.c_int32, c_vec, c_vec, C.c_void_p]),
    "pgh_dist_need_counts": (C.c_int, [c_graph, C.c_void_p]),
    "pgh_dist_need_list": (C.c_int, [c_graph, C.c_int32, C.c_void_p]),
    "pgh_dist_set_send_lists": (C.c_int, [c_graph, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "pgh_dist_pack": (C.c_int, [c_graph, c_vec, c_vec]),
    "pgh_dist_compact_from_dense": (C.c_int, [c_graph, C.c_int32, c_vec, C.c_int64, c_vec, C.c_int64]),
    "pgh_dist_close_err": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_int64]),
    "pgh_dist_prescale": (C.c_int, [c_graph, c_vec, c_vec]),
    "pgh_graph_perm": (C.c_int, [c_graph, C.c_void_p, c_i64p]),
    "pgh_graph_set_gather_bases_split": (C.c_int, [c_graph, C.c_void_p, C.c_void_p]),
    "pgh_comm_unique_id": (C.c_int, [C.c_void_p]),
    "pgh_comm_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "pgh_comm_create_external": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "pgh_comm_set_alltoallv": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pgh_comm_destroy": (C.c_int, [C.c_void_p]),
    "pgh_dist_ppr_run": (C.c_int, [c_graph, C.c_void_p, c_vec, c_vec, C.POINTER(DistCfg), C.POINTER(DistResult)]),
    "pgh_dist_poly_run": (C.c_int, [c_graph, C.c_void_p, c_vec, C.c_void_p, C.c_int32, c_vec, C.POINTER(DistCfg), C.POINTER(DistResult)]),
    "pgh_dist_set_timeout": (C.c_int, [C.c_double]),
    "pgh_graph_rmat_part": (C.c_int, [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_uint64, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_int32, C.POINTER(c_graph)]),
    "pgh_graph_rmat": (C.c_int, [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_uint64, C.c_int32,
                                 C.c_int32, C.c_int64, C.c_int64, C.POINTER(c_graph)]),
}

# enum values of include/pgh.h
ADD, SUB, MUL, DIV, POW, MAXOP, MINOP, GT, GE, LT, LE, EQ, NE = range(13)
ABS, EXP, LOG, NEG, SQRT, SAFE_INV = range(6)
SUM, ABSSUM, MAX, MIN = range(4)
ERR_MABS, ERR_L1, ERR_LINF, ERR_ITERS = range(4)
K_SPMV, K_FIXUP, K_RESIDUAL, K_FINAL, K_SPMM, K_COMBINE, K_PB_GATHER, K_PB_ACCUM, K_PACK = range(9)

# name -> (restype, argtypes); every symbol include/pgh_batch.h declares.  Bound apart from SIGNATURES (batch_entry): a library
# without them -- the host test double under oracle/ -- still loads, and the filters run such batches column by column.
BATCH_SIGNATURES = {
    "pgh_poly_run_batch": (C.c_int, [c_graph, c_mat, C.c_void_p, C.c_int32, c_mat, C.POINTER(LoopCfg), C.c_void_p,
                                     C.POINTER(LoopResult)]),
    "pgh_absorb_run_batch": (C.c_int, [c_graph, c_mat, c_vec, c_mat, C.POINTER(LoopCfg), C.c_void_p, C.POINTER(LoopResult)]),
    "pgh_sarw_run_batch": (C.c_int, [c_graph, c_mat, c_mat, C.POINTER(LoopCfg), C.c_void_p, C.POINTER(LoopResult)]),
}
BATCH_DECLINED = 2        # include/pgh_batch.h PGH_BATCH_DECLINED: the loop does not serve this input, nothing was written

# name -> (restype, argtypes); every symbol include/pgh_tune.h declares.  Bound apart like the batch loops (tune_entry): on a library
# without them the tuner scores its probes column by column.
c_plan = C.c_void_p
TUNE_SIGNATURES = {
    "pgh_probe_plan_create": (C.c_int, [c_vec, c_vec, C.POINTER(c_plan)]),
    "pgh_probe_plan_info": (C.c_int, [c_plan, c_i64p, c_i64p]),
    "pgh_probe_plan_destroy": (C.c_int, [c_plan]),
    "pgh_probe_auc": (C.c_int, [c_mat, C.c_void_p, C.c_int32, C.c_int32, c_plan, c_f64p]),
}
TUNE_DECLINED = 2         # include/pgh_tune.h PGH_TUNE_DECLINED: nothing was written, the caller takes the unfused route
TUNE_LDS_BYTES = 61440    # include/pgh_tune.h PGH_TUNE_LDS_BYTES
TUNE_MAX_POSITIVES = 8192 # include/pgh_tune.h PGH_TUNE_MAX_POSITIVES

# name -> (restype, argtypes); every symbol include/pgh_measure.h declares.  Bound apart like the tuner's entries (measure_entry): on a
# library without them Conductance and Density take the reference's route, one backend primitive at a time.
MEASURE_SIGNATURES = {
    "pgh_mat_col_stats": (C.c_int, [c_mat, C.c_void_p]),
    "pgh_cut_forms": (C.c_int, [c_graph, c_mat, C.c_void_p, C.c_double, C.c_int32, C.c_void_p]),
}
MEASURE_DECLINED = 2      # include/pgh_measure.h PGH_MEASURE_DECLINED: nothing was written, the caller takes the per-column route
CUT_ALL, CUT_INTERNAL = 0, 1                                                        # include/pgh_measure.h PGH_CUT_*

# name -> (restype, argtypes); every symbol include/pgh_supervised.h declares.  Bound apart like the measures' entries
# (supervised_entry): on a library without it every supervised measure takes the reference's route, one backend primitive at a time.
SUPERVISED_SIGNATURES = {
    "pgh_pair_forms": (C.c_int, [c_mat, c_vec, c_mat, c_vec, c_mat, C.c_void_p, C.c_double, C.c_int32, C.c_void_p]),
}
PAIR_DECLINED = 2         # include/pgh_supervised.h PGH_PAIR_DECLINED: nothing was written, the caller takes the per-column route
PAIR_SLOTS = 20           # include/pgh_supervised.h PGH_PAIR_SLOTS: doubles written per column
PAIR_MOMENTS, PAIR_LOGS = 0, 1                                                      # include/pgh_supervised.h PGH_PAIR_*

# name -> (restype, argtypes); every symbol include/pgh_fair.h declares.  Bound apart like the supervised measures' entry (fair_entry):
# on a library without it FairPersonalizer builds every candidate's edited prior from backend operations.
FAIR_SIGNATURES = {
    "pgh_prior_edit": (C.c_int, [c_vec, c_vec, c_vec, C.c_double, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_mat]),
}
FAIR_DECLINED = 2         # include/pgh_fair.h PGH_FAIR_DECLINED: nothing was written, the caller takes the per-candidate route
FAIR_MAX_PROBES = 64      # include/pgh_fair.h PGH_FAIR_MAX_PROBES
FAIR_MAX_BUCKETS = 4      # include/pgh_fair.h PGH_FAIR_MAX_BUCKETS

# name -> (restype, argtypes); every symbol include/pgh_mixed.h declares.  Bound apart like the prior-editing entry (mixed_entry): on a
# library without them AlgorithmSelection runs every candidate filter one by one.
MIXED_SIGNATURES = {
    "pgh_ppr_run_batch_mixed": (C.c_int, [c_graph, c_mat, c_mat, C.POINTER(LoopCfg), C.c_void_p, C.c_void_p, C.POINTER(LoopResult)]),
    "pgh_poly_run_batch_mixed": (C.c_int, [c_graph, c_mat, C.c_void_p, C.c_int32, c_mat, C.POINTER(LoopCfg), C.c_void_p,
                                           C.POINTER(LoopResult)]),
}
MIXED_DECLINED = 2        # include/pgh_mixed.h PGH_MIXED_DECLINED: nothing was written, the caller runs the columns one by one

# name -> (restype, argtypes); every symbol include/pgh_lfpr.h declares.  Bound apart like the mixed batches (lfpr_entry): on a library
# without them LFPR takes the reference's route, one backend primitive at a time.
LFPR_SIGNATURES = {
    "pgh_lfpr_setup": (C.c_int, [c_vec, c_vec, c_vec, c_vec, C.c_double, c_vec, c_vec, c_vec, c_vec, c_vec, c_f64p]),
    "pgh_lfpr_close": (C.c_int, [c_vec, c_vec, C.c_double, c_vec, c_vec, c_vec, c_vec, c_vec, C.c_double, C.c_double, C.c_double,
                                 C.c_int32, c_vec, c_vec, c_f64p]),
}
LFPR_DECLINED = 2         # include/pgh_lfpr.h PGH_LFPR_DECLINED: nothing was written, the caller takes the backend-primitive route

# name -> (restype, argtypes); every symbol include/pgh_oversample.h declares.  Bound apart like LFPR's entries (oversample_entry): on a
# library without them SeedOversampling and BoostedSeedOversampling take the backend-primitive route.
OVERSAMPLE_SIGNATURES = {
    "pgh_seed_floor": (C.c_int, [c_mat, c_mat, c_f64p, c_i64p]),
    "pgh_seed_resample": (C.c_int, [c_mat, c_f64p, C.c_int32, c_mat, c_mat, c_i64p]),
    "pgh_boost_forms": (C.c_int, [c_mat, c_mat, c_mat, c_f64p]),
    "pgh_boost_update": (C.c_int, [c_mat, c_mat, c_f64p, c_mat, c_f64p, c_i64p]),
}
OVERSAMPLE_DECLINED = 2   # include/pgh_oversample.h PGH_OVERSAMPLE_DECLINED: nothing was written, the caller takes the backend-primitive route
OVERSAMPLE_MAX_COLS = 64  # include/pgh_oversample.h PGH_OVERSAMPLE_MAX_COLS

# name -> (restype, argtypes); every symbol include/pgh_rank.h declares.  Bound apart like the oversampling passes (rank_entry): on a
# library without them NDCG and SpearmanCorrelation take the columns route.
c_rank_plan = C.c_void_p
RANK_SIGNATURES = {
    "pgh_rank_plan_create": (C.c_int, [c_vec, c_vec, C.POINTER(c_rank_plan)]),
    "pgh_rank_plan_info": (C.c_int, [c_rank_plan, c_i64p, c_i64p, c_i32p]),
    "pgh_rank_plan_destroy": (C.c_int, [c_rank_plan]),
    "pgh_ndcg": (C.c_int, [c_mat, c_rank_plan, C.c_int64, C.c_int32, c_f64p, c_f64p]),
    "pgh_spearman": (C.c_int, [c_mat, c_rank_plan, c_f64p]),
    "pgh_ndcg_vec": (C.c_int, [c_vec, c_rank_plan, C.c_int64, C.c_int32, c_f64p, c_f64p]),
    "pgh_spearman_vec": (C.c_int, [c_vec, c_rank_plan, c_f64p]),
}
RANK_DECLINED = 2         # include/pgh_rank.h PGH_RANK_DECLINED: nothing was written, the caller takes the columns route
RANK_MAX_RELEVANT = 8192  # include/pgh_rank.h PGH_RANK_MAX_RELEVANT
RANK_LDS_BYTES = 61440    # include/pgh_rank.h PGH_RANK_LDS_BYTES
RANK_AUTO, RANK_STREAMING, RANK_SORTED = 0, 1, 2                                    # include/pgh_rank.h PGH_RANK_*

# name -> (restype, argtypes); every symbol include/pgh_krylov.h declares.  Bound apart like LFPR's entries (krylov_entry): on a library
# without them the Krylov-space filters take the reference's route, one backend primitive at a time.
KRYLOV_SIGNATURES = {
    "pgh_lanczos_close": (C.c_int, [c_vec, c_vec, C.c_double, c_vec, C.c_double, c_vec, c_mat, C.c_int32, c_f64p]),
    "pgh_krylov_residuals": (C.c_int, [c_mat, c_f64p, C.c_int32, C.c_int32, c_f64p, c_f64p]),
}
KRYLOV_DECLINED = 2       # include/pgh_krylov.h PGH_KRYLOV_DECLINED: nothing was written, the caller takes the backend-primitive route
KRYLOV_MAX_DIMS = 64      # include/pgh_krylov.h PGH_KRYLOV_MAX_DIMS
KRYLOV_MAX_PROBES = 64    # include/pgh_krylov.h PGH_KRYLOV_MAX_PROBES

# name -> (restype, argtypes); every symbol include/pgh_link.h declares.  Bound apart like the Krylov entries (link_entry): on a library
# without them LinkAssessment and ClusteringCoefficient score the downloaded slab with numpy.
c_link_plan = C.c_void_p
LINK_SIGNATURES = {
    "pgh_link_plan_create": (C.c_int, [C.c_int64, C.c_int64, c_i32p, c_i32p, C.POINTER(C.c_uint8), C.POINTER(c_link_plan)]),
    "pgh_link_plan_info": (C.c_int, [c_link_plan, c_i64p, c_i64p, c_i64p]),
    "pgh_link_plan_destroy": (C.c_int, [c_link_plan]),
    "pgh_link_auc": (C.c_int, [c_mat, c_link_plan, C.c_int32, c_f64p, c_i64p, c_i64p]),
    "pgh_link_predictions": (C.c_int, [c_mat, c_link_plan, C.c_int32, C.c_int64, C.c_int64, c_f64p]),
    "pgh_link_factors": (C.c_int, [c_mat, C.c_int32, c_vec]),
}
LINK_DECLINED = 2         # include/pgh_link.h PGH_LINK_DECLINED: nothing was written, the caller scores the downloaded slab on the host
LINK_MAX_PAIRS = 1 << 27  # include/pgh_link.h PGH_LINK_MAX_PAIRS
LINK_COS, LINK_DOT = 0, 1                                                           # include/pgh_link.h PGH_LINK_*

# name -> (restype, argtypes); every symbol include/pgh_arnoldi.h declares.  Bound apart like the Krylov entries (arnoldi_entry): on a
# library without them arnoldi_iteration takes the reference's route, one backend primitive at a time.
ARNOLDI_SIGNATURES = {
    "pgh_basis_dots": (C.c_int, [c_mat, C.c_int32, c_vec, c_f64p]),
    "pgh_arnoldi_close": (C.c_int, [c_mat, C.c_int32, c_vec, c_f64p, c_vec, C.c_int32, c_f64p]),
}
ARNOLDI_DECLINED = 2      # include/pgh_arnoldi.h PGH_ARNOLDI_DECLINED: nothing was written, the caller takes the backend-primitive route
ARNOLDI_MAX_DIMS = 64     # include/pgh_arnoldi.h PGH_ARNOLDI_MAX_DIMS

# name -> (restype, argtypes); every symbol include/pgh_post.h declares.  Bound apart like the Arnoldi entries (post_entry): on a library
# without them a postprocessor's propagate transforms the columns of the inner ranker's batch one by one.
POST_SIGNATURES = {
    "pgh_post_kth_largest": (C.c_int, [c_mat, C.c_int64, c_f64p]),
    "pgh_post_col_threshold": (C.c_int, [c_mat, c_f64p, C.c_int32, c_mat]),
    "pgh_post_col_affine": (C.c_int, [c_mat, c_f64p, c_f64p, c_mat]),
    "pgh_post_row_op": (C.c_int, [c_mat, c_vec, C.c_int32, C.c_double, c_mat]),
    "pgh_post_ordinals": (C.c_int, [c_mat, c_mat]),
}
POST_DECLINED = 2         # include/pgh_post.h PGH_POST_DECLINED: nothing was written, the caller takes the columns route
POST_MAX_COLS = 64        # include/pgh_post.h PGH_POST_MAX_COLS
POST_ROW_SUB, POST_ROW_SWEEP = 0, 1                                                 # include/pgh_post.h PGH_POST_ROW_*

_lib = None
_initialised = False
ACCEPTED_RUNTIMES = ("hip:",)      # pgh_runtime_name() prefixes ensure_init() agrees to drive


class EngineError(Exception):
    """Raised for every non-zero status of the C-ABI (the reference raises plain Exception)."""


def _bind(cdll):
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(cdll, name)      # AttributeError if the library does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    return cdll


def _bind_optional(cdll, table):
    bound = {}
    for name, (restype, argtypes) in table.items():
        try:
            fn = getattr(cdll, name)
        except AttributeError:
            bound[name] = None
            continue
        fn.restype = restype
        fn.argtypes = argtypes
        bound[name] = fn
    return bound


def bind_batch(cdll):
    """Binds the include/pgh_batch.h entries `cdll` exports; returns {name: function or None when the library lacks it}."""
    return _bind_optional(cdll, BATCH_SIGNATURES)


def bind_tune(cdll):
    """Binds the include/pgh_tune.h entries `cdll` exports; returns {name: function or None when the library lacks it}."""
    return _bind_optional(cdll, TUNE_SIGNATURES)


def bind_measure(cdll):
    """Binds the include/pgh_measure.h entries `cdll` exports; returns {name: function or None when the library lacks it}."""
    return _bind_optional(cdll, MEASURE_SIGNATURES)


def bind_supervised(cdll):
    """Binds the include/pgh_supervised.h entries `cdll` exports; returns {name: function or None when the library lacks it}."""
    return _bind_optional(cdll, SUPERVISED_SIGNATURES)


def bind_fair(cdll):
    """Binds the include/pgh_fair.h entries `cdll` exports; returns {name: function or None when the library lacks it}."""
    return _bind_optional(cdll, FAIR_SIGNATURES)


def bind_mixed(cdll):
    """Binds the include/pgh_mixed.h entries `cdll` exports; returns {name: function or None when the library lacks it}."""
    return _bind_optional(cdll, MIXED_SIGNATURES)


def bind_lfpr(cdll):
    """Binds the include/pgh_lfpr.h entries `cdll` exports; returns {name: function or None when the library lacks it}."""
    return _bind_optional(cdll, LFPR_SIGNATURES)


def bind_oversample(cdll):
    """Binds the include/pgh_oversample.h entries `cdll` exports; returns {name: function or None when the library lacks it}."""
    return _bind_optional(cdll, OVERSAMPLE_SIGNATURES)


def bind_rank(cdll):
    """Binds the include/pgh_rank.h entries `cdll` exports; returns {name: function or None when the library lacks it}."""
    return _bind_optional(cdll, RANK_SIGNATURES)


def bind_krylov(cdll):
    """Binds the include/pgh_krylov.h entries `cdll` exports; returns {name: function or None when the library lacks it}."""
    return _bind_optional(cdll, KRYLOV_SIGNATURES)


def bind_link(cdll):
    """Binds the include/pgh_link.h entries `cdll` exports; returns {name: function or None when the library lacks it}."""
    return _bind_optional(cdll, LINK_SIGNATURES)


def bind_arnoldi(cdll):
    """Binds the include/pgh_arnoldi.h entries `cdll` exports; returns {name: function or None when the library lacks it}."""
    return _bind_optional(cdll, ARNOLDI_SIGNATURES)


def bind_post(cdll):
    """Binds the include/pgh_post.h entries `cdll` exports; returns {name: function or None when the library lacks it}."""
    return _bind_optional(cdll, POST_SIGNATURES)


def post_entry(name):
    """The bound include/pgh_post.h entry `name` of the loaded library, or None when that library does not export it."""
    cdll = lib()
    cache = getattr(cdll, "_pgh_post_entries", None)
    if cache is None:
        cache = bind_post(cdll)
        cdll._pgh_post_entries = cache
    return cache[name]


def arnoldi_entry(name):
    """The bound include/pgh_arnoldi.h entry `name` of the loaded library, or None when that library does not export it."""
    cdll = lib()
    cache = getattr(cdll, "_pgh_arnoldi_entries", None)
    if cache is None:
        cache = bind_arnoldi(cdll)
        cdll._pgh_arnoldi_entries = cache
    return cache[name]


def link_entry(name):
    """The bound include/pgh_link.h entry `name` of the loaded library, or None when that library does not export it."""
    cdll = lib()
    cache = getattr(cdll, "_pgh_link_entries", None)
    if cache is None:
        cache = bind_link(cdll)
        cdll._pgh_link_entries = cache
    return cache[name]


def krylov_entry(name):
    """The bound include/pgh_krylov.h entry `name` of the loaded library, or None when that library does not export it."""
    cdll = lib()
    cache = getattr(cdll, "_pgh_krylov_entries", None)
    if cache is None:
        cache = bind_krylov(cdll)
        cdll._pgh_krylov_entries = cache
    return cache[name]


def rank_entry(name):
    """The bound include/pgh_rank.h entry `name` of the loaded library, or None when that library does not export it."""
    cdll = lib()
    cache = getattr(cdll, "_pgh_rank_entries", None)
    if cache is None:
        cache = bind_rank(cdll)
        cdll._pgh_rank_entries = cache
    return cache[name]


def oversample_entry(name):
    """The bound include/pgh_oversample.h entry `name` of the loaded library, or None when that library does not export it."""
    cdll = lib()
    cache = getattr(cdll, "_pgh_oversample_entries", None)
    if cache is None:
        cache = bind_oversample(cdll)
        cdll._pgh_oversample_entries = cache
    return cache[name]


def lfpr_entry(name):
    """The bound include/pgh_lfpr.h entry `name` of the loaded library, or None when that library does not export it."""
    cdll = lib()
    cache = getattr(cdll, "_pgh_lfpr_entries", None)
    if cache is None:
        cache = bind_lfpr(cdll)
        cdll._pgh_lfpr_entries = cache
    return cache[name]


def mixed_entry(name):
    """The bound include/pgh_mixed.h entry `name` of the loaded library, or None when that library does not export it."""
    cdll = lib()
    cache = getattr(cdll, "_pgh_mixed_entries", None)
    if cache is None:
        cache = bind_mixed(cdll)
        cdll._pgh_mixed_entries = cache
    return cache[name]


def fair_entry(name):
    """The bound include/pgh_fair.h entry `name` of the loaded library, or None when that library does not export it."""
    cdll = lib()
    cache = getattr(cdll, "_pgh_fair_entries", None)
    if cache is None:
        cache = bind_fair(cdll)
        cdll._pgh_fair_entries = cache
    return cache[name]


def supervised_entry(name):
    """The bound include/pgh_supervised.h entry `name` of the loaded library, or None when that library does not export it."""
    cdll = lib()
    cache = getattr(cdll, "_pgh_supervised_entries", None)
    if cache is None:
        cache = bind_supervised(cdll)
        cdll._pgh_supervised_entries = cache
    return cache[name]


def measure_entry(name):
    """The bound include/pgh_measure.h entry `name` of the loaded library, or None when that library does not export it."""
    cdll = lib()
    cache = getattr(cdll, "_pgh_measure_entries", None)
    if cache is None:
        cache = bind_measure(cdll)
        cdll._pgh_measure_entries = cache
    return cache[name]


def tune_entry(name):
    """The bound include/pgh_tune.h entry `name` of the loaded library, or None when that library does not export it."""
    cdll = lib()
    cache = getattr(cdll, "_pgh_tune_entries", None)
    if cache is None:
        cache = bind_tune(cdll)
        cdll._pgh_tune_entries = cache
    return cache[name]


def batch_entry(name):
    """The bound include/pgh_batch.h entry `name` of the loaded library, or None when that library does not export it."""
    cdll = lib()
    cache = getattr(cdll, "_pgh_batch_entries", None)
    if cache is None:
        cache = bind_batch(cdll)
        cdll._pgh_batch_entries = cache
    return cache[name]


def load_library(path=None):
    """dlopen + bind without touching the GPU (used by the build check and the symbol test)."""
    path = LIB_PATH if path is None else path
    if not os.path.exists(path):
        raise EngineError(
            f"MI355X engine library not found at {path}: build it with `make -C pygrank_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    return _bind(C.CDLL(path))


def lib():
    """The bound engine library; loads the HIP build on first use."""
    global _lib
    if _lib is None:
        _lib = load_library()
    return _lib


def check(status):
    if status != 0:
        msg = lib().pgh_last_error()
        raise EngineError(msg.decode("utf-8", "replace") if msg else f"engine call failed with status {status}")


def ensure_init(device=None):
    """backend_init(): selects the GPU (LOCAL_RANK when launched by torch.distributed.run) and fails loudly
    when none is visible."""
    global _initialised
    if _initialised:
        return
    L = lib()
    name = L.pgh_runtime_name().decode()
    if not name.startswith(ACCEPTED_RUNTIMES):
        raise EngineError(f"refusing to run the product path on runtime '{name}'")
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    check(L.pgh_init(int(device)))
    _initialised = True


def runtime_name():
    return lib().pgh_runtime_name().decode()
