"""ctypes binding of the C-ABI: include/pgh.h, which every engine library exports in full, and the optional headers
include/pgh_*.h (TABLES below), one per fused entry family.

Every symbol of SIGNATURES is bound when the library loads; a library that lacks one does not load.  The optional tables are bound
apart, on the first ``entry(name)``: a library without them -- the host test double under oracle/ -- still loads, ``entry`` returns
None for it, and each caller then takes its unfused route (named beside its table).  Every optional entry may also return DECLINED:
it does not serve this input and wrote nothing, and the caller takes that same route; ``accepted(status)`` tells the two apart.

A header's bound table lives on the library object as ``_pgh_<family>_entries`` (include/pgh_lfpr.h: ``_pgh_lfpr_entries``).  That
attribute is the hook of the host tests: they put numpy stand-ins for one family's entries there and take them out again.

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

# name -> (restype, argtypes), here and in every table below; every symbol include/pgh.h declares
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

# include/pgh_batch.h.  Unfused route: the filters run such batches column by column.
BATCH_SIGNATURES = {
    "pgh_poly_run_batch": (C.c_int, [c_graph, c_mat, C.c_void_p, C.c_int32, c_mat, C.POINTER(LoopCfg), C.c_void_p,
                                     C.POINTER(LoopResult)]),
    "pgh_absorb_run_batch": (C.c_int, [c_graph, c_mat, c_vec, c_mat, C.POINTER(LoopCfg), C.c_void_p, C.POINTER(LoopResult)]),
    "pgh_sarw_run_batch": (C.c_int, [c_graph, c_mat, c_mat, C.POINTER(LoopCfg), C.c_void_p, C.POINTER(LoopResult)]),
}

# include/pgh_tune.h.  Unfused route: the tuner scores its probes column by column.
c_plan = C.c_void_p
TUNE_SIGNATURES = {
    "pgh_probe_plan_create": (C.c_int, [c_vec, c_vec, C.POINTER(c_plan)]),
    "pgh_probe_plan_info": (C.c_int, [c_plan, c_i64p, c_i64p]),
    "pgh_probe_plan_destroy": (C.c_int, [c_plan]),
    "pgh_probe_auc": (C.c_int, [c_mat, C.c_void_p, C.c_int32, C.c_int32, c_plan, c_f64p]),
}
TUNE_LDS_BYTES = 61440    # include/pgh_tune.h PGH_TUNE_LDS_BYTES
TUNE_MAX_POSITIVES = 8192 # include/pgh_tune.h PGH_TUNE_MAX_POSITIVES

# include/pgh_measure.h.  Unfused route: Conductance and Density take the reference's route, one backend primitive at a time.
MEASURE_SIGNATURES = {
    "pgh_mat_col_stats": (C.c_int, [c_mat, C.c_void_p]),
    "pgh_cut_forms": (C.c_int, [c_graph, c_mat, C.c_void_p, C.c_double, C.c_int32, C.c_void_p]),
}
CUT_ALL, CUT_INTERNAL = 0, 1                                                        # include/pgh_measure.h PGH_CUT_*

# include/pgh_supervised.h.  Unfused route: every supervised measure takes the reference's route, one backend primitive at a time.
SUPERVISED_SIGNATURES = {
    "pgh_pair_forms": (C.c_int, [c_mat, c_vec, c_mat, c_vec, c_mat, C.c_void_p, C.c_double, C.c_int32, C.c_void_p]),
}
PAIR_SLOTS = 20           # include/pgh_supervised.h PGH_PAIR_SLOTS: doubles written per column
PAIR_MOMENTS, PAIR_LOGS = 0, 1                                                      # include/pgh_supervised.h PGH_PAIR_*

# include/pgh_fair.h.  Unfused route: FairPersonalizer builds every candidate's edited prior from backend operations.
FAIR_SIGNATURES = {
    "pgh_prior_edit": (C.c_int, [c_vec, c_vec, c_vec, C.c_double, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_mat]),
}
FAIR_MAX_PROBES = 64      # include/pgh_fair.h PGH_FAIR_MAX_PROBES
FAIR_MAX_BUCKETS = 4      # include/pgh_fair.h PGH_FAIR_MAX_BUCKETS

# include/pgh_mixed.h.  Unfused route: AlgorithmSelection runs every candidate filter one by one.
MIXED_SIGNATURES = {
    "pgh_ppr_run_batch_mixed": (C.c_int, [c_graph, c_mat, c_mat, C.POINTER(LoopCfg), C.c_void_p, C.c_void_p, C.POINTER(LoopResult)]),
    "pgh_poly_run_batch_mixed": (C.c_int, [c_graph, c_mat, C.c_void_p, C.c_int32, c_mat, C.POINTER(LoopCfg), C.c_void_p,
                                           C.POINTER(LoopResult)]),
}

# include/pgh_lfpr.h.  Unfused route: LFPR takes the reference's route, one backend primitive at a time.
LFPR_SIGNATURES = {
    "pgh_lfpr_setup": (C.c_int, [c_vec, c_vec, c_vec, c_vec, C.c_double, c_vec, c_vec, c_vec, c_vec, c_vec, c_f64p]),
    "pgh_lfpr_close": (C.c_int, [c_vec, c_vec, C.c_double, c_vec, c_vec, c_vec, c_vec, c_vec, C.c_double, C.c_double, C.c_double,
                                 C.c_int32, c_vec, c_vec, c_f64p]),
}

# include/pgh_oversample.h.  Unfused route: SeedOversampling and BoostedSeedOversampling take the backend-primitive route.
OVERSAMPLE_SIGNATURES = {
    "pgh_seed_floor": (C.c_int, [c_mat, c_mat, c_f64p, c_i64p]),
    "pgh_seed_resample": (C.c_int, [c_mat, c_f64p, C.c_int32, c_mat, c_mat, c_i64p]),
    "pgh_boost_forms": (C.c_int, [c_mat, c_mat, c_mat, c_f64p]),
    "pgh_boost_update": (C.c_int, [c_mat, c_mat, c_f64p, c_mat, c_f64p, c_i64p]),
}
OVERSAMPLE_MAX_COLS = 64  # include/pgh_oversample.h PGH_OVERSAMPLE_MAX_COLS

# include/pgh_rank.h.  Unfused route: NDCG and SpearmanCorrelation take the columns route.
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
RANK_MAX_RELEVANT = 8192  # include/pgh_rank.h PGH_RANK_MAX_RELEVANT
RANK_LDS_BYTES = 61440    # include/pgh_rank.h PGH_RANK_LDS_BYTES
RANK_AUTO, RANK_STREAMING, RANK_SORTED = 0, 1, 2                                    # include/pgh_rank.h PGH_RANK_*

# include/pgh_krylov.h.  Unfused route: the Krylov-space filters take the reference's route, one backend primitive at a time.
KRYLOV_SIGNATURES = {
    "pgh_lanczos_close": (C.c_int, [c_vec, c_vec, C.c_double, c_vec, C.c_double, c_vec, c_mat, C.c_int32, c_f64p]),
    "pgh_krylov_residuals": (C.c_int, [c_mat, c_f64p, C.c_int32, C.c_int32, c_f64p, c_f64p]),
}
KRYLOV_MAX_DIMS = 64      # include/pgh_krylov.h PGH_KRYLOV_MAX_DIMS
KRYLOV_MAX_PROBES = 64    # include/pgh_krylov.h PGH_KRYLOV_MAX_PROBES

# include/pgh_link.h.  Unfused route: LinkAssessment and ClusteringCoefficient score the downloaded slab with numpy.
c_link_plan = C.c_void_p
LINK_SIGNATURES = {
    "pgh_link_plan_create": (C.c_int, [C.c_int64, C.c_int64, c_i32p, c_i32p, C.POINTER(C.c_uint8), C.POINTER(c_link_plan)]),
    "pgh_link_plan_info": (C.c_int, [c_link_plan, c_i64p, c_i64p, c_i64p]),
    "pgh_link_plan_destroy": (C.c_int, [c_link_plan]),
    "pgh_link_auc": (C.c_int, [c_mat, c_link_plan, C.c_int32, c_f64p, c_i64p, c_i64p]),
    "pgh_link_predictions": (C.c_int, [c_mat, c_link_plan, C.c_int32, C.c_int64, C.c_int64, c_f64p]),
    "pgh_link_factors": (C.c_int, [c_mat, C.c_int32, c_vec]),
}
LINK_MAX_PAIRS = 1 << 27  # include/pgh_link.h PGH_LINK_MAX_PAIRS
LINK_COS, LINK_DOT = 0, 1                                                           # include/pgh_link.h PGH_LINK_*

# include/pgh_arnoldi.h.  Unfused route: arnoldi_iteration takes the reference's route, one backend primitive at a time.
ARNOLDI_SIGNATURES = {
    "pgh_basis_dots": (C.c_int, [c_mat, C.c_int32, c_vec, c_f64p]),
    "pgh_arnoldi_close": (C.c_int, [c_mat, C.c_int32, c_vec, c_f64p, c_vec, C.c_int32, c_f64p]),
}
ARNOLDI_MAX_DIMS = 64     # include/pgh_arnoldi.h PGH_ARNOLDI_MAX_DIMS

# include/pgh_post.h.  Unfused route: a postprocessor's propagate transforms the columns of the inner ranker's batch one by one.
POST_SIGNATURES = {
    "pgh_post_kth_largest": (C.c_int, [c_mat, C.c_int64, c_f64p]),
    "pgh_post_col_threshold": (C.c_int, [c_mat, c_f64p, C.c_int32, c_mat]),
    "pgh_post_col_affine": (C.c_int, [c_mat, c_f64p, c_f64p, c_mat]),
    "pgh_post_row_op": (C.c_int, [c_mat, c_vec, C.c_int32, C.c_double, c_mat]),
    "pgh_post_ordinals": (C.c_int, [c_mat, c_mat]),
}
POST_MAX_COLS = 64        # include/pgh_post.h PGH_POST_MAX_COLS
POST_ROW_SUB, POST_ROW_SWEEP = 0, 1                                                 # include/pgh_post.h PGH_POST_ROW_*

# include/pgh_gnn.h.  Unfused route: gnn.differentiable_propagate steps its recurrences one conv at a time (needs pgh_graph_transposed
# under graph_dropout), stages its slabs through the host, and builds the transposed operator from a scipy round trip.
GNN_SIGNATURES = {
    "pgh_graph_transposed": (C.c_int, [c_graph, C.POINTER(c_graph)]),
    "pgh_linear_run_batch": (C.c_int, [c_graph, c_mat, C.c_double, C.c_int32, c_f64p, c_f64p, c_f64p, c_mat, C.c_double, C.c_uint64,
                                       C.c_int64, c_f64p]),
    "pgh_mat_wrap": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(c_mat)]),
}

# include/pgh_select.h.  Unfused route: top / nonzero / Subgraph / Supergraph work with numpy on the downloaded values, MabsMaintain and
# SeparateNormalization transform the columns of the inner ranker's batch one by one.
SELECT_SIGNATURES = {
    "pgh_vec_select": (C.c_int, [c_vec, C.c_int32, C.c_double, C.c_int64, c_i32p, c_vec, c_i64p]),
    "pgh_vec_gather": (C.c_int, [c_vec, c_i32p, C.c_int64, c_vec]),
    "pgh_vec_scatter": (C.c_int, [c_vec, c_i32p, C.c_int64, c_vec]),
    "pgh_mat_topk": (C.c_int, [c_mat, C.c_int64, c_i32p, c_f64p]),
    "pgh_mat_col_scale": (C.c_int, [c_mat, c_f64p, c_mat]),
    "pgh_mat_split_sums": (C.c_int, [c_mat, c_vec, c_f64p]),
    "pgh_mat_split_blend": (C.c_int, [c_mat, c_vec, c_f64p, c_f64p, c_mat]),
}
SELECT_NONZERO, SELECT_GT, SELECT_GE = 0, 1, 2                                     # include/pgh_select.h PGH_SELECT_*
TOPK_MAX_K = 4096         # include/pgh_select.h PGH_TOPK_MAX_K
SELECT_MAX_COLS = 64      # include/pgh_select.h PGH_SELECT_MAX_COLS

# include/pgh_retire.h.  Unfused route: propagate (and AlgorithmSelection's mixed PageRank group) takes the plain multi-seed entry.
RETIRE_MAX_STAGES = 8     # include/pgh_retire.h PGH_RETIRE_MAX_STAGES
RETIRE_NARROWED = 32      # include/pgh_retire.h PGH_RETIRE_NARROWED (a bit of pgh_loop_result::flags)


class RetireReport(C.Structure):
    _fields_ = [("num_stages", C.c_int32), ("reserved", C.c_int32), ("ld", C.c_int32 * RETIRE_MAX_STAGES),
                ("live", C.c_int32 * RETIRE_MAX_STAGES), ("first_step", C.c_int32 * RETIRE_MAX_STAGES), ("column_steps", C.c_int64)]


_RETIRE_TAIL = [c_i32p, C.c_int32, C.POINTER(RetireReport)]      # levels, num_levels, report: behind the plain sibling's arguments
RETIRE_SIGNATURES = {
    "pgh_ppr_run_batch_retire": (C.c_int, [c_graph, c_mat, c_mat, C.POINTER(LoopCfg), C.c_void_p, C.POINTER(LoopResult)] + _RETIRE_TAIL),
    "pgh_ppr_run_batch_mixed_retire": (C.c_int, [c_graph, c_mat, c_mat, C.POINTER(LoopCfg), C.c_void_p, C.c_void_p, C.POINTER(LoopResult)]
                                       + _RETIRE_TAIL),
    "pgh_absorb_run_batch_retire": (C.c_int, [c_graph, c_mat, c_vec, c_mat, C.POINTER(LoopCfg), C.c_void_p, C.POINTER(LoopResult)]
                                    + _RETIRE_TAIL),
    "pgh_sarw_run_batch_retire": (C.c_int, [c_graph, c_mat, c_mat, C.POINTER(LoopCfg), C.c_void_p, C.POINTER(LoopResult)] + _RETIRE_TAIL),
}


def retire_on(retire):
    """Whether a ranker's ``retire`` asks for the retiring loops: True or a list of levels (an empty one included: a run that never
    narrows); False and None do not."""
    return retire is True or isinstance(retire, (list, tuple))


def retire_levels(retire):
    """(levels, num_levels) of an include/pgh_retire.h call for a ranker's ``retire``: True -> the engine's default levels, a list ->
    those live-column counts (the engine checks them)."""
    if retire is True:
        return None, -1
    levels = [int(level) for level in retire]
    return (C.c_int32 * max(len(levels), 1))(*levels), len(levels)


def retire_stages(report):
    """An engine report as the dict ``last_batches`` and ``mixed_calls`` carry under "stages"."""
    count = report.num_stages
    return dict(ld=list(report.ld[:count]), live=list(report.live[:count]), first_step=list(report.first_step[:count]),
                column_steps=int(report.column_steps))


# include/pgh_batch64.h.  Unfused route: a filter whose run wants f64 iterates propagates column by column (the single-vector f64 loops).
_BATCH64_TAIL = [C.c_void_p, C.POINTER(LoopResult)]              # out_scales, results
BATCH64_SIGNATURES = {
    "pgh_spmm_f64": (C.c_int, [c_graph, C.c_void_p, C.c_int32, C.c_void_p]),
    "pgh_ppr_run_batch_f64": (C.c_int, [c_graph, c_mat, c_mat, C.POINTER(LoopCfg)] + _BATCH64_TAIL + [C.c_void_p]),
    "pgh_absorb_run_batch_f64": (C.c_int, [c_graph, c_mat, c_vec, c_mat, C.POINTER(LoopCfg)] + _BATCH64_TAIL + [C.c_void_p]),
    "pgh_sarw_run_batch_f64": (C.c_int, [c_graph, c_mat, c_mat, C.POINTER(LoopCfg)] + _BATCH64_TAIL + [C.c_void_p]),
    "pgh_poly_run_batch_f64": (C.c_int, [c_graph, c_mat, C.c_void_p, C.c_int32, c_mat, C.POINTER(LoopCfg)] + _BATCH64_TAIL),
}


# header -> its table: every optional entry family; the names are distinct across the tables and from SIGNATURES
OPTIONAL = {
    "pgh_batch.h": BATCH_SIGNATURES, "pgh_tune.h": TUNE_SIGNATURES, "pgh_measure.h": MEASURE_SIGNATURES,
    "pgh_supervised.h": SUPERVISED_SIGNATURES, "pgh_fair.h": FAIR_SIGNATURES, "pgh_mixed.h": MIXED_SIGNATURES,
    "pgh_lfpr.h": LFPR_SIGNATURES, "pgh_oversample.h": OVERSAMPLE_SIGNATURES, "pgh_rank.h": RANK_SIGNATURES,
    "pgh_krylov.h": KRYLOV_SIGNATURES, "pgh_link.h": LINK_SIGNATURES, "pgh_arnoldi.h": ARNOLDI_SIGNATURES,
    "pgh_post.h": POST_SIGNATURES,
}
# ... and every header entry() serves: OPTIONAL -- the thirteen families whose number and 41 names tests/test_fused_plumbing.py pins --
# and the headers added since, which tests of their own enumerate (include/pgh_gnn.h: tests/test_gnn_host.py; include/pgh_select.h:
# tests/test_subgraph_host.py; include/pgh_retire.h: tests/test_retire_host.py; include/pgh_batch64.h: tests/test_batch64_host.py)
TABLES = dict(OPTIONAL, **{"pgh_gnn.h": GNN_SIGNATURES, "pgh_select.h": SELECT_SIGNATURES, "pgh_retire.h": RETIRE_SIGNATURES,
                           "pgh_batch64.h": BATCH64_SIGNATURES})
_HEADER_OF = {name: header for header, table in TABLES.items() for name in table}
DECLINED = 2              # every optional header's PGH_*_DECLINED: nothing was written, the caller takes its unfused route

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


def bind_optional(cdll, table):
    """Binds the entries of the optional `table` that `cdll` exports; returns {name: function or None when the library lacks it}."""
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


def entry(name):
    """The bound optional entry `name` of the loaded library, or None when that library does not export it; KeyError for a name no
    optional header declares.  A header's table is bound on its first lookup and kept on the library object, as the attribute
    ``_pgh_<family>_entries`` for include/pgh_<family>.h: another library (the tests' host double) has its own, and a test puts
    stand-ins for one family's entries there."""
    header = _HEADER_OF[name]
    attribute = "_%s_entries" % header[:-2]
    cdll = lib()
    cache = getattr(cdll, attribute, None)
    if cache is None:
        cache = bind_optional(cdll, TABLES[header])
        setattr(cdll, attribute, cache)
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


def accepted(status):
    """False when an optional entry DECLINED (the caller takes its unfused route); otherwise check(status) and True."""
    if status == DECLINED:
        return False
    check(status)
    return True


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
