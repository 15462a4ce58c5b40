/*
 * pgh_batch.h -- multi-seed device loops of the filters other than PageRank (include/pgh.h has pgh_ppr_run_batch).
 *
 * NodeRanking.propagate (signals.py:225-226) runs one rank() per feature column.  These entry points run up to 64 such columns
 * as ONE device loop over the multi-seed layout of pgh_spmm: the adjacency is streamed once per iteration for the whole batch.
 * Column j behaves like the single-vector fused run of that column (pgh_poly_run / pgh_absorb_run / pgh_sarw_run): it keeps its
 * own quotient, residual and stopping iteration and is frozen once it stops; results[j] is what the single-vector run would
 * report for it.  The loops are f32 loops (the f64 routes and graph_dropout are not batched).
 *
 * Common arguments
 *   p            [n, b] personalizations, one per column, already L1-normalised (zero columns stay zero), 1 <= b <= 64
 *   out          [n, b] output only
 *   cfg          the pgh_loop_cfg of include/pgh.h; the loop always starts from p (start_from_p is implied), in_norm is not used
 *   out_scales   nullable: per-column preserve_norm factor (cfg->out_scale for every column when null)
 *   results      [b] per-column pgh_loop_result
 *
 * Square graphs that carry the blocked layout only.  An input these loops do not serve returns PGH_BATCH_DECLINED with nothing
 * written (pgh_last_error says why): the caller then runs the columns one by one.  Any other non-zero status is an error.
 */
#ifndef PGH_BATCH_H
#define PGH_BATCH_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_BATCH_DECLINED 2

/* The taylor form of ClosedFormGraphFilter (abstract_filters.py:196-256; HeatKernel, GenericGraphFilter, PageRankClosed) for b
 * columns, as the f32 route of pgh_poly_run: iteration it uses coeffs[it - 1] (0 beyond num_coeffs); result_1 = c_1 p and the check
 * of iteration 2 on |result_1|; step k adds c_{k+1} (M^T)^k p and the check of iteration k + 2 compares result_{k+1} with result_k
 * (the exact change of the f32 accumulator summed in f64: L1, Mabs with the graph's n, or the max).  A zero coefficient changes
 * nothing (a change of 0).  results[j].iterations = 2 + the column's steps (1 when max_iters <= 1: out is all zeros).  The
 * "chebyshev" recurrence is not served here. */
int pgh_poly_run_batch(pgh_graph_t g, pgh_mat_t p, const double* coeffs, int32_t num_coeffs, pgh_mat_t out,
                       const pgh_loop_cfg* cfg, const double* out_scales, pgh_loop_result* results);

/* AbsorbingWalks (adhoc.py:157-169) for b columns: y = a_j * u * (M^T x) + v * p with u = deg / (lam + deg), v = lam / (lam + deg),
 * a_j the column's L1 quotient (cfg->use_quotient), deg = the graph's degrees and lam [n] ONE absorption vector shared by every
 * column (already times (1 - alpha) / alpha).  The residual and stopping rule of pgh_ppr_run_batch's separate residual pass.
 * A node with lam + deg == 0 (the single-vector loop's 0 / 0) is declined. */
int pgh_absorb_run_batch(pgh_graph_t g, pgh_mat_t p, pgh_vec_t lam, pgh_mat_t out, const pgh_loop_cfg* cfg,
                         const double* out_scales, pgh_loop_result* results);

/* SymmetricAbsorbingRandomWalks (adhoc.py:348-364) for b columns: the walk above with lam = (1 + sqrt(1 + 4 deg)) / 2 per node and
 * the source factor 1 / lam applied to the iterate before the product (folded into the gather form). */
int pgh_sarw_run_batch(pgh_graph_t g, pgh_mat_t p, pgh_mat_t out, const pgh_loop_cfg* cfg, const double* out_scales,
                       pgh_loop_result* results);

#ifdef __cplusplus
}
#endif

#endif /* PGH_BATCH_H */
