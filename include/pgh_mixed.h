/*
 * pgh_mixed.h -- multi-seed device loops whose COLUMNS ARE DIFFERENT FILTERS: what AlgorithmSelection needs from the engine beyond
 * include/pgh.h and include/pgh_batch.h.
 *
 * The reference's AlgorithmSelection (pygrank/algorithms/autotune/selection.py) runs every candidate filter on every training split, one
 * rank() after the other on the same matrix: PageRank at several alpha, HeatKernel at several t, ...  pgh_ppr_run_batch and
 * pgh_poly_run_batch share one adjacency pass between their columns but take ONE alpha / ONE coefficient schedule for the whole batch.
 * The entries below are those two loops with the parameter per column: the same kernels (a further template parameter of k_mm_step,
 * k_mm_close2, k_mm_poly_init and k_mm_poly_step: the per-column values travel as kernel arguments, nothing is read per row for them),
 * the same gather pass, the same per-column quotient, residual (PageRank: the in-kernel residual against the predicted quotient, formed
 * with the lane's own alpha), stopping iteration and freezing.
 *
 * Common arguments: as include/pgh_batch.h (p [n, b] already L1-normalised, 1 <= b <= 64, out_scales nullable, results [b]).
 *
 * Square graphs that carry the blocked layout only, f32 loops only.  An input these loops do not serve returns PGH_MIXED_DECLINED with
 * nothing written (pgh_last_error says why): the caller then runs the columns one by one.  b outside [1, 64], a null argument, a shape
 * mismatch or a non-finite parameter is an error.
 *
 * Not served here (the caller runs such rankers one by one): AbsorbingWalks with a per-column alpha (its row words are per row: a
 * per-column absorption needs a different step), the "chebyshev" recurrence, the f64 routes, graph_dropout.
 */
#ifndef PGH_MIXED_H
#define PGH_MIXED_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_MIXED_DECLINED 2

/* pgh_ppr_run_batch with column j running PageRank(alphas[j]); cfg->alpha is ignored.  The factors (float)(alphas[j] * quotient_j) and
 * (float)(1 - alphas[j]) are formed per column as the uniform loop forms them; results[j] is what pgh_ppr_run would report for column j
 * at alphas[j].  cfg->start_from_p == 0 starts column j from ranks[:, j] (a warm start). */
int pgh_ppr_run_batch_mixed(pgh_graph_t g, pgh_mat_t p, pgh_mat_t ranks, const pgh_loop_cfg* cfg, const double* alphas /* [b], host */,
                            const double* out_scales, pgh_loop_result* results);

/* The taylor form of pgh_poly_run_batch with a coefficient schedule per column: column j uses coeffs[(it - 1) * b + j] at iteration it
 * (0 beyond num_coeffs; a shorter schedule is zero-padded by the caller).  A zero coefficient changes nothing and counts as a change of
 * 0 for that column, as in the uniform entry. */
int pgh_poly_run_batch_mixed(pgh_graph_t g, pgh_mat_t p, const double* coeffs /* [num_coeffs][b], host, row k = iteration k + 1 */,
                             int32_t num_coeffs, pgh_mat_t out, const pgh_loop_cfg* cfg, const double* out_scales,
                             pgh_loop_result* results);

#ifdef __cplusplus
}
#endif

#endif /* PGH_MIXED_H */
