/*
 * pgh_cheb64.h -- the "chebyshev" form of the closed-form filters as an f64 multi-seed loop: the sibling of the taylor loop
 * pgh_poly_run_batch_f64 of include/pgh_batch64.h, over the same stream and the same [n, ld] slabs of doubles.
 *
 * The reference's recurrence (abstract_filters.py:215-224; pgh_poly_run with form 1 for a single vector):
 *     T_1 = p,   T_2 = M^T T_1,   T_k = 2 M^T T_{k-1} - T_{k-1} from iteration 3 on,   result_k = result_{k-1} + c_k T_k
 * under the taylor loop's stopping rule on |result_k - result_{k-1}|.  From iteration 3 on a zero c_k adds nothing (the change of that
 * iteration is then 0); at iterations 1 and 2 the term is added whatever c_k is.  The recurrence amplifies rounding noise, so the form
 * runs in f64 at every tolerance; cfg->tol is used as given.
 *
 * Arguments, refusals, PGH_BATCH64_DECLINED and the report per column (iterations = 2 + the column's steps; max_iters <= 1: zeros and
 * 1 iteration) are those of the taylor sibling.  A column that has stopped no longer changes; no atomics: two calls on the same operands
 * return the same bits.
 */
#ifndef PGH_CHEB64_H
#define PGH_CHEB64_H

#include "pgh_batch64.h"

#ifdef __cplusplus
extern "C" {
#endif

int pgh_cheb_run_batch_f64(pgh_graph_t g, pgh_mat_t p, const double* coeffs, int32_t num_coeffs, pgh_mat_t out,
                           const pgh_loop_cfg* cfg, const double* out_scales, pgh_loop_result* results);

#ifdef __cplusplus
}
#endif

#endif /* PGH_CHEB64_H */
