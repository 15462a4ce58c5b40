/*
 * pgh_batch64.h -- the f64 siblings of the multi-seed device loops (include/pgh.h pgh_ppr_run_batch, include/pgh_batch.h).
 *
 * A filter whose tolerance lies below fp32 eps runs its single-vector loop in f64 (pgh_ppr_run_f64, pgh_absorb_run_f64,
 * pgh_sarw_run_f64, pgh_poly_run with form 2).  The entries below run up to 64 such columns as ONE device loop over the multi-seed
 * stream of pgh_spmm: iterates, row sums, cross-tile carries, quotients and residuals are doubles, one column per lane slot; the
 * stream's f32 values and the image's f32 row and source scales are widened to double where they are used.  No image is built
 * beside the multi-seed one.  Column j does what the single-vector f64 entry does for that column and results[j] reports what
 * that entry would report.  No atomics: two calls on the same operands return the same bits.
 *
 * Common arguments
 *   p            [n, b] f32 personalizations, 1 <= b <= 64.  The recursive loops take it UN-normalised with in_norms beside it and
 *                form p / |p| in f64 (as pgh_loop_cfg::in_norm does for the single-vector entries); pgh_poly_run_batch_f64 takes it
 *                as its f32 sibling does.
 *   in_norms     [b] host: the L1 norm of every column.  in_norms[j] == 0 marks a zero column: it stays zero, takes no part in
 *                the loop and reports 0 iterations.
 *   out          [n, b] f32, output only: the f64 iterate times quotient x output scale in f64, rounded once
 *   cfg          the pgh_loop_cfg of include/pgh.h; tol is used as given (the caller clamps it at fp64 eps); the loop always starts
 *                from p (start_from_p is implied); in_norm is not used
 *   out_scales   nullable: per-column preserve_norm factor (cfg->out_scale for every column when null; a negative cfg->out_scale
 *                means the column's in_norm, as in the single-vector entries)
 *   results      [b] per-column pgh_loop_result
 *
 * The stopping check comes before every step (convergence.py:86); the residual of a step is |y_new s_new - y_old s_old| of the
 * un-normalised iterates and their quotients, summed (L1; Mabs divides by n) or maxed in f64.  A stopped column no longer changes.
 *
 * Square graphs that carry the blocked layout and hold at least one entry only: anything else returns PGH_BATCH64_DECLINED with
 * nothing written (pgh_last_error says why) and the caller runs the columns one by one.  A width outside [1, 64], a null argument,
 * a shape mismatch and a non-finite alpha or coefficient are errors.
 */
#ifndef PGH_BATCH64_H
#define PGH_BATCH64_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_BATCH64_DECLINED 2

/* Y = M^T X for row-major [n, b] HOST doubles in the caller's ids, 1 <= b <= 64: upload, way in, one product pass, way out,
 * download.  The primitive the loops are built on (and a conv for f64 feature matrices). */
int pgh_spmm_f64(pgh_graph_t g, const double* x_host, int32_t b, double* y_host);

/* PageRank (adhoc.py:34-36): y = alpha s_j (M^T y_old) + (1 - alpha) p / |p|, s_j the column's quotient (cfg->use_quotient). */
int pgh_ppr_run_batch_f64(pgh_graph_t g, pgh_mat_t p, pgh_mat_t out, const pgh_loop_cfg* cfg, const double* out_scales,
                          pgh_loop_result* results, const double* in_norms /* [b] */);

/* AbsorbingWalks (adhoc.py:157-169) with ONE absorption vector lam [n] (already times (1 - alpha) / alpha): the row weights
 * deg / (lam + deg) and lam / (lam + deg) are formed in f64 from the f32 degrees and lam.  A node with lam + deg == 0 is declined. */
int pgh_absorb_run_batch_f64(pgh_graph_t g, pgh_mat_t p, pgh_vec_t lam, pgh_mat_t out, const pgh_loop_cfg* cfg,
                             const double* out_scales, pgh_loop_result* results, const double* in_norms /* [b] */);

/* SymmetricAbsorbingRandomWalks (adhoc.py:348-364): the walk above with lam = (1 + sqrt(1 + 4 deg)) / 2 per node and the source
 * factor 1 / lam folded into the gather slab. */
int pgh_sarw_run_batch_f64(pgh_graph_t g, pgh_mat_t p, pgh_mat_t out, const pgh_loop_cfg* cfg, const double* out_scales,
                           pgh_loop_result* results, const double* in_norms /* [b] */);

/* The taylor form of ClosedFormGraphFilter for b columns with f64 terms and accumulator (pgh_poly_run with form 2): arguments and
 * iteration counts as pgh_poly_run_batch. */
int pgh_poly_run_batch_f64(pgh_graph_t g, pgh_mat_t p, const double* coeffs, int32_t num_coeffs, pgh_mat_t out,
                           const pgh_loop_cfg* cfg, const double* out_scales, pgh_loop_result* results);

#ifdef __cplusplus
}
#endif

#endif /* PGH_BATCH64_H */
