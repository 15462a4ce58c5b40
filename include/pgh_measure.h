/*
 * pgh_measure.h -- what the unsupervised measures need from the engine beyond include/pgh.h: the cut forms of up to 64 score
 * columns in ONE pass over the adjacency per slab, and the per-column statistics their decisions are taken from.
 *
 * The reference's Conductance and Density (pygrank/measures/unsupervised.py:52-145) score one column with two convolutions (of the
 * scores s and of their complement max_rank - s) and four dot products.  For the b columns of a propagate() result that is 2 b
 * passes over the adjacency.  Here a pack kernel writes a slab X = [s | c] of up to 64 columns, the multi-seed pass of include/pgh.h
 * (pgh_spmm) gives Y = M^T X, and one streaming kernel reads every row of X and Y once and accumulates the four forms of every
 * column: 64 score columns cost two passes over the adjacency.
 *
 * Sums are taken in f64: by a lane over its rows, by a wavefront with shuffles, by a workgroup through LDS.  Every one of a FIXED
 * number of row parts writes its partial sums to a buffer and a second kernel adds the parts in index order.  There are no
 * floating-point atomics, and the parts do not depend on the launch: a result depends on neither the grid shape nor the order in
 * which workgroups arrive, and two calls on the same input return the same bits.
 *
 * A request pgh_cut_forms does not serve returns PGH_MEASURE_DECLINED with nothing written (the error text says why): the caller
 * then takes the reference's route one column at a time.  Any other non-zero status is an error.
 */
#ifndef PGH_MEASURE_H
#define PGH_MEASURE_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_MEASURE_DECLINED 2
/* `forms` of pgh_cut_forms */
#define PGH_CUT_ALL 0
#define PGH_CUT_INTERNAL 1

/* per column j of m: out[4j..4j+3] = sum, sum of squares, max, min (f64 accumulation; one pass over the slab).  Max and min are the
 * stored f32 values, exactly.  A slab without rows gives 0, 0, -inf, +inf. */
int pgh_mat_col_stats(pgh_mat_t m, double* out_host /* [4 * b] */);

/* Per column j of `scores` ([n, b], 1 <= b <= 64), on a square graph g (the stored CSR(M^T), any image):
 *   s = scores[:, j] * (float)factors[j]     (one f32 product, the value pgh_ewise_vs stores for PGH_MUL; factors == NULL: all ones)
 *   c = (float)max_rank - s                  (one f32 difference, the value pgh_ewise_vs stores for PGH_SUB, scalar on the left)
 *   N = M^T s,  C = M^T c                    (what pgh_spmm stores for those columns)
 *   out[4j..4j+3] = <N, s>, <N, c>, <C, s>, <C, c>     (products and sums in f64)
 * forms == PGH_CUT_INTERNAL: only <N, s> is computed (Density); the other three slots are written as 0.
 * Declined: b > 64, a non-finite factor or max_rank, a graph without the multi-seed layout (rectangular matrices, slices of a row
 * partition, graphs kept in the row-major image only).  Shape mismatches, null arguments and an unknown `forms` are errors. */
int pgh_cut_forms(pgh_graph_t g, pgh_mat_t scores, const double* factors_host, double max_rank, int32_t forms,
                  double* out_host /* [4 * b] */);

#ifdef __cplusplus
}
#endif

#endif /* PGH_MEASURE_H */
