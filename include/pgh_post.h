/*
 * pgh_post.h -- what the postprocessors of pygrank_amd/postprocess.py (the reference's Normalize, Ordinals, Top, Threshold, Sweep and
 * LinearSweep, pygrank/algorithms/postprocess/postprocess.py:106-450) need from the engine beyond include/pgh.h so that a chain such as
 * PageRank() >> Sweep() >> Normalize() >> Top(10) keeps the [n, b] slab of a multi-seed run on the device: the k-th largest value of
 * every column without a sort, and the per-column and per-row transformations as single slab passes.
 *
 * All slabs are row-major f32 [n, b] with 1 <= b <= 64; `out` has the shape of `m`.  Every stored value is the outcome of the f32
 * operations the entry's comment names, in that order: the value the single-vector primitive of include/pgh.h stores for the same
 * column.  Per-column host arguments are doubles and are rounded to f32 once, as pgh_ewise_vs rounds its scalar.
 *
 * No floating-point atomics.  The select counts in integers (LDS and global integer atomics): a count does not depend on the order
 * of its increments, so a result depends on neither the grid nor the arrival order and two calls on the same input return the same
 * bits.  The other entries write every element from its own inputs alone.
 *
 * A request an entry does not serve returns PGH_POST_DECLINED with nothing written (the error text says why): the caller then takes
 * the column route.  Any other non-zero status is an error; nothing is written then either.  `out` may not share its memory with `m`.
 */
#ifndef PGH_POST_H
#define PGH_POST_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_POST_DECLINED 2
/* most columns of one call */
#define PGH_POST_MAX_COLS 64
/* `op` of pgh_post_row_op */
#define PGH_POST_ROW_SUB 0
#define PGH_POST_ROW_SWEEP 1

/* values_host[j] = the k-th largest stored value of column j (k = 1: the maximum, k = n: the minimum): a selection, one of the stored
 * f32 values, the one pgh_vec_kth_largest returns for that column (== ; -0.0 and +0.0 tie and either may be returned).  +-inf and
 * denormals are ordinary values.  A NaN changes nothing outside its own column, whose value is then unspecified.
 * A radix select: f32 bits become order-preserving 32-bit keys and four passes stream the slab, each counting one 8-bit digit of the
 * elements that match their column's prefix so far; between the passes a small kernel picks every column's digit and the k left.
 * Declined: b > 64.  k outside [1, n], n >= 2^31 and null arguments are errors.  Synchronises. */
int pgh_post_kth_largest(pgh_mat_t m, int64_t k, double* values_host /* [b] */);

/* out[i, j] = (m[i, j] >= (float)cuts_host[j]) ? 1 : 0   (inclusive == 0:  >): the value pgh_ewise_vs stores under PGH_GE / PGH_GT for
 * column j and the scalar cuts_host[j].
 * Declined: b > 64.  Shape mismatches, out == m and null arguments are errors. */
int pgh_post_col_threshold(pgh_mat_t m, const double* cuts_host /* [b] */, int32_t inclusive, pgh_mat_t out);

/* out[i, j] = (m[i, j] - (float)sub_host[j]) / (float)div_host[j]: one f32 difference, then one f32 quotient (pgh_ewise_vs under PGH_SUB,
 * then under PGH_DIV).  A column with div_host[j] == 0 is copied unchanged, whatever sub_host[j] is.
 * Declined: b > 64.  Shape mismatches, out == m and null arguments are errors. */
int pgh_post_col_affine(pgh_mat_t m, const double* sub_host /* [b] */, const double* div_host /* [b] */, pgh_mat_t out);

/* v has n entries.
 *   PGH_POST_ROW_SUB    out[i, j] = m[i, j] - v[i]                              (pgh_ewise_vv under PGH_SUB; `offset` is not read)
 *   PGH_POST_ROW_SWEEP  out[i, j] = m[i, j] / (v[i] + (float)offset)            (the f32 sum pgh_ewise_vs stores under PGH_ADD, then the
 *                                                                               f32 quotient of pgh_ewise_vv under PGH_DIV)
 * Declined: b > 64.  Shape mismatches, an unknown op, out == m and null arguments are errors. */
int pgh_post_row_op(pgh_mat_t m, pgh_vec_t v, int32_t op, double offset, pgh_mat_t out);

/* out[:, j] = what pgh_vec_ordinals stores for column j: 1 for the largest entry, 2 for the next, ..., ties in ascending row order,
 * positions as f32.  One call; inside, the slab is transposed, the columns go through the sort of pgh_vec_ordinals one after the other
 * and the positions are transposed back (two temporaries of n * b floats).
 * Declined: b > 64.  Shape mismatches, n >= 2^31 - 1, out == m and null arguments are errors. */
int pgh_post_ordinals(pgh_mat_t m, pgh_mat_t out);

#ifdef __cplusplus
}
#endif

#endif /* PGH_POST_H */
