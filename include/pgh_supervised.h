/*
 * pgh_supervised.h -- what the supervised measures need from the engine beyond include/pgh.h: every sum over (score, known) pairs
 * that a closed-form measure is made of, for up to 64 score columns in ONE streaming pass over the slab.
 *
 * The reference's supervised measures (pygrank/measures/supervised.py:93-333) score one vector against the known scores with two to
 * six elementwise passes and reductions.  All of them but the sort-based ones (AUC, NDCG, Spearman, Mann-Whitney) are closed-form
 * functions of a handful of sums: of s, s^2, k, k^2, k s, |k - s|, (k - s)^2, of three maxima, and for the entropies of five sums of
 * logarithms.  For the b columns of a propagate() result a per-column evaluation tears the slab apart (one strided pass per column)
 * and then pays those passes per column.  Here one kernel reads every row of the slab once and accumulates every such sum for every
 * column.
 *
 * Sums are taken in f64 from the stored f32 values: by a lane over its rows, by a wavefront with shuffles, by a workgroup through LDS.
 * Every one of a FIXED number of row parts writes its partial sums to a buffer and a second kernel folds the parts in a fixed order.
 * There are no floating-point atomics, and the parts do not depend on the launch: a result depends on neither the grid shape nor
 * the order in which workgroups arrive, and two calls on the same input return the same bits.
 *
 * A request pgh_pair_forms does not serve returns PGH_PAIR_DECLINED with nothing written (the error text says why): the caller then
 * takes the reference's route one column at a time.  Any other non-zero status is an error.
 */
#ifndef PGH_SUPERVISED_H
#define PGH_SUPERVISED_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_PAIR_DECLINED 2
/* doubles written per column */
#define PGH_PAIR_SLOTS 20
/* `groups` of pgh_pair_forms: MOMENTS computes the slots 0..11 (the slots 12..19 are written as 0), LOGS all 20 */
#define PGH_PAIR_MOMENTS 0
#define PGH_PAIR_LOGS 1

/* Per column j of `scores` ([n, b], 1 <= b <= 64), over the KEPT rows i: those whose exclude value equals 0 (the rule of
 * pgh_filter_out; without an exclude argument every row is kept), with
 *   s = (double)scores[i, j] * factors[j]        (factors == NULL: all ones)
 *   k = (double)known[i]  or  (double)known[i, j]
 * formed and accumulated in f64, plain IEEE arithmetic without special cases (0 * log(0) is NaN):
 *   out[20 j +  0] = number of kept rows     out[20 j +  6] = sum |k - s|
 *   out[20 j +  1] = sum s                   out[20 j +  7] = sum (k - s)^2
 *   out[20 j +  2] = sum s^2                 out[20 j +  8] = max |k - s|
 *   out[20 j +  3] = sum k                   out[20 j +  9] = max s
 *   out[20 j +  4] = sum k^2                 out[20 j + 10] = max k
 *   out[20 j +  5] = sum k s                 out[20 j + 11] = sum |k|
 * and for groups == PGH_PAIR_LOGS (PGH_PAIR_MOMENTS writes 0 into these slots and evaluates no logarithm)
 *   out[20 j + 12] = sum k log(s + eps)
 *   out[20 j + 13] = sum (1 - k) log(1 - s + eps)
 *   out[20 j + 14] = sum (s + eps) log(s + eps)
 *   out[20 j + 15] = sum (s + eps) log(k + eps)
 *   out[20 j + 16] = sum s log(k)
 *   out[20 j + 17 .. 19] = 0 (reserved)
 * A column without a kept row gives 0 for the sums and -inf for the maxima.
 * Exactly one of known_vec ([n]) and known_mat ([n, b]) is given, at most one of exclude_vec and exclude_mat.
 * Declined: b > 64, a non-finite factor or eps.  Shape mismatches, both or neither of the known arguments, both exclude arguments,
 * a null out_host and an unknown `groups` are errors. */
int pgh_pair_forms(pgh_mat_t scores, pgh_vec_t known_vec, pgh_mat_t known_mat, pgh_vec_t exclude_vec, pgh_mat_t exclude_mat,
                   const double* factors_host, double eps, int32_t groups, double* out_host /* [PGH_PAIR_SLOTS * b] */);

#ifdef __cplusplus
}
#endif

#endif /* PGH_SUPERVISED_H */
