/*
 * pgh_link.h -- what the multi-group measures (the reference's pygrank/measures/multigroup.py: LinkAssessment, i.e. LinkAUC / HopAUC,
 * and ClusteringCoefficient) need from the engine beyond include/pgh.h: the similarity of a fixed list of node pairs under the [n, b]
 * slab of a batch (one column per group), and the AUC of those similarities against the pairs' labels.
 *
 * THE SIMILARITY, with the reference's quirk kept.  _dot_similarity and _cos_similarity (multigroup.py:8-27) ASSIGN `dot = ui * vi`
 * inside their loop over the groups, they do not accumulate: the numerator of a pair (v, u) is the product of the LAST column's two
 * scores alone.  The cos denominator is sqrt(l2[u] * l2[v]) with l2[i] the sum of the squares of row i over ALL columns, added in
 * column order; a zero denominator gives 0 (safe_div).  Everything is formed in f64 from the stored f32 scores exactly as Python forms
 * it from doubles: the product of two f32 values and the square of one are exact in f64, the row sum is SEQUENTIAL in column order
 * (one lane adds its row), the division and the square root are IEEE.  A prediction therefore equals numpy's to the bit.
 *
 * Counts are 64-bit integers (integer atomics only), there are no floating-point atomics, no result depends on the grid or on the
 * order in which workgroups arrive, and two calls on the same input return the same bits.
 *
 * A request an entry cannot serve (its scratch does not fit in device memory) returns PGH_LINK_DECLINED with nothing written
 * (pgh_last_error says why): the caller then scores the downloaded slab on the host.  Any other non-zero status is an error; nothing
 * is written then either.
 */
#ifndef PGH_LINK_H
#define PGH_LINK_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_LINK_DECLINED 2
/* more pairs than this (2^27) is an error: the ids, the 64-bit keys with their labels and the sort's space come to about 3.5 GB there */
#define PGH_LINK_MAX_PAIRS 134217728
/* `similarity` */
#define PGH_LINK_COS 0
#define PGH_LINK_DOT 1

typedef struct pgh_link_plan_s* pgh_link_plan_t;

/* The pairs of every call, uploaded once: pair k is (first_host[k], second_host[k]), node ids in [0, n), with label_host[k] != 0 for a
 * positive pair.  Duplicates stay and count.  The count is checked before a single element is read.  The plan owns the scratch of its
 * calls -- an [n] f64 buffer, [num_pairs] 64-bit keys with their label payload in and out of the sort, a prefix count and the sort's
 * temporary -- allocated by the first call that needs it and kept: repeated calls allocate nothing.
 * Errors: null arguments, n < 1 or n >= 2^31 - 1, num_pairs < 0 or > PGH_LINK_MAX_PAIRS, an id outside [0, n). */
int pgh_link_plan_create(int64_t n, int64_t num_pairs, const int32_t* first_host, const int32_t* second_host, const uint8_t* label_host,
                         pgh_link_plan_t* out);
int pgh_link_plan_info(pgh_link_plan_t plan, int64_t* n, int64_t* num_pairs, int64_t* num_positive);
int pgh_link_plan_destroy(pgh_link_plan_t plan);

/* The AUC (ties at mid-rank) of the pairs' similarities against their labels under `scores` ([n, b], n = the plan's, ANY b >= 1: the
 * row pass loops over the columns).  Four stages on the engine's stream:
 *   row pass   l2[i] = sum_j (double)S[i, j]^2, j ascending (PGH_LINK_DOT skips it)
 *   pair pass  pred = ((double)S[v, b-1] * (double)S[u, b-1]) / sqrt(l2[u] * l2[v]), 0 where the denominator is 0 (PGH_LINK_DOT: the
 *              numerator alone), written as an order-preserving 64-bit key; -0.0 and +0.0 are one key
 *   sort       one radix sort of (key, label)
 *   counting   two_wins = sum over the tie groups of positives_in_group * (2 * negatives_below + negatives_in_group), 64-bit integers
 * and *auc = (double)two_wins / (2.0 * P * N): every operand is below 2^53, one rounding.  *num_positive = P and *num_negative = N are
 * always written on success; with P == 0 or N == 0 no stage runs and *auc is NaN.  A NaN prediction (non-finite scores) gives NaN.
 * Errors: null arguments, a slab whose row count is not the plan's, an unknown similarity.  Synchronises. */
int pgh_link_auc(pgh_mat_t scores, pgh_link_plan_t plan, int32_t similarity, double* auc, int64_t* num_positive, int64_t* num_negative);

/* out_host[k] = the f64 prediction of pair first + k, k < count (0 <= first, first + count <= num_pairs): what measures other than AUC
 * are given.  Errors as pgh_link_auc, and a range outside the plan.  Synchronises. */
int pgh_link_predictions(pgh_mat_t scores, pgh_link_plan_t plan, int32_t similarity, int64_t first, int64_t count, double* out_host);

/* out[i] = t_i, the factor of row i in a pair's similarity (the similarity of (v, u) is t_v * t_u up to rounding):
 *   PGH_LINK_DOT  S[i, b-1]        PGH_LINK_COS  (double)S[i, b-1] / sqrt(l2[i]), 0 where l2[i] is 0
 * formed in f64 and rounded once to f32.  out has n elements.  Errors: null arguments, a length mismatch, an unknown similarity. */
int pgh_link_factors(pgh_mat_t scores, int32_t similarity, pgh_vec_t out);

#ifdef __cplusplus
}
#endif

#endif /* PGH_LINK_H */
