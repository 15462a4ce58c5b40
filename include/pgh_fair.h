/*
 * pgh_fair.h -- what the fairness-aware prior editing of [krasanakis2020prioredit] needs from the engine beyond include/pgh.h: the
 * edited personalizations of up to 64 candidate parameter vectors, written straight into one [n, probes] slab by ONE elementwise
 * kernel.
 *
 * The reference's FairPersonalizer (pygrank/algorithms/postprocess/fairness.py:78-93) builds one candidate's edited prior with about
 * ten elementwise backend calls per parameter bucket, each a pass over n and a temporary vector.  A coordinate step of its optimiser
 * scores ten candidates that share the three operand vectors (personalization, sensitive, original ranks): here the operands are read
 * once and every candidate's column is stored where the multi-seed loops of include/pgh_batch.h expect it.
 *
 * The kernel is elementwise: no reductions, no atomics.  Two calls on the same input return the same bits.
 *
 * A request the entry does not serve returns PGH_FAIR_DECLINED with nothing written (the error text says why): the caller then builds
 * the candidates one at a time from backend operations.  Any other non-zero status is an error.
 */
#ifndef PGH_FAIR_H
#define PGH_FAIR_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_FAIR_DECLINED 2
/* most candidates (columns of `out`) and most parameter buckets of one call */
#define PGH_FAIR_MAX_PROBES 64
#define PGH_FAIR_MAX_BUCKETS 4

/* Per row i and probe q, with P = params_host + q * (4 * buckets + 1), in f64 from the stored f32 operands and rounded ONCE to f32 at
 * the store (the convention of pgh_mat_gemm):
 *   p = personalization[i],  s = sensitive[i],  r = ranks[i] / rank_max,  d = r - p  (skew != 0)  or  |r - p|  (skew == 0)
 *   a_t = s (P[4t] - P[4t+1]) + P[4t+1]
 *   b_t = s (P[4t+2] - P[4t+3]) + P[4t+3]
 *   res = r  when buckets == 0,  else  sum over t < buckets of  (1 - a_t) exp(b_t d) + a_t exp(-b_t d)
 *   out[i, q] = (1 - P[4 buckets]) res + P[4 buckets] p
 * `sensitive` may hold fractions.  1 <= probes <= PGH_FAIR_MAX_PROBES, 0 <= buckets <= PGH_FAIR_MAX_BUCKETS.
 * Declined: probes > 64, buckets > 4, a non-finite parameter, rank_max zero or non-finite.  Length mismatches between the three
 * vectors and `out`, an `out` whose column count is not `probes`, probes < 1, buckets < 0 and null arguments are errors. */
int pgh_prior_edit(pgh_vec_t personalization, pgh_vec_t sensitive, pgh_vec_t ranks, double rank_max,
                   const double* params_host /* [probes][4 * buckets + 1] */, int32_t buckets, int32_t probes, int32_t skew,
                   pgh_mat_t out /* [n, probes] */);

#ifdef __cplusplus
}
#endif

#endif /* PGH_FAIR_H */
