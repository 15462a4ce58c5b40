/*
 * pgh_rank.h -- what the rank-based supervised measures need from the engine beyond include/pgh.h: the DCG of up to 64 score columns
 * against shared known scores, and Spearman's rho of up to 64 score columns, for the [n, b] slab of a batch.
 *
 * The reference's NDCG (pygrank/measures/supervised.py:68-90) sorts the n scores of one vector on the host and sums the known scores
 * of the first k positions; its SpearmanCorrelation (:274-279) hands both vectors to scipy.stats.spearmanr.  Both start from
 * to_numpy(): the nodes of the exclude list leave both vectors first.
 *
 * ORDER RULE.  A column's order is score descending, ties in ascending row order (Python's sorted(..., reverse=True) is stable).
 * -0.0 and +0.0 are the same score (they are canonicalised before any radix key is formed); +-inf are ordinary scores.  pos_v, the
 * position of a kept row v in column j, is the number of kept rows that precede v in that order.
 *
 * DCG needs no sort of n elements: only rows with a non-zero known score contribute, and a validation split has few of them.  The
 * streaming route sorts those few (score, row) pairs per column, reads every kept row of the slab once with the lanes across the
 * columns, finds with one binary search per element the first relevant entry that the element precedes, and counts it into an integer
 * bin; a prefix sum over a column's bins is every pos_v.  The sorted route is a radix sort of (key, kept position) pairs per column.
 *
 * All counts are integers (integer atomics only), every f64 sum is taken over a FIXED assignment of terms to lanes, wavefronts,
 * workgroups and parts and folded in a fixed order: a result depends on neither the grid shape nor the order in which workgroups
 * arrive, and two calls on the same input return the same bits.  There are no floating-point atomics.
 *
 * A request an entry does not serve returns PGH_RANK_DECLINED with nothing written (pgh_last_error says why): the caller then takes
 * the columns route.  Any other non-zero status is an error.
 */
#ifndef PGH_RANK_H
#define PGH_RANK_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_RANK_DECLINED 2
/* more relevant rows than this and the streaming route declines (the per-column sort of the relevant rows is one workgroup's LDS) */
#define PGH_RANK_MAX_RELEVANT 8192
/* bins + the sorted relevant entries' scores of all columns (8 bytes per entry and column) stay in LDS up to this many bytes per
 * workgroup; above it the bins are counted and the entries searched in global memory (they stay in L2) */
#define PGH_RANK_LDS_BYTES 61440
/* `route` of pgh_ndcg */
#define PGH_RANK_AUTO 0
#define PGH_RANK_STREAMING 1
#define PGH_RANK_SORTED 2

typedef struct pgh_rank_plan_s* pgh_rank_plan_t;

/* What the columns of every call share, built once per (known scores, exclude) pair; exclude is nullable, both vectors have n rows
 * (n >= 2^31 - 1 is an error).
 *   kept rows      exclude == 0 (the rule of pgh_filter_out; without exclude every row); their count is n'; they are listed in
 *                  ascending row order with their known scores (the "kept position" of a row is its index in that list)
 *   relevant rows  kept and known != 0, listed in ascending row order with their known scores
 *   has_negative   1 when a kept known score is below 0
 * and, built by the first call that needs them and kept:
 *   the kept known scores in descending order (IDCG of any k; the tie groups of the known scores)
 *   d_known[kept position] = 2 midrank - (n' + 1) of the known score among the kept known scores, an int32: with lo = kept known scores
 *                  above it and hi = kept known scores not below it, d_known = lo + hi - n' (ranks counted from the top; rho does not
 *                  change when both sides are ranked from the top).  2 midrank is an integer, f32 could not hold it at n = 2^23. */
int pgh_rank_plan_create(pgh_vec_t known, pgh_vec_t exclude, pgh_rank_plan_t* out);
int pgh_rank_plan_info(pgh_rank_plan_t plan, int64_t* num_kept, int64_t* num_relevant, int32_t* has_negative);
int pgh_rank_plan_destroy(pgh_rank_plan_t plan);

/* Per column j of `scores` ([n, b], 1 <= b <= 64, n = the plan's rows), with k >= 1:
 *   dcg_host[j]  = sum over the relevant rows v with pos_v < k of (double)known[v] / log2(pos_v + 2)      (f64, fixed order)
 *   idcg_host[0] = sum over i < min(k, n') of (double)K[i] / log2(i + 2), K = the kept known scores in descending order
 * Python divides.  k is not reduced by the exclusion: with n' < k every kept row is inside the first k positions.
 * A plan without relevant rows gives 0 for every DCG and for IDCG whatever the scores hold.  Otherwise a column that holds a NaN
 * score in a kept row returns NaN for that column and for no other: the reference's order is undefined there.
 * route  PGH_RANK_STREAMING  the streaming count; declined for more than PGH_RANK_MAX_RELEVANT relevant rows and for a plan with a
 *                            negative kept known score (the streaming sum is argued for non-negative terms only; graded
 *                            relevance is non-negative, and the sorted route, which sums positions and not rows, serves the rest)
 *        PGH_RANK_SORTED     one radix sort of (key, kept position) pairs per column (hipcub), then the known scores of the first
 *                            min(k, n') positions summed in a fixed order
 *        PGH_RANK_AUTO       streaming where it is served, else sorted
 * Both routes order alike and differ only in the order of the f64 sum.
 * Declined: b > 64, the streaming route as above.  Errors: null arguments, a shape mismatch, k < 1, an unknown route. */
int pgh_ndcg(pgh_mat_t scores, pgh_rank_plan_t plan, int64_t k, int32_t route, double* dcg_host /* [b] */, double* idcg_host /* [1] */);

/* Per column j of `scores` ([n, b], 1 <= b <= 64), over the kept rows:
 *   rho_host[j] = sum d_s d_k / sqrt(sum d_s^2 * sum d_k^2),  d_s = 2 midrank - (n' + 1) of the score within its column (as d_known)
 * the centred form: d_s and d_k are exact integers, their products and the three sums are f64 over fixed parts; sum d_k^2 comes from
 * the plan.  The division is IEEE: a constant column, constant known scores, n' < 2 give NaN (0 / 0), as scipy.stats.spearmanr does.
 * One radix sort of (key, kept position) pairs per column; a tie group is found by two binary searches in the sorted keys.
 * A column that holds a NaN score in a kept row returns NaN.
 * Declined: b > 64.  Errors: null arguments, a shape mismatch. */
int pgh_spearman(pgh_mat_t scores, pgh_rank_plan_t plan, double* rho_host /* [b] */);

/* The b = 1 case on a vector's own storage (a row-major [n, 1] slab IS the vector: no strided copy). */
int pgh_ndcg_vec(pgh_vec_t scores, pgh_rank_plan_t plan, int64_t k, int32_t route, double* dcg_host /* [1] */, double* idcg_host /* [1] */);
int pgh_spearman_vec(pgh_vec_t scores, pgh_rank_plan_t plan, double* rho_host /* [1] */);

#ifdef __cplusplus
}
#endif

#endif /* PGH_RANK_H */
