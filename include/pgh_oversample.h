/*
 * pgh_oversample.h -- what the seed oversampling postprocessors of [krasanakis2019boosted] (the reference's SeedOversampling and
 * BoostedSeedOversampling, pygrank/algorithms/postprocess/oversampling.py:9-130) need from the engine beyond include/pgh.h: the work
 * between two runs of the base ranker, for up to 64 seed sets at once, as four passes over [n, b] slabs.
 *
 * The reference finds a threshold with `min(ranks[u] for u in personalization if personalization[u] == 1)`, builds the next seed set
 * with a dictionary comprehension over the nodes and combines the rounds of the boosted variant with three more comprehensions: on a
 * device vector that is one read per node, on backend primitives about a dozen passes with temporaries per round and column.  Here a
 * round of B seed sets is one multi-seed run of the ranker plus:
 *   pgh_seed_floor     the lowest rank a seed holds, and how many seeds there are          (once, before the first round)
 *   pgh_seed_resample  the nodes that reach that rank become the next seeds
 *   pgh_boost_forms    the three sums the weight of a round is made of
 *   pgh_boost_update   the weighted rank sum, and the next round's threshold in the same pass
 *
 * All slabs are row-major f32 [n, b] with 1 <= b <= 64 and equal shapes.  Arithmetic is in f64 from the stored f32 values; a store is
 * rounded once to f32.  Counts are 64-bit integers.  Every column keeps its own threshold, weight, sums and counts.
 *
 * Reductions: an element belongs to a lane and a lane to one of a FIXED number of slab parts, whatever the launch; a part's lanes are
 * folded per column in lane order, the parts in index order (the scheme of pgh_mat_col_stats, include/pgh_measure.h).  No atomics: two
 * calls on the same input return the same bits, whatever the grid shape.  Behaviour on NaN ranks is unspecified.
 *
 * A request an entry does not serve returns PGH_OVERSAMPLE_DECLINED with nothing written (the error text says why): the caller then
 * takes the backend-primitive route.  Any other non-zero status is an error; nothing is written then either.
 */
#ifndef PGH_OVERSAMPLE_H
#define PGH_OVERSAMPLE_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_OVERSAMPLE_DECLINED 2
/* most columns of one call */
#define PGH_OVERSAMPLE_MAX_COLS 64

/* Per column c:  floor_host[c] = min of ranks[i, c] over the rows with seeds[i, c] == 1 exactly (a selection: one of the stored f32
 * values, exactly),  count_host[c] = the number of such rows.  A column without such a row gives count 0 and floor +inf.
 * Declined: b > 64.  Shape mismatches and null arguments are errors.  Synchronises. */
int pgh_seed_floor(pgh_mat_t ranks, pgh_mat_t seeds, double* floor_host /* [b] */, int64_t* count_host /* [b] */);

/* out[i, c] = 1 when ranks[i, c] >= (float)floor_host[c]  (strict != 0: >),  or when `keep` is given and keep[i, c] == 1;  else 0.
 * count_host[c] = the number of ones written to column c.  The comparison is between f32 values: the floor is the f32 it came from.
 * `out` may be `keep`, not `ranks`.
 * Declined: b > 64, a non-finite floor.  Shape mismatches, out == ranks and null arguments other than `keep` are errors.
 * Synchronises. */
int pgh_seed_resample(pgh_mat_t ranks, const double* floor_host /* [b] */, int32_t strict, pgh_mat_t keep /* nullable */, pgh_mat_t out,
                      int64_t* count_host /* [b] */);

/* The sums of BoostedSeedOversampling._boosting_weight (oversampling.py:95-103), per column c with s = seeds[i, c], R = fresh[i, c],
 * RN = total[i, c]:
 *   forms_host[3c] = S1 = sum s * R^2,   forms_host[3c + 1] = S2 = sum R^2,   forms_host[3c + 2] = S3 = sum s * RN * R
 * Declined: b > 64.  Shape mismatches and null arguments are errors.  Synchronises. */
int pgh_boost_forms(pgh_mat_t seeds, pgh_mat_t fresh, pgh_mat_t total, double* forms_host /* [3 * b] */);

/* total[i, c] = (float)(total[i, c] + weights_host[c] * fresh[i, c]), in place (oversampling.py:125), and in the same pass what
 * pgh_seed_floor(total AFTER the update, mask, floor_host, count_host) would return: the next round's threshold.  `mask` is the seed
 * slab the round ran on (oversampling "previous") or the original personalization ("original").
 * Declined: b > 64, a non-finite weight.  Shape mismatches, total == fresh, total == mask and null arguments are errors.
 * Synchronises. */
int pgh_boost_update(pgh_mat_t total, pgh_mat_t fresh, const double* weights_host /* [b] */, pgh_mat_t mask, double* floor_host /* [b] */,
                     int64_t* count_host /* [b] */);

#ifdef __cplusplus
}
#endif

#endif /* PGH_OVERSAMPLE_H */
