/*
 * pgh_tune.h -- what a parameter tuner needs from the engine beyond include/pgh.h: the AUC of up to 64 probes (coefficient
 * vectors of a closed-form filter) in ONE streaming pass over the stored powers of a personalization.
 *
 * A coordinate step of the reference's tuner (autotune/optimization.py:160-180, autotune/parameterized.py:135-145) scores a
 * handful of candidates that share their personalization, hence their power slab (filters._PowerSlab, one [n, 64] slab).  Scored
 * one by one each candidate costs a pass over the slab, a normalisation, two compactions and a radix sort of n pairs.  The AUC is a
 * count over (positive, negative) pairs and the positives of a validation split are few: their scores are sorted once per probe,
 * every negative row is read once, and two binary searches per probe give the pairs that row wins, ties and loses.  No sort of n
 * elements and no [n, probes] intermediate.
 *
 * The counts are 64-bit integers throughout (lane, wavefront, workgroup, device), so a result does not depend on the grid
 * shape or on the order in which workgroups arrive.
 *
 * A request these entries do not serve returns PGH_TUNE_DECLINED with nothing written (the error text says why): the caller
 * then scores the probes column by column.  Any other non-zero status is an error.
 */
#ifndef PGH_TUNE_H
#define PGH_TUNE_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_TUNE_DECLINED 2
/* coefficients (terms * probes doubles) + sorted positives (probes * num_positive floats) stay in LDS up to this many bytes per
 * workgroup (two workgroups per CU fit the 160 KiB of a gfx950 CU with room to spare); above it the positives are searched in
 * global memory (they stay in L2) */
#define PGH_TUNE_LDS_BYTES 61440
/* more positives than this are declined (the per-probe sort is one workgroup's LDS) */
#define PGH_TUNE_MAX_POSITIVES 8192

typedef struct pgh_probe_plan_s* pgh_probe_plan_t;

/* Node classes of one (known scores, exclude) pair, built once per validation split and reused by every step:
 * positive = known != 0 and exclude == 0, negative = known == 0 and exclude == 0 (the rule of filter_out); exclude is
 * nullable.  One pass writes a class byte per node, counts both classes and lists the positives' rows. */
int pgh_probe_plan_create(pgh_vec_t known, pgh_vec_t exclude, pgh_probe_plan_t* out);
int pgh_probe_plan_info(pgh_probe_plan_t plan, int64_t* num_positive, int64_t* num_negative);
int pgh_probe_plan_destroy(pgh_probe_plan_t plan);

/* auc[q] = AUC of the scores  s_q[i] = (float) sum_{j < terms} (double) slab[i, j] * coeffs[j * probes + q]  (the value the
 * [n, terms] x [terms, probes] product of include/pgh.h stores: f64 accumulation in j order, one rounding to f32) against the
 * plan's classes, ties at their mid-rank: what the engine's sort-based AUC returns for the filtered column against the filtered
 * known scores.  1 <= probes <= 64, 1 <= terms <= columns of the slab <= 64, rows of the slab = length of the plan's vectors.
 * Declined: terms > 64, a plan without positives or without negatives, more than PGH_TUNE_MAX_POSITIVES positives, a non-finite
 * coefficient. */
int pgh_probe_auc(pgh_mat_t slab, const double* coeffs_host, int32_t terms, int32_t probes, pgh_probe_plan_t plan,
                  double* auc_host);

#ifdef __cplusplus
}
#endif

#endif /* PGH_TUNE_H */
