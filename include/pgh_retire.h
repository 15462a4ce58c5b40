/*
 * pgh_retire.h -- the multi-seed device loops of include/pgh.h, include/pgh_batch.h and include/pgh_mixed.h in the mode that RETIRES
 * CONVERGED COLUMNS inside the loop.
 *
 * A plain multi-seed run streams every column of its [n, ld] slabs until the slowest column has stopped: a stopped column is copied
 * forward bit for bit by every executed step and fetched by every gather.  The entries below run the same loops -- the same kernels, the
 * same per-column quotient, residual, stopping iteration -- and NARROW the run between two steps once few enough columns are still live:
 * the stopped columns leave for `ranks`, the live ones are repacked into an [n, ld'] workspace and the loop goes on there with the
 * narrower forms of its kernels (16, 8 or 4 lanes per row for ld' <= 64, 32, 16).  Nothing about a column's arithmetic changes, only the
 * columns that accompany it: a narrowed column may still differ from the plain entry's in its last bits, because the order in which the
 * rows of a pass are folded into the per-column sums depends on ld.
 *
 * levels      strictly descending live-column counts, each in [1, 63]; null: {32, 16, 8, 4}.  After the committed close of a step, if
 *             the number of live columns is at or below the greatest level that lies below the current slab width ld (and a narrower slab
 *             results: at or below ld - 4), the run narrows to ld' = (live + 3) & ~3.  num_levels == 0 never narrows.  There is no minimum
 *             stage length.  A list that is not strictly descending or holds a value outside [1, 63] is an error.
 * report      nullable.  A run is a sequence of stages, one per slab width; at most PGH_RETIRE_MAX_STAGES (a run that has reached that
 *             many stays in its last one).
 * results[j]  what the plain entry reports for the caller's column j; bit 5 of flags (32) is set on every column of a run that narrowed
 *             at least once.
 *
 * Served: what the plain sibling serves.  The closed-form filters' loop, graph_dropout and the f64 loops are not served; neither is
 * anything the plain entries decline (a graph that is not square or lacks the blocked layout, an absorption + degree of zero): such a
 * call returns PGH_RETIRE_DECLINED with nothing written and the caller takes the plain entry.
 */
#ifndef PGH_RETIRE_H
#define PGH_RETIRE_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_RETIRE_DECLINED 2
#define PGH_RETIRE_MAX_STAGES 8
#define PGH_RETIRE_NARROWED 32 /* pgh_loop_result::flags */

typedef struct pgh_retire_report {
    int32_t num_stages;                         /* >= 1 */
    int32_t reserved;
    int32_t ld[PGH_RETIRE_MAX_STAGES];          /* the stage's slab width */
    int32_t live[PGH_RETIRE_MAX_STAGES];        /* live columns when it starts (stage 0: b) */
    int32_t first_step[PGH_RETIRE_MAX_STAGES];  /* its first step (stage 0: 1); step k is iteration k + 1 */
    int64_t column_steps;                       /* sum over the executed steps of the slab's ld: what was streamed */
} pgh_retire_report;

int pgh_ppr_run_batch_retire(pgh_graph_t g, pgh_mat_t p, pgh_mat_t ranks, const pgh_loop_cfg* cfg, const double* out_scales,
                             pgh_loop_result* results, const int32_t* levels, int32_t num_levels, pgh_retire_report* report);

int pgh_ppr_run_batch_mixed_retire(pgh_graph_t g, pgh_mat_t p, pgh_mat_t ranks, const pgh_loop_cfg* cfg, const double* alphas /* [b], host */,
                                   const double* out_scales, pgh_loop_result* results, const int32_t* levels, int32_t num_levels,
                                   pgh_retire_report* report);

int pgh_absorb_run_batch_retire(pgh_graph_t g, pgh_mat_t p, pgh_vec_t lam, pgh_mat_t out, const pgh_loop_cfg* cfg, const double* out_scales,
                                pgh_loop_result* results, const int32_t* levels, int32_t num_levels, pgh_retire_report* report);

int pgh_sarw_run_batch_retire(pgh_graph_t g, pgh_mat_t p, pgh_mat_t out, const pgh_loop_cfg* cfg, const double* out_scales,
                              pgh_loop_result* results, const int32_t* levels, int32_t num_levels, pgh_retire_report* report);

#ifdef __cplusplus
}
#endif

#endif /* PGH_RETIRE_H */
