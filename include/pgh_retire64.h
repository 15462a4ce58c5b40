/*
 * pgh_retire64.h -- the recursive f64 multi-seed loops of include/pgh_batch64.h in the mode that RETIRES CONVERGED COLUMNS inside the
 * loop (include/pgh_retire.h for the f32 loops), and the product pass their last stage ends in.
 *
 * The entries below run the loops of their pgh_batch64.h siblings -- the same kernels, the same per-column quotient, residual and
 * stopping iteration -- and NARROW the run between two steps once few enough columns are still live: the stopped columns leave for `out`
 * (the f64 iterate times quotient x output scale in f64, rounded once to f32, as the plain way out does it), the live ones are repacked
 * into [n, ld'] slabs of doubles and the loop goes on there with the narrower forms of its kernels.  A slab is ld = (b + 1) & ~1
 * doubles wide.
 *
 * levels      strictly descending live-column counts, each in [1, 63]; null with num_levels != 0: {32, 16, 8, 4, 2}.  After the
 *             committed close of a step that leaves `live` columns not yet stopped, the run narrows to ld' = (live + 1) & ~1 when
 *             0 < live <= min(greatest level below ld, ld - 2).  num_levels == 0 never narrows.  A list that is not strictly descending
 *             or holds a value outside [1, 63] is an error.
 * report      nullable; pgh_retire_report of include/pgh_retire.h: at most PGH_RETIRE_MAX_STAGES stages (a run that has reached that
 *             many stays in its last one), live[0] = b, first_step[0] = 1, step numbers go on across stages, column_steps is the sum of
 *             ld over the executed steps.
 * results[j]  what the plain f64 entry reports for the caller's column j; PGH_RETIRE_NARROWED (bit 5 of flags) is set on every column
 *             of a run that narrowed.  A zero column (in_norms[j] == 0) leaves at the first narrowing as zeros with 0 iterations.
 *
 * A run that never narrows is bit-identical to the plain f64 entry.  A narrowed column may differ in the last bits of its f64 sums (the
 * rows of a pass are folded in an order that depends on ld); the f32 value it rounds to stays within one ulp.
 *
 * A stage with ld == 2 that a narrowing led to runs its product pass in the PAIR FORM: one lane per stream entry and a segmented scan
 * over the wavefront, instead of four lanes per 512-entry tile of which one holds columns.  (A run that STARTS one pair wide never
 * narrows and keeps the plain entry's form and bits.)  PGH_MM64_PAIR=0 in the environment, read per call, keeps the four-lane form.
 *
 * What the plain sibling declines is declined (PGH_RETIRE_DECLINED, nothing written) and the caller takes the plain f64 entry.  The
 * closed-form loop (pgh_poly_run_batch_f64) is not served.
 */
#ifndef PGH_RETIRE64_H
#define PGH_RETIRE64_H

#include "pgh_batch64.h"
#include "pgh_retire.h"

#ifdef __cplusplus
extern "C" {
#endif

int pgh_ppr_run_batch_f64_retire(pgh_graph_t g, pgh_mat_t p, pgh_mat_t out, const pgh_loop_cfg* cfg, const double* out_scales,
                                 pgh_loop_result* results, const double* in_norms /* [b] */, const int32_t* levels, int32_t num_levels,
                                 pgh_retire_report* report);

int pgh_absorb_run_batch_f64_retire(pgh_graph_t g, pgh_mat_t p, pgh_vec_t lam, pgh_mat_t out, const pgh_loop_cfg* cfg,
                                    const double* out_scales, pgh_loop_result* results, const double* in_norms /* [b] */,
                                    const int32_t* levels, int32_t num_levels, pgh_retire_report* report);

int pgh_sarw_run_batch_f64_retire(pgh_graph_t g, pgh_mat_t p, pgh_mat_t out, const pgh_loop_cfg* cfg, const double* out_scales,
                                  pgh_loop_result* results, const double* in_norms /* [b] */, const int32_t* levels, int32_t num_levels,
                                  pgh_retire_report* report);

/* pgh_spmm_f64 for b = 1 or 2 with the product pass in the pair form: the primitive that runs that kernel alone.  Any other width is
 * an error; what pgh_spmm_f64 declines is declined. */
int pgh_spmm_f64_pair(pgh_graph_t g, const double* x_host, int32_t b /* 1 or 2 */, double* y_host);

#ifdef __cplusplus
}
#endif

#endif /* PGH_RETIRE64_H */
