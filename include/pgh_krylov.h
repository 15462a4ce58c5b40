/*
 * pgh_krylov.h -- what the Krylov-space filters (the reference's ClosedFormGraphFilter(krylov_dims=...), abstract_filters.py:196-267
 * over pygrank/algorithms/filters/krylov_space.py:16-57) need from the engine beyond include/pgh.h: everything that follows the
 * product of one Lanczos step in one pass, and the convergence residuals of up to 64 filter iterations in one pass over the basis.
 *
 * Both entries work on plain vectors and [n, b] slabs and know nothing about graphs or id spaces: they serve vectors in a graph's
 * resident id space (pgh_graph_resident_len; padding slots hold zeros in every operand) and vectors in the caller's ids alike.
 *
 * Sums are accumulated in f64 by the engine's deterministic reduction (wavefront shuffles, LDS, block partials, a single-workgroup
 * fold; no atomics): two calls on the same input return the same bits.
 *
 * A request an entry does not serve returns PGH_KRYLOV_DECLINED with nothing written (the error text says why): the caller then takes
 * the backend-primitive route.  Any other non-zero status is an error; nothing is written then either.
 */
#ifndef PGH_KRYLOV_H
#define PGH_KRYLOV_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_KRYLOV_DECLINED 2
#define PGH_KRYLOV_MAX_DIMS 64     /* columns of a basis slab pgh_krylov_residuals reads */
#define PGH_KRYLOV_MAX_PROBES 64   /* filter iterations per pgh_krylov_residuals pass */

/* What follows the product w = conv(v) in one Lanczos step (krylov_space.py:28-31), one pass.  Per i, in f64 from the stored f32
 * operands, in the reference's order, rounded ONCE to f32:
 *   out[i] = (w[i] - a * v[i]) - b * u[i]                      (the last term is dropped when u is NULL)
 *   basis[i, col] = out[i]                                      (when basis is given: no pgh_mat_set_col pass)
 *   sums_host = { sum out^2, sum out * v }                      (over the STORED out; the second is the loss-of-orthogonality diagnostic)
 * Normalisation never gets a pass of its own: the caller keeps the raw out and carries 1 / sqrt(sum out^2) as a host scalar into the
 * next product's multiplier, the next pgh_dot, the next close's a and b, and one pgh_mat_div_cols over the finished slab.
 * out is distinct from w, v and u.  Synchronises.
 * Declined: a non-finite a or b.  Length mismatches, col outside the slab, a forbidden aliasing and a null w, v, out or sums_host
 * are errors. */
int pgh_lanczos_close(pgh_vec_t w, pgh_vec_t v, double a, pgh_vec_t u /* nullable */, double b, pgh_vec_t out,
                      pgh_mat_t basis /* nullable */, int32_t col, double* sums_host /* [2] */);

/* The convergence residuals of `probes` filter iterations in one pass over the basis: an [n, count] x [count, probes] product whose
 * columns are reduced instead of stored (nothing of size n is written).  With r[i, t] = sum_{c < count} basis[i, c] * deltas[c * probes + t]
 * accumulated in f64 in ascending c:
 *   abssum_host[t] = sum_i |r[i, t]|,   absmax_host[t] = max_i |r[i, t]|
 * Limits: 1 <= count <= basis.b <= PGH_KRYLOV_MAX_DIMS, 1 <= probes <= PGH_KRYLOV_MAX_PROBES; anything else is an error, as are null
 * arguments.  Declined: a non-finite delta.  n == 0 returns zeros.  Synchronises. */
int pgh_krylov_residuals(pgh_mat_t basis, const double* deltas_host /* [count * probes], row-major */, int32_t count, int32_t probes,
                         double* abssum_host /* [probes] */, double* absmax_host /* [probes] */);

#ifdef __cplusplus
}
#endif

#endif /* PGH_KRYLOV_H */
