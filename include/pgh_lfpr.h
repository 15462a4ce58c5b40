/*
 * pgh_lfpr.h -- what the locally fair PageRank of [tsioutsiouliklis2021fairness] (the reference's LFPR,
 * pygrank/algorithms/filters/adhoc.py:196-314) needs from the engine beyond include/pgh.h: the filter's row operands in one pass, and
 * everything that follows the product of one step in one pass.
 *
 * The reference's fair matrix is Q @ W with Q = diag(d), a row scaling of the raw adjacency, so conv(x, Q @ W) = W^T (d * x): the loop
 * runs on the raw-adjacency graph and scales the iterate by d before each product.  What follows W^T (d * x) in a step is elementwise
 * plus five sums -- the rank-two correction deltaR * xR + deltaB * xB, the next product's operand d * y, sum(y) for the quotient, the
 * next step's deltaR and deltaB, the residual -- about ten backend calls on the primitive route, ONE streaming kernel here.
 *
 * Both entries work on plain vectors of equal length and know nothing about graphs or id spaces: they serve vectors in a graph's
 * resident id space (pgh_graph_resident_len; padding slots hold zeros in every operand) and vectors in the caller's ids alike.
 *
 * Sums are accumulated in f64 by the engine's deterministic reduction (wavefront shuffles, LDS, block partials, a single-workgroup
 * fold; no atomics): two calls on the same input return the same bits.
 *
 * A request an entry does not serve returns PGH_LFPR_DECLINED with nothing written (the error text says why): the caller then takes the
 * backend-primitive route.  Any other non-zero status is an error; nothing is written then either.
 */
#ifndef PGH_LFPR_H
#define PGH_LFPR_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_LFPR_DECLINED 2

/* LFPR.normalization + LFPR._start (adhoc.py:227-241, 256-281), one pass.  Per i, in f64 from the stored f32 operands,
 * rounded ONCE to f32 at each store, products in the reference's order:
 *   R = out_r[i], B = out_b[i], s = sensitive[i], o = original ? original[i] : 1,   inv(v) = v != 0 ? 1 / v : 0
 *   case1 = R < phi * (R + B);  case2 = !case1 && R != 0;  case3 = neither
 *   d[i]  = case1 ? inv(B) * (1 - phi) : case2 ? inv(R) * phi : 1
 *   dR[i] = case1 ? phi - (1 - phi) * inv(B) * R : case3 ? phi : 0
 *   dB[i] = case2 ? (1 - phi) - phi * inv(R) * B : case3 ? 1 - phi : 0
 *   xR[i] = o * s;   xB[i] = o * (1 - s)                       (un-normalised)
 *   sums_host[0] = sum xR, sums_host[1] = sum xB               (f64 over the stored values, deterministic; synchronises)
 * Declined: a non-finite phi.  Length mismatches, an output that is another output or an input, and null arguments other than
 * `original` are errors. */
int pgh_lfpr_setup(pgh_vec_t sensitive, pgh_vec_t out_r, pgh_vec_t out_b, pgh_vec_t original /* nullable */, double phi,
                   pgh_vec_t d, pgh_vec_t dR, pgh_vec_t dB, pgh_vec_t xR, pgh_vec_t xB, double* sums_host /* [2] */);

/* What follows the product in one LFPR step (LFPR._formula adhoc.py:284-293, the quotient abstract_filters.py:133-134, the
 * residual convergence.py:96-101).  y0 = alpha * x_scale * W^T(d * x) + (1 - alpha) * p comes from the existing step entry.
 *   y[i] = y0[i] + cR * xR[i] + cB * xB[i]          (f64, rounded once)
 *   u[i] = y[i] * d[i]                              (operand of the next product, from the rounded y)
 *   t_i  = y[i] * y_scale - x[i] * x_scale          (y_scale = the caller's prediction of 1 / sum y)
 *   sums_host = { sum y, sum y*dR, sum y*dB,  kind L1 / MABS: sum |t_i|,  kind LINF: max |t_i|,  sum sign(t_i) * y[i] }
 * (every sum over the stored y; sign(0) = 0).  The last sum lets the caller correct an L1 residual for the true 1 / sum y, as the
 * PageRank loops do (DESIGN.md section 5, R = R' + (inv - inv') * D).  y may be y0 itself; u, y and x are otherwise distinct from
 * each other and from every input.  Synchronises.
 * Declined: a non-finite cR, cB, x_scale or y_scale, an err_kind other than PGH_ERR_MABS / PGH_ERR_L1 / PGH_ERR_LINF.  Length
 * mismatches, a forbidden aliasing and null arguments are errors. */
int pgh_lfpr_close(pgh_vec_t y0, pgh_vec_t x, double x_scale, pgh_vec_t xR, pgh_vec_t xB, pgh_vec_t d, pgh_vec_t dR, pgh_vec_t dB,
                   double cR, double cB, double y_scale, int32_t err_kind, pgh_vec_t y, pgh_vec_t u, double* sums_host /* [5] */);

#ifdef __cplusplus
}
#endif

#endif /* PGH_LFPR_H */
