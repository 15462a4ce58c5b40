/*
 * pgh_arnoldi.h -- what an Arnoldi step (the reference's arnoldi_iteration, pygrank/algorithms/filters/krylov_space.py:60-85) needs from
 * the engine beyond include/pgh.h: the inner products of a vector with every column of the basis slab in one pass, and the pass that
 * subtracts the projection, stores the next raw column and returns that column's inner products with the basis.
 *
 * The reference orthogonalises by modified Gram-Schmidt: h_j = <q_j, v>, v -= h_j q_j for j = 0 .. k - 1, one after the other, 2 k vector
 * passes.  With c = Q^T v and G = Q^T Q the same coefficients solve the unit lower triangular system (I + strictly_lower(G)) h = c, for
 * ANY Q (the reference's first column is L1-normalised, so Q is not orthonormal and classical Gram-Schmidt would not reproduce it):
 * pgh_basis_dots returns c, the host solves the k x k system in f64, pgh_arnoldi_close forms v - Q h and returns the next row of G.
 *
 * Both entries work on plain vectors and [n, b] slabs and know nothing about graphs, id spaces or column scales.
 *
 * Sums are accumulated in f64 over a fixed number of row parts that are folded in index order (no atomics): two calls on the same
 * input return the same bits whatever the grid.
 *
 * A request an entry does not serve returns PGH_ARNOLDI_DECLINED with nothing written (the error text says why): the caller then takes
 * the backend-primitive route.  Any other non-zero status is an error; nothing is written then either.
 */
#ifndef PGH_ARNOLDI_H
#define PGH_ARNOLDI_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_ARNOLDI_DECLINED 2
#define PGH_ARNOLDI_MAX_DIMS 64    /* columns of a basis slab either entry reads */

/* dots_host[j] = sum_i basis[i, j] * w[i] for j < count;  dots_host[count] = sum_i w[i]^2.
 * Limits: 1 <= count <= basis.b <= PGH_ARNOLDI_MAX_DIMS; anything else is an error, as are a length mismatch and null arguments.
 * n == 0 returns zeros.  Synchronises. */
int pgh_basis_dots(pgh_mat_t basis, int32_t count, pgh_vec_t w, double* dots_host /* [count + 1] */);

/* out[i] = f32( w[i] - sum_{j < count} coeffs[j] * basis[i, j] )   -- f64 from the stored f32 operands, ascending j, rounded ONCE;
 * basis[i, col] = out[i] when col >= 0 (col >= count: the columns read are not the column written; other columns untouched);
 * over the STORED out:  dots_host[j] = sum_i basis[i, j] * out[i] (j < count),  dots_host[count] = sum_i out[i]^2.
 * Limits as above; out is distinct from w.  Declined: a non-finite coefficient.  Length mismatches, 0 <= col < count, col >= basis.b,
 * out sharing w's memory and null arguments are errors.  n == 0 returns zeros.  Synchronises. */
int pgh_arnoldi_close(pgh_mat_t basis, int32_t count, pgh_vec_t w, const double* coeffs_host /* [count] */, pgh_vec_t out,
                      int32_t col, double* dots_host /* [count + 1] */);

#ifdef __cplusplus
}
#endif

#endif /* PGH_ARNOLDI_H */
