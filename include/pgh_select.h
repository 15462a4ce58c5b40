/*
 * pgh_select.h -- node selections that leave the device as lists: which rows of a vector pass a test (and their values), the inverse
 * scatter, and the k best rows of every column of a slab.  What Subgraph, Supergraph, GraphSignal.top and DeviceMatrix.top of
 * pygrank_amd need (the reference's pygrank/algorithms/postprocess/subgraph.py:5-68) so that a selection of count rows costs count
 * indices on the way to the host, not a download of all n values.  The slab passes of MabsMaintain and SeparateNormalization
 * (pygrank/algorithms/postprocess/postprocess.py:83-103,475-503) live here too.
 *
 * Vectors are f32, slabs are row-major f32 [n, b].  Indices are int32 rows.  Per-column host arguments are doubles and are rounded to
 * f32 once, as pgh_ewise_vs rounds its scalar.
 *
 * No floating-point atomics.  Every position of a list is an integer prefix of fixed stretches of rows, so a result depends on neither
 * the grid nor the arrival order: two calls on the same input return the same bytes.
 *
 * A request an entry does not serve returns PGH_SELECT_DECLINED with nothing written (the error text says why): the caller takes the
 * other route.  Any other non-zero status is an error with the error text set; nothing is written then either.
 */
#ifndef PGH_SELECT_H
#define PGH_SELECT_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_SELECT_DECLINED 2
/* `mode` of the row test */
#define PGH_SELECT_NONZERO 0
#define PGH_SELECT_GT 1
#define PGH_SELECT_GE 2
/* most rows per column of one top-k call: 32 KB of (key, row) pairs per workgroup */
#define PGH_TOPK_MAX_K 4096
/* most columns of one slab call */
#define PGH_SELECT_MAX_COLS 64

/* The rows of x that pass the test:  PGH_SELECT_NONZERO  x[i] != 0  (-0.0 is zero, a NaN is selected, `cut` is not read)
 *                                    PGH_SELECT_GT       x[i] >  (float)cut
 *                                    PGH_SELECT_GE       x[i] >= (float)cut
 * *count receives how many there are.  When *count <= capacity their indices go to idx_host[0 .. *count) in ascending order and, when
 * `values` is given (at least `capacity` entries, not x itself), their stored values to values[0 .. *count) in the same order.  When
 * *count > capacity only *count is written and the status is 0: the caller comes back with a larger capacity.
 * A count pass (one count per workgroup over a fixed stretch of rows), an exclusive sum of those counts, a write pass in which a
 * wavefront places its rows at the workgroup's offset + the earlier wavefronts' counts + its ballot prefix.
 * Errors: n >= 2^31, an unknown mode, a negative capacity, null x / idx_host / count.  Synchronises. */
int pgh_vec_select(pgh_vec_t x, int32_t mode, double cut, int64_t capacity, int32_t* idx_host, pgh_vec_t values, int64_t* count);

/* out[t] = x[idx_host[t]], t < count.  The indices are checked on the host before anything is launched: inside [0, n), strictly
 * ascending, count <= the length of out; out is not x.  A bad index is an error, never an out-of-range access.  Synchronises. */
int pgh_vec_gather(pgh_vec_t x, const int32_t* idx_host, int64_t count, pgh_vec_t out);

/* dst[idx_host[t]] = src[t], t < count; every other entry of dst keeps its bits.  The same checks (count <= the length of src; strictly
 * ascending indices: no duplicate, so the outcome does not depend on an order of stores).  Synchronises. */
int pgh_vec_scatter(pgh_vec_t dst, const int32_t* idx_host, int64_t count, pgh_vec_t src);

/* For every column j the k rows with the largest stored values, by value descending, ties by ascending row -- the order
 * pgh_vec_ordinals defines; -0.0 and +0.0 tie.  idx_host[t * b + j] is the row in place t, val_host[t * b + j] its stored value,
 * widened.  +-inf and denormals are ordinary values.  A NaN makes its own column unspecified (rows inside [0, n) all the same) and
 * changes no other column.
 * pgh_post_kth_largest gives every column's cut; one pass counts, per wavefront stretch of rows and column, the rows above the cut and
 * the rows equal to it; a scan per column turns the counts into offsets; one pass places every row above the cut and the first
 * k - (rows above) rows equal to it, in row order; one workgroup per column sorts its k (value, row) pairs in LDS.
 * Declined: b > 64, k > PGH_TOPK_MAX_K.  Errors: k outside [1, n], n >= 2^31, null arguments.  Synchronises. */
int pgh_mat_topk(pgh_mat_t m, int64_t k, int32_t* idx_host /* [k][b] */, double* val_host /* [k][b] */);

/* out[i, j] = m[i, j] * (float)scale_host[j]: the f32 product pgh_ewise_vs stores under PGH_MUL for column j.
 * Declined: b > 64.  Shape mismatches, out == m and null arguments are errors. */
int pgh_mat_col_scale(pgh_mat_t m, const double* scale_host /* [b] */, pgh_mat_t out);

/* s has n entries.  sums_host[2 j] = sum_i f32(m[i, j] * s[i]), sums_host[2 j + 1] = sum_i f32(m[i, j] * f32(1 - s[i])): the sums of the
 * f32 values pgh_ewise_vv stores under PGH_MUL (the second factor being what pgh_ewise_vs stores under PGH_SUB, reflected), added in
 * f64 in a fixed order.
 * Declined: b > 64.  Shape mismatches and null arguments are errors.  Synchronises. */
int pgh_mat_split_sums(pgh_mat_t m, pgh_vec_t s, double* sums_host /* [b][2] */);

/* out[i, j] = f32(f32(m[i, j] * s[i]) * (float)a_host[j]) + f32(f32(m[i, j] * f32(1 - s[i])) * (float)b_host[j]): five f32 operations in
 * this order, no contraction.
 * Declined: b > 64.  Shape mismatches, out == m and null arguments are errors. */
int pgh_mat_split_blend(pgh_mat_t m, pgh_vec_t s, const double* a_host /* [b] */, const double* b_host /* [b] */, pgh_mat_t out);

#ifdef __cplusplus
}
#endif

#endif /* PGH_SELECT_H */
