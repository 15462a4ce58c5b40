/*
 * pgh_gnn.h -- what training through a propagation needs from the engine beyond include/pgh.h (pygrank_amd/gnn.py; the reference's APPNP
 * example, tests/test_gnn.py:22-28: ranker.propagate(graph, features, graph_dropout=0.5 if training else 0) inside a model's forward
 * pass): the transposed graph built in HBM, whose multi-seed image applies the TRANSPOSE of the masked matrix its partner applies for the
 * same seed; one resident loop that serves the forward and the adjoint recurrences of the linear filters; a view of a slab somebody
 * else owns (a torch tensor).
 *
 * The dropout mask is a pure function of (seed, index of the entry in CSR(M^T) order of the graph it was drawn on).  The multi-seed
 * kernel reads that index from one word per stream entry; the transposed graph's words hold, for its entry (i, j), the index of the
 * mirrored entry (j, i) of its partner.  So for every seed  masked(gt, seed) = masked(g, seed)^T  entry for entry, and the adjoint of a
 * run of K masked steps on g is K steps on gt with the same seeds in descending order.  A symmetric M needs this as well: its mask is
 * not symmetric.
 *
 * An input an entry does not serve returns PGH_GNN_DECLINED with nothing written (pgh_last_error says why); any other non-zero status
 * is an error.
 */
#ifndef PGH_GNN_H
#define PGH_GNN_H

#include "pgh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_GNN_DECLINED 2

/* *out = the graph whose stored CSR is the transpose of g's stored CSR(M^T): its conv is x -> M x.  Built from g's arrays in HBM (one
 * stable sort by column, no host copy of the matrix): pgh_graph_download(*out) is the transpose of pgh_graph_download(g) with the
 * entries of a row in ascending column order, repeated entries kept in their order, values bit for bit.  A value-free g (integer
 * multiplicities between two scale vectors) gives a value-free *out with the two scales swapped.
 * *out records g as its MASK PARTNER: the index words of its multi-seed image are built here, from g's CSR, and *out does not refer
 * to g afterwards (g may be destroyed first).  pgh_spmm_dropout, pgh_ppr_run_batch_dropout and pgh_linear_run_batch on *out apply
 * masked(g, seed)^T.  The single-vector dropout entries (pgh_spmv_dropout, pgh_ppr_run_dropout) and pgh_graph_degrees_dropout have no
 * mirrored index words: on *out they return an error that says so.
 * Declined: a graph without the stored CSR or without the blocked layout, a non-square graph, a slice of a row partition. */
int pgh_graph_transposed(pgh_graph_t g, pgh_graph_t* out);

/* One resident multi-seed loop for the linear recurrences of a forward and of a backward pass, b columns at once:
 *     s_0 = s0 * v,                                   acc  = c[0] * s_0
 *     s_k = a[k-1] * (A_k s_{k-1}) + b[k-1] * v,      acc += c[k] * s_k        k = 1 .. steps
 *     out = acc
 * A_k is the stored M^T of g under the mask of seed  seed_first + (k - 1) * seed_stride  (rate in (0, 1)), the plain M^T for rate == 0.
 * v and out are [n, b] f32 slabs, 1 <= b <= 64, and may not share memory; a, b, c are host arrays.  The iterate stays in the
 * multi-seed image's id space from the way in to the way out; a step is the masked product and one close kernel that reads the
 * step's row sums, v and acc once and writes the next iterate in gather form and acc.  Row sums as in pgh_spmm (f64 within a tile
 * piece, f32 across); a, b, c are rounded to f32 once; every other operation is one f32 operation.  No residual, no quotient and no
 * host look between the steps; loop_ms (nullable) is the time between the first and the last launch, by events.  Synchronises.
 *   PageRank, K products, no quotient:        s0 = 1, a = alpha, b = 1 - alpha, c = e_K, stride +1
 *   its adjoint (on the transposed graph):    s0 = 1, a = 1, b = 0, c_j = (1 - alpha) alpha^j (j < K), c_K = alpha^K,
 *                                             seed_first = the forward's + K - 1, stride -1
 *   sum_k c_k (M^T)^k (taylor form):          s0 = 1, a = 1, b = 0, c, stride +1
 *   its adjoint (Horner, transposed graph):   s0 = c_K, a = 1, b[k-1] = c_{K-k}, c = e_K, seed_first = the forward's + K - 1, stride -1
 * Declined: a graph without the blocked layout or (rate > 0) without the stored CSR, a non-square graph, b > 64.  Shape mismatches,
 * steps < 0, a rate outside [0, 1) and null arguments are errors. */
int pgh_linear_run_batch(pgh_graph_t g, pgh_mat_t v, double s0, int32_t steps, const double* a /* [steps] */,
                         const double* b /* [steps] */, const double* c /* [steps + 1] */, pgh_mat_t out, double rate,
                         uint64_t seed_first, int64_t seed_stride, double* loop_ms);

/* A non-owning view of a contiguous row-major f32 [n, b] buffer in device memory, as pgh_vec_wrap is for vectors: pgh_mat_free
 * releases the handle and leaves the buffer alone.  The caller keeps the buffer alive and orders its own work on it against the
 * engine's stream (pgh_set_stream). */
int pgh_mat_wrap(void* device_ptr, int64_t n, int32_t b, pgh_mat_t* out);

#ifdef __cplusplus
}
#endif

#endif /* PGH_GNN_H */
