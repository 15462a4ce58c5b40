"""Graphs, inputs and the row-wise bound of the f64 multi-seed product (include/pgh_batch64.h pgh_spmm_f64), shared by
tests/test_gpu_batch64.py (the engine) and tests/test_batch64_host.py (which proves that the bound rejects an f32 accumulation).

The bound of row i, column j:  |got - ref| <= (nnz_i + 4) 2^-53 S_ij,  S_ij = sum_k |m_ik x_kj|.  Derived, not measured: the a-priori
bound of a sum of nnz_i terms in ANY order is (nnz_i - 1) u S with u = 2^-53; each term carries one rounding of its product (the f32
value or the f32 source scale times an f64 operand is not exact; a value-free entry is added as it is), the row sum one for the output
scale, and the f64 copy of the operator the reference multiplies by (f64_common.effective_matrix: right_i * w * left_j) two.  The
reference itself is long double (64-bit significand: 2^-11 of every term above).  nnz_i counts stream entries: a multiplicity of m
is m entries."""
import numpy as np
import scipy.sparse as sp

import f64_common as fc

U53 = 2.0 ** -53
WIDTHS = (1, 2, 3, 5, 16, 17, 32, 33, 64)


def product_reference(op, X):
    """M^T X in long double, column by column."""
    X = np.asarray(X, dtype=np.float64)
    return np.stack([fc.matvec_ld(op.MT, X[:, j]) for j in range(X.shape[1])], axis=1)


def product_bound(op, X):
    S = op.absMT @ np.abs(np.asarray(X, dtype=np.float64))
    return (op.nnz_row[:, None] + 4.0) * U53 * S


def product_ratio(got, op, X):
    """The worst |got - ref| / bound over the rows whose bound is not zero, and whether every row with a zero bound is exactly zero."""
    ref, bound = product_reference(op, X), product_bound(op, X)
    err = np.abs(np.asarray(got, dtype=fc.LD) - ref).astype(np.float64)
    live = bound > 0
    exact = bool(np.all(err[~live] == 0))
    return (float(np.max(err[live] / bound[live])) if live.any() else 0.0), exact


def draw_x(rng, n, b):
    """Signed f32-representable values over thirteen binades; with more than one column, column b // 2 is zero."""
    X = (rng.choice([-1.0, 1.0], (n, b)) * 2.0 ** rng.uniform(-6, 7, (n, b))).astype(fc.F32).astype(np.float64)
    if b > 1:
        X[:, b // 2] = 0.0
    return X


def hub_graph(rng, n=8192, weights="mult"):
    """W[src, dst]: one row of M^T with 6000 distinct sources (at least 11 tiles of 512: a long chain of carries), one with 1100
    (3 tiles), 400 ids without in-edges (empty rows of M^T; 100 of them without any edge), a sparse random rest of 1 .. 4 in-edges.
    weights: "mult" -- integer multiplicities up to 3 (the upload stays value-free), "real" -- f32-representable weights in [0.5, 2)."""
    ids = rng.permutation(n)
    hub0, hub1, empty, rest = ids[0], ids[1], ids[2:402], ids[402:]
    senders = ids[:n - 100]                                   # the last 100 ids of the permutation send nothing ...
    senders = senders[~np.isin(senders, empty[:100])]         # ... and 100 of the empty rows send nothing either: isolated
    rows, cols = [rng.choice(senders, 6000, replace=False), rng.choice(senders, 1100, replace=False)], [np.full(6000, hub0), np.full(1100, hub1)]
    for dst in rest:
        k = int(rng.integers(1, 5))
        rows.append(rng.choice(senders, k, replace=False))
        cols.append(np.full(k, dst))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    W = sp.csr_array((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    W.sum_duplicates()
    assert W.nnz == len(rows) and not W[:, empty].nnz
    if weights == "mult":
        W.data = rng.choice([1.0, 2.0, 3.0], W.nnz, p=[0.88, 0.08, 0.04])
    else:
        W.data = rng.uniform(0.5, 2.0, W.nnz).astype(fc.F32).astype(np.float64)
    return W, hub0, hub1, empty


def small_graph(rng, n=50, entries=200):
    """n ids, `entries` distinct edges with multiplicities up to 3: less than one tile."""
    flat = rng.choice(n * n, entries, replace=False)
    W = sp.csr_array((rng.choice([1.0, 2.0, 3.0], entries, p=[0.8, 0.15, 0.05]), (flat // n, flat % n)), shape=(n, n))
    return W


def operator_of(W, kind):
    """The Operator (f64_common) of `W` under a normalisation whose f32 factors the test knows exactly: "col" / "symmetric" on a
    value-free upload (integer W, factors kept apart), "col-valued" / "symmetric-valued" as an f32 matrix of products.  Returns
    (Operator, upload(pg) -> DeviceGraph)."""
    from pygrank_amd.device import DeviceGraph
    W = sp.csr_array(W).astype(np.float64)
    out_w, in_w = np.asarray(W.sum(axis=1)).ravel(), np.asarray(W.sum(axis=0)).ravel()
    if kind == "col":
        left = fc.f32_inverse(out_w)
        return fc.effective_matrix(W, left, None), lambda pg: DeviceGraph.from_factored(W, left, None)
    if kind == "symmetric":
        left, right = fc.f32_inverse(out_w, 0.5), fc.f32_inverse(in_w, 0.5)
        return fc.effective_matrix(W, left, right), lambda pg: DeviceGraph.from_factored(W, left, right)
    if kind == "col-valued":
        M = sp.csr_array(sp.diags(fc.f32_inverse(out_w)) @ W)
    else:
        assert kind == "symmetric-valued"
        M = sp.csr_array(sp.diags(fc.f32_inverse(out_w, 0.5)) @ W @ sp.diags(fc.f32_inverse(in_w, 0.5)))
    M.data = M.data.astype(fc.F32).astype(np.float64)
    return fc.effective_matrix(M, valued=True), lambda pg: pg.scipy_sparse_to_backend(M)


def f32_row_accumulation(op, X):
    """The product with every row sum kept in f32: what the f32 multi-seed pass stores (exact f64 products, f32 running sums)."""
    X = np.asarray(X, dtype=np.float64)
    out = np.zeros((op.n, X.shape[1]))
    counts = np.diff(op.MT.indptr)
    rows = np.flatnonzero(counts > 0)
    for j in range(X.shape[1]):
        prods = (op.MT.data * X[op.MT.indices, j]).astype(fc.F32)
        out[rows, j] = np.add.reduceat(prods, op.MT.indptr[:-1][rows], dtype=fc.F32)
    return out
