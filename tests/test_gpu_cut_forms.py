"""pgh_mat_col_stats and pgh_cut_forms (include/pgh_measure.h) on the GPU against numpy in f64 on the SAME f32 inputs.

The reference forms s = f32(score * f32(factor)) and c = f32(f32(max_rank) - s) with f32 rounding as the header specifies, takes
N = M^T s and C = M^T c in f64 from the graph's downloaded CSR(M^T), and the four forms in f64.  Scores lie in [0, max_rank], so every
form is a sum of non-negative terms and a relative bound is meaningful: 4 * 2^-24 per form covers one f32 rounding of each entry of
N and C (what pgh_spmm stores) plus the f64 summation.  A form whose reference is 0 must be 0.  Sum and sum of squares of
pgh_mat_col_stats are held to 1e-12 relative (f64 accumulation of f32 values), max and min exactly.

Shapes: n = 3 (less than one workgroup's rows), 257 (just past 256), 300, 1024, 20 037 (odd, many parts) and a 40 000-node dense graph
(sources beyond the 29 696-slot hot cache); b = 1, 3 (padding columns), 5, 32, 33 (the 32-column chunk boundary), 64."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

FORM_TOL = 4 * 2.0 ** -24
SENTINEL = -7.25


def _random_graph(n, in_degree, seed, weighted):
    """Directed, about `in_degree` edges per node, every 7th node without out-edges; unit weights with duplicates summed (small
    integers: the value-free image) or real weights (the valued image)."""
    rng = np.random.default_rng(seed)
    m = n * in_degree
    rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = rows % 7 != 3
    w = rng.random(m) + 0.1 if weighted else np.ones(m)
    A = sp.coo_array((w[keep], (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def _build(key):
    import cases
    if key in ("rmat10_dir", "weighted300"):
        return cases.GRAPHS[key]()[0]
    if key == "tiny3":
        return sp.csr_array(np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]]))
    if key == "n257":
        return _random_graph(257, 8, 11, weighted=True)
    if key == "n20037":
        return _random_graph(20037, 8, 12, weighted=False)
    if key == "dense40k":
        return _random_graph(40000, 64, 13, weighted=False)
    raise KeyError(key)


@pytest.fixture(scope="module")
def graphs(gpu_engine):
    from pygrank_amd.device import DeviceGraph
    cache = {}

    def get(key):
        if key not in cache:
            g = DeviceGraph.from_adjacency(_build(key), "none")
            cache[key] = (g, sp.csr_array(g.download_transposed().astype(np.float64)))
        return cache[key]
    return get


def _scores(n, b, max_rank, seed):
    """[n, b] f32 scores and f64 factors with scores * factor in [0, max_rank]: column j % 5 == 1 all zero, j % 5 == 2 equal to
    max_rank everywhere (c == 0), the others random with a factor in [0.5, 1)."""
    rng = np.random.default_rng(seed)
    S = (rng.random((n, b)) * max_rank).astype(np.float32)
    factors = 0.5 + 0.5 * rng.random(b)
    for j in range(b):
        if j % 5 == 1:
            S[:, j] = 0
        if j % 5 == 2:
            S[:, j] = max_rank
            factors[j] = 1.0
    return S, factors


def _call(L, g, mat, factors, max_rank, forms):
    b = mat.b
    out = np.full(4 * b + 4, SENTINEL)
    status = L.entry("pgh_cut_forms")(g._h, mat._h, None if factors is None else factors.ctypes.data_as(C.c_void_p), float(max_rank),
                                      forms, out.ctypes.data_as(C.c_void_p))
    return status, out


def _reference(MT, S, factors, max_rank):
    f = np.ones(S.shape[1], dtype=np.float32) if factors is None else factors.astype(np.float32)
    s32 = (S * f[None, :]).astype(np.float32)                # one f32 product
    c32 = (np.float32(max_rank) - s32).astype(np.float32)    # one f32 difference
    s, c = s32.astype(np.float64), c32.astype(np.float64)
    N, Cc = MT @ s, MT @ c
    return np.stack([(N * s).sum(0), (N * c).sum(0), (Cc * s).sum(0), (Cc * c).sum(0)], axis=1)


CASES = [(key, b) for key in ("rmat10_dir", "weighted300") for b in (1, 3, 5, 32, 33, 64)] + \
        [("tiny3", 1), ("tiny3", 5), ("tiny3", 64), ("n257", 3), ("n257", 33), ("n20037", 5), ("n20037", 64), ("dense40k", 33)]


@pytest.mark.parametrize("key,b", CASES)
def test_cut_forms_and_col_stats_against_numpy(gpu_engine, graphs, key, b):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix
    g, MT = graphs(key)
    n = g.shape[0]
    max_rank = 2 if b % 2 else 1
    S, factors = _scores(n, b, max_rank, seed=1000 + b)
    if b == 3:
        factors = None                                       # NULL: all ones
    mat = DeviceMatrix.from_host(S)
    assert np.array_equal(mat.numpy().astype(np.float32), S)

    # ---- column statistics
    stats = np.full(4 * b + 4, SENTINEL)
    L.check(L.entry("pgh_mat_col_stats")(mat._h, stats.ctypes.data_as(C.c_void_p)))
    assert np.all(stats[4 * b:] == SENTINEL)
    stats = stats[:4 * b].reshape(b, 4)
    S64 = S.astype(np.float64)
    want_sum, want_sq = S64.sum(0), (S64 * S64).sum(0)
    print(f"{key} b={b}: col_stats sum err {np.max(np.abs(stats[:, 0] - want_sum) / np.maximum(want_sum, 1e-300)):.2e}, "
          f"sumsq err {np.max(np.abs(stats[:, 1] - want_sq) / np.maximum(want_sq, 1e-300)):.2e}")
    assert np.all(np.abs(stats[:, 0] - want_sum) <= 1e-12 * want_sum)
    assert np.all(np.abs(stats[:, 1] - want_sq) <= 1e-12 * want_sq)
    assert np.array_equal(stats[:, 2], S64.max(0)) and np.array_equal(stats[:, 3], S64.min(0))

    # ---- all four forms
    want = _reference(MT, S, factors, max_rank)
    status, out = _call(L, g, mat, factors, max_rank, L.CUT_ALL)
    assert status == 0, L.lib().pgh_last_error()
    assert np.all(out[4 * b:] == SENTINEL)
    got = out[:4 * b].reshape(b, 4)
    err = np.abs(got - want) / np.where(want != 0, want, 1.0)
    print(f"{key} b={b} max_rank={max_rank}: largest relative form error {err.max():.3e} (bound {FORM_TOL:.3e})")
    assert np.all(got[want == 0] == 0)
    assert np.all(np.abs(got - want) <= FORM_TOL * want), (key, b, float(err.max()))
    for j in range(b):
        if j % 5 == 1:
            assert got[j, 0] == 0 and got[j, 1] == 0 and got[j, 2] == 0           # s == 0
        if j % 5 == 2:
            assert got[j, 1] == 0 and got[j, 2] == 0 and got[j, 3] == 0           # c == 0
    status, again = _call(L, g, mat, factors, max_rank, L.CUT_ALL)
    assert status == 0 and np.array_equal(out, again)        # bit for bit

    # ---- PGH_CUT_INTERNAL: <N, s> only, zeros in the other slots
    status, inner = _call(L, g, mat, factors, max_rank, L.CUT_INTERNAL)
    assert status == 0 and np.all(inner[4 * b:] == SENTINEL)
    inner = inner[:4 * b].reshape(b, 4)
    assert np.all(inner[:, 1:] == 0)
    assert np.all(np.abs(inner[:, 0] - want[:, 0]) <= FORM_TOL * want[:, 0])
    assert np.all(inner[want[:, 0] == 0, 0] == 0)
    status, inner_again = _call(L, g, mat, factors, max_rank, L.CUT_INTERNAL)
    assert status == 0 and np.array_equal(inner_again[:4 * b].reshape(b, 4), inner)


def test_cut_forms_refusals_leave_the_output_alone(gpu_engine, graphs):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceGraph, DeviceMatrix
    g, _ = graphs("rmat10_dir")
    n = g.shape[0]
    rng = np.random.default_rng(5)

    def untouched(status, out, declined=True):
        assert (status == L.DECLINED) if declined else (status not in (0, L.DECLINED)), status
        assert np.all(out == SENTINEL)
    wide = DeviceMatrix.from_host(rng.random((n, 65)))
    untouched(*_call(L, g, wide, None, 1, L.CUT_ALL))
    untouched(*_call(L, g, wide, None, 1, L.CUT_INTERNAL))
    mat = DeviceMatrix.from_host(rng.random((n, 4)))
    bad = np.array([1.0, np.nan, 1.0, 1.0])
    untouched(*_call(L, g, mat, bad, 1, L.CUT_ALL))
    untouched(*_call(L, g, mat, np.array([1.0, 1.0, np.inf, 1.0]), 1, L.CUT_ALL))
    untouched(*_call(L, g, mat, None, float("nan"), L.CUT_ALL))
    untouched(*_call(L, g, mat, None, float("inf"), L.CUT_INTERNAL))
    rect = DeviceGraph.from_scipy(sp.random(300, 200, density=0.05, random_state=3, format="csr"))
    untouched(*_call(L, rect, DeviceMatrix.from_host(rng.random((200, 4))), None, 1, L.CUT_ALL))
    untouched(*_call(L, rect, DeviceMatrix.from_host(rng.random((300, 4))), None, 1, L.CUT_ALL))
    # a shape mismatch is an error, not a decline
    untouched(*_call(L, g, DeviceMatrix.from_host(rng.random((n + 1, 4))), None, 1, L.CUT_ALL), declined=False)
    status, out = _call(L, g, mat, None, 1, 7)               # unknown forms
    untouched(status, out, declined=False)
    # and the entry still serves the next request
    status, out = _call(L, g, mat, None, 1, L.CUT_ALL)
    assert status == 0 and np.all(out[:16] != SENTINEL)
