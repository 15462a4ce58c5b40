"""Multi-seed device loops of the closed-form filters and the absorbing walks (include/pgh_batch.h: pgh_poly_run_batch,
pgh_absorb_run_batch, pgh_sarw_run_batch) behind ``propagate`` (signals.py:225-226: one rank() per feature column).

Every column must equal the single-vector fused run of that column -- the oracle at the engine's fp32 epsilon with its iteration
count -- and the configurations a single rank() would not run on the f32 fused loop must keep the column loop."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cases
from oracle import ref_loops as orc
from oracle import rmat_np
from parity_common import EPS32, build_ranker, rel_linf, run_oracle, runs_in_f64, tolerance_for

pytestmark = pytest.mark.gpu

BATCH_ALGOS = ("heat", "generic", "pagerank_closed", "absorbing", "sarw")
# the batch route: taylor form, a tolerance the f32 loop honours
BATCH_CASES = [c for c in cases.CASES if c[2] in BATCH_ALGOS and c[3].get("coefficient_type", "taylor") == "taylor"
               and not runs_in_f64(c[2], c[3])]
# cases whose tolerance lies below fp32 eps, run again at tol = 1e-6 (absorbing_custom also covers absorption=)
BATCH_CASES += [(name + "@1e-6", gkey, algo, dict(kwargs, tol=1e-6)) for name, gkey, algo, kwargs in cases.CASES
                if name in ("rmat10/generic20", "rmat10/pagerank_closed", "rmat10/absorbing_custom")]
F64_CASES = [c for c in cases.CASES if c[2] in BATCH_ALGOS and c[3].get("coefficient_type", "taylor") == "taylor"
             and runs_in_f64(c[2], c[3])]
WIDTHS = (1, 5, 64, 65)


@pytest.fixture(scope="module")
def pg():
    import pygrank_amd
    from pygrank_amd import _lib
    pygrank_amd.load_backend("hip")
    assert _lib.runtime_name().startswith("hip:")
    assert _lib.entry("pgh_poly_run_batch") is not None
    return pygrank_amd


@pytest.fixture(scope="module")
def golden_vectors():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden.npz"))


@pytest.fixture(scope="module")
def small_graphs():
    built = {}

    def get(key):
        if key not in built:
            built[key] = cases.GRAPHS[key]()
        return built[key]
    return get


def _column_factors(b):
    """c_j = a power of two (the normalised personalization of c_j p is that of p, bit for bit); column 2 (or the only one) ..."""
    c = np.array([2.0 ** ((j % 5) - 2) for j in range(b)])
    if b > 2:
        c[2] = 0.0                                         # ... a zero column, which must stay zero
    return c


def _call_kwargs(kwargs, n):
    return {"absorption": cases.absorption_vector(kwargs["_absorption"], n)} if kwargs.get("_absorption") is not None else {}


def _iterations(ranker):
    return [c["iterations"] for batch in ranker.last_batches for c in batch]


@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("name,gkey,algo,kwargs", BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
def test_golden_cases_through_the_batch_route(pg, small_graphs, name, gkey, algo, kwargs, b):
    A, directed, p = small_graphs(gkey)
    n = A.shape[0]
    want, want_iters = run_oracle(A, directed, p, algo, kwargs, eps=EPS32)
    c = _column_factors(b)
    F = np.outer(p, c)
    ranker = build_ranker(pg, algo, kwargs)
    out = np.asarray(ranker.propagate(pg.AdjacencyWrapper(A, directed=directed), pg.to_primitive(F), **_call_kwargs(kwargs, n)),
                     dtype=np.float64)
    assert out.shape == (n, b)
    assert hasattr(ranker, "last_batches") and len(ranker.last_batches) == (2 if b > 64 else 1)
    iters = _iterations(ranker)
    for j in range(b):
        if c[j] == 0:
            assert np.all(out[:, j] == 0), j
            continue
        assert iters[j] == want_iters, (j, iters[j], want_iters)
        assert rel_linf(out[:, j], c[j] * want) <= tolerance_for(kwargs), j


def _stop_margin_ok(run_iters, M, p, stop, tol):
    """An iteration apart is accepted only when the oracle's own L1 change at the engine's stopping check lies within f32 rounding
    (2 %) of the tolerance (kernel_checks.py, batched PageRank).  run_iters(max_iters) -> the oracle's ranks after that many."""
    at_stop, before = run_iters(stop), run_iters(stop - 1)
    residual = np.abs(at_stop - before).sum() / np.abs(p).sum()
    return abs(residual - tol) <= 0.02 * tol, at_stop


@pytest.mark.parametrize("which", ["heat", "absorbing"])
def test_columns_stop_at_their_own_iteration(pg, which):
    """Distinct seed sets on a directed RMAT graph: each column equals the single-vector rank() of that column."""
    A = rmat_np.rmat_csr(12, 8, seed=5)
    n = A.shape[0]
    Mn = sp.csr_array(orc.normalize(A, "col", True))
    graph = pg.AdjacencyWrapper(A, directed=True)
    pre = pg.preprocessor(assume_immutability=True)
    feats = np.zeros((n, 5))
    for j in range(5):
        feats[rmat_np.seed_nodes(A, [1, 2000, 40, 5, 300][j], seed=j + 1), j] = 1.0 + j

    def make():
        if which == "heat":
            return pg.HeatKernel(5, preprocessor=pre, error_type=pg.L1, tol=1e-6, max_iters=500)
        return pg.AbsorbingWalks(0.85, preprocessor=pre, error_type=pg.L1, tol=1e-6, max_iters=500)

    def oracle(p, **kw):
        if which == "heat":
            return orc.heat_kernel(Mn, p, t=5, eps=EPS32, **kw)
        return orc.absorbing_walks(Mn, p, alpha=0.85, eps=EPS32, **kw)
    ranker = make()
    out = np.asarray(ranker.propagate(graph, pg.to_primitive(feats)), dtype=np.float64)
    iters = _iterations(ranker)
    for j in range(5):
        single = make()
        got1 = np.asarray(single.rank(graph, feats[:, j].copy()).np, dtype=np.float64)
        it1 = single.convergence.iteration
        want, it = oracle(feats[:, j], error_type="l1", tol=1e-6, max_iters=500)
        assert it1 == it, (j, it1, it)
        if iters[j] != it:
            assert abs(iters[j] - it) == 1, (j, iters[j], it)
            ok, want = _stop_margin_ok(lambda m: oracle(feats[:, j], error_type="iters", max_iters=m)[0], Mn, feats[:, j], iters[j], 1e-6)
            assert ok, (j, iters[j], it)
        else:
            assert rel_linf(out[:, j], got1) <= 1e-6, j
        assert rel_linf(out[:, j], want) <= 1e-6, j
    if which == "absorbing":
        assert len(set(iters)) > 1, iters


def test_scale23_batch_of_64(pg):
    """HeatKernel t = 5 (default rule) and AbsorbingWalks (L1 1e-6) on RMAT scale 23 with 64 columns: sampled columns against the
    single-vector run and the oracle on the engine's own matrix; two runs of the same propagate are bit-identical."""
    from pygrank_amd.synthetic import rmat_graph
    adj = rmat_graph(23, 16, seed=0, normalization="col", a=0.57, b=0.19, c=0.19)
    g = adj.array
    M = sp.csr_array(g.download_transposed().T.astype(np.float64))
    deg = np.asarray(pg.degrees(g))
    cand = np.flatnonzero(deg > 0)
    n = g.shape[0]
    F = np.zeros((n, 64))
    for k in range(64):
        F[np.sort(np.random.default_rng(1 + k).choice(cand, 100, replace=False)), k] = 1.0
    X = pg.to_primitive(F)
    for make, oracle in ((lambda: pg.HeatKernel(5), lambda p, **kw: orc.heat_kernel(M, p, t=5, eps=EPS32, **kw)),
                         (lambda: pg.AbsorbingWalks(0.85, error_type=pg.L1, tol=1e-6, max_iters=1000),
                          lambda p, **kw: orc.absorbing_walks(M, p, alpha=0.85, eps=EPS32, error_type="l1", tol=1e-6, **kw))):
        ranker = make()
        out = np.asarray(ranker.propagate(adj, X), dtype=np.float64)
        iters = _iterations(ranker)
        again = np.asarray(ranker.propagate(adj, X), dtype=np.float64)
        assert np.array_equal(out, again)
        for j in (0, 31, 63):
            single = make()
            got1 = np.asarray(single.rank(adj, F[:, j].copy()).np, dtype=np.float64)
            want, it = oracle(F[:, j])
            assert single.convergence.iteration == it, (j, single.convergence.iteration, it)
            if iters[j] != it:
                # (only the walk's L1 rule has the margin check; the heat kernel's stops must agree)
                assert isinstance(single, pg.AbsorbingWalks) and abs(iters[j] - it) == 1, (j, iters[j], it)
                ok, want = _stop_margin_ok(
                    lambda m: orc.absorbing_walks(M, F[:, j], alpha=0.85, eps=EPS32, error_type="iters", max_iters=m)[0],
                    M, F[:, j], iters[j], 1e-6)
                assert ok, (j, iters[j], it)
            else:
                assert rel_linf(out[:, j], got1) <= 1e-6, j
            assert rel_linf(out[:, j], want) <= 1e-6, j


def _assert_column_loop(ranker, run):
    out = run()
    assert not hasattr(ranker, "last_batches")
    return np.asarray(out, dtype=np.float64)


def test_route_selection_keeps_the_column_loop(pg, small_graphs):
    A, directed, p = small_graphs("rmat10_dir")
    n = A.shape[0]
    graph = pg.AdjacencyWrapper(A, directed=directed)
    F = np.outer(p, [1.0, 0.5])
    X = pg.to_primitive(F)
    heat = dict(t=5, error_type="iters", max_iters=31)
    # f64 iterates asked for
    r = pg.HeatKernel(**heat, dtype="float64")
    out = _assert_column_loop(r, lambda: r.propagate(graph, X))
    want, _ = run_oracle(A, directed, p, "heat", heat)
    assert rel_linf(out[:, 0], want) <= 1e-6 and rel_linf(out[:, 1], 0.5 * want) <= 1e-6
    # the chebyshev form
    r = pg.HeatKernel(**heat, coefficient_type="chebyshev")
    out = _assert_column_loop(r, lambda: r.propagate(graph, X))
    want, _ = run_oracle(A, directed, p, "heat", dict(heat, coefficient_type="chebyshev"))
    assert rel_linf(out[:, 0], want) <= 1e-6
    # an optimisation dict
    r = pg.HeatKernel(**heat, optimization_dict={})
    out = _assert_column_loop(r, lambda: r.propagate(graph, X))
    want, _ = run_oracle(A, directed, p, "heat", heat, eps=EPS32)
    assert rel_linf(out[:, 0], want) <= 1e-6
    # graph_dropout > 0
    r = pg.HeatKernel(**heat)
    out = _assert_column_loop(r, lambda: r.propagate(graph, X, graph_dropout=0.1))
    assert out.shape == (n, 2) and np.all(np.isfinite(out))

    # overridden hooks and a convergence manager of another type
    class MyHeat(pg.HeatKernel):
        def _start(self, *args, **kwargs):
            super()._start(*args, **kwargs)

    class MyWalk(pg.AbsorbingWalks):
        def _formula(self, *args, **kwargs):
            return super()._formula(*args, **kwargs)

    class MyManager(pg.ConvergenceManager):
        pass
    walk = dict(alpha=0.85, max_iters=1000)
    want_w, _ = run_oracle(A, directed, p, "absorbing", walk, eps=EPS32)
    want_h, _ = run_oracle(A, directed, p, "heat", heat, eps=EPS32)
    for r, want in ((MyHeat(**heat), want_h), (MyWalk(**walk), want_w),
                    (pg.AbsorbingWalks(0.85, convergence=MyManager(max_iters=1000)), want_w)):
        out = _assert_column_loop(r, lambda: r.propagate(graph, X))
        assert rel_linf(out[:, 0], want) <= 1e-6, type(r).__name__
    # a personalization transform: the column loop's result
    r = pg.HeatKernel(**heat)
    r << pg.HeatKernel(t=2, error_type="iters", max_iters=5)
    out = _assert_column_loop(r, lambda: r.propagate(graph, X))
    ref = pg.HeatKernel(**heat)
    ref << pg.HeatKernel(t=2, error_type="iters", max_iters=5)
    assert rel_linf(out[:, 0], np.asarray(ref.rank(graph, p.copy()).np, dtype=np.float64)) <= 1e-6
    # a row-major graph (PGH_FORMAT=csr at upload)
    saved = os.environ.get("PGH_FORMAT")
    os.environ["PGH_FORMAT"] = "csr"
    try:
        rm = pg.AdjacencyWrapper(A, directed=directed)
        pre = pg.preprocessor(assume_immutability=True)
        assert "row-major" in pre(rm).array.format()
    finally:
        if saved is None:
            os.environ.pop("PGH_FORMAT", None)
        else:
            os.environ["PGH_FORMAT"] = saved
    for r in (pg.HeatKernel(**heat, preprocessor=pre), pg.SymmetricAbsorbingRandomWalks(max_iters=1000, preprocessor=pre)):
        out = _assert_column_loop(r, lambda: r.propagate(rm, X))
        algo, kw = ("heat", heat) if isinstance(r, pg.HeatKernel) else ("sarw", dict(max_iters=1000))
        want, _ = run_oracle(A, directed, p, algo, kw, eps=EPS32)
        assert rel_linf(out[:, 0], want) <= 1e-6


@pytest.mark.parametrize("name,gkey,algo,kwargs", F64_CASES, ids=[c[0] for c in F64_CASES])
def test_f64_cases_keep_the_column_loop(pg, small_graphs, golden_vectors, name, gkey, algo, kwargs):
    A, directed, p = small_graphs(gkey)
    ranker = build_ranker(pg, algo, kwargs)
    F = np.outer(p, [1.0, 2.0])
    out = _assert_column_loop(ranker, lambda: ranker.propagate(pg.AdjacencyWrapper(A, directed=directed), pg.to_primitive(F),
                                                               **_call_kwargs(kwargs, A.shape[0])))
    assert ranker.convergence.iteration == int(golden_vectors[name + "|iters"])
    assert rel_linf(out[:, 0], golden_vectors[name + "|ranks"]) <= tolerance_for(kwargs)
    assert rel_linf(out[:, 1], 2.0 * golden_vectors[name + "|ranks"]) <= tolerance_for(kwargs)


@pytest.mark.parametrize("make", [lambda pg: pg.HeatKernel(5, error_type=pg.L1, tol=1e-7, dtype="float32", max_iters=4),
                                  lambda pg: pg.AbsorbingWalks(0.85, error_type=pg.L1, tol=1e-7, dtype="float32", max_iters=3)],
                         ids=["heat", "absorbing"])
def test_non_converging_column_raises_like_the_column_loop(pg, small_graphs, make):
    from pygrank_amd.signals import NodeRanking
    A, directed, p = small_graphs("rmat10_dir")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    X = pg.to_primitive(np.outer(p, [1.0, 0.0]))
    caught = []
    for run in (lambda r: r.propagate(graph, X), lambda r: NodeRanking.propagate(r, graph, X)):
        r = make(pg)
        with pytest.raises(Exception) as info:
            run(r)
        caught.append((type(info.value), str(info.value)))
    assert caught[0] == caught[1]


def test_differentiable_propagate_heat_kernel(pg):
    """gnn.differentiable_propagate with HeatKernel(error_type="iters", max_iters=10) takes the batch route: forward output and gradient
    against the oracle (the same filter on the transposed matrix) on a directed and an undirected graph."""
    import torch
    from pygrank_amd.gnn import differentiable_propagate
    rng = np.random.default_rng(5)
    for gkey in ("rmat10_dir", "er10k"):
        A, directed, _ = cases.GRAPHS[gkey]()
        n = A.shape[0]
        M = sp.csr_array(orc.normalize(A, "auto", directed))
        graph = pg.AdjacencyWrapper(A, directed=directed)
        pre = pg.preprocessor(assume_immutability=True)
        ranker = pg.HeatKernel(3, preprocessor=pre, error_type="iters", max_iters=10)
        X = torch.tensor(rng.random((n, 3)) * (rng.random((n, 3)) < 0.05), dtype=torch.float32, requires_grad=True)
        W = torch.tensor(rng.random((n, 3)), dtype=torch.float32)
        Y = differentiable_propagate(ranker, graph, X)
        assert hasattr(ranker, "last_batches")
        (Y * W).sum().backward()
        Xn, Wn = X.detach().numpy().astype(np.float64), W.numpy().astype(np.float64)
        kw = dict(t=3, error_type="iters", max_iters=10)
        for j in range(3):
            want = orc.heat_kernel(M, Xn[:, j], **kw)[0] if Xn[:, j].any() else Xn[:, j]
            assert np.max(np.abs(Y.detach().numpy()[:, j] - want)) <= 2e-6 * max(np.max(np.abs(want)), 1e-30), (gkey, j)
            grad = orc.heat_kernel(sp.csr_array(M.T), Wn[:, j], **kw)[0]
            assert np.max(np.abs(X.grad.numpy()[:, j] - grad)) <= 2e-6 * np.max(np.abs(grad)), (gkey, j)
