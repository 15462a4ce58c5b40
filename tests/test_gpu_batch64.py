"""The f64 multi-seed loops (include/pgh_batch64.h, pygrank_amd/csrc/pgh_spmm64.hip) on the MI355X.

1. The product pgh_spmm_f64 is held to f64 row by row against a long-double product of the operator the kernels multiply by
   (batch64_common: |err| <= (nnz_row + 4) 2^-53 sum |m_ij x_ij|, every term derived), on a graph smaller than one tile, on hub rows
   whose carries chain over eleven tiles, on RMAT, value-free and valued, at every lane shape; a repeat returns the same bits.
2. Every golden case whose tolerance lies below fp32 eps runs through ``propagate(f64_batch=True)`` with the reference's iteration
   count, at widths 1, 5, 64 and 65.
3. Columns stop on their own: each has the iterations of the single-vector f64 rank() and of the f64 oracle and values within one f32
   ulp of the single-vector run (both round an f64 value that agrees far below half an ulp), without any "one iteration apart"
   allowance -- the seeds are chosen so that the oracle's residual at the stopping check and at the one before stay clear of tol.
4. The other stopping rules and options, the column that cannot converge, and what the f64 batch does not serve."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import batch64_common as bc
import cases
import f64_common as fc
from oracle import ref_loops as orc
from oracle import rmat_np
from parity_common import build_ranker, rel_linf, runs_in_f64, tolerance_for

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
F64_CASES = [c for c in cases.CASES if c[2] in ("pagerank", "heat", "generic", "pagerank_closed", "absorbing", "sarw")
             and c[3].get("coefficient_type", "taylor") == "taylor" and runs_in_f64(c[2], c[3])]
CASE_WIDTHS = (1, 5, 64, 65)


@pytest.fixture(scope="module")
def pg():
    import pygrank_amd
    from pygrank_amd import _lib
    pygrank_amd.load_backend("hip")
    assert _lib.runtime_name().startswith("hip:")
    assert all(_lib.entry(name) is not None for name in _lib.BATCH64_SIGNATURES)
    return pygrank_amd


@pytest.fixture(scope="module")
def golden_vectors():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden.npz"))


def _spmm(g, X, b=None, out=None):
    """(status, Y) of pgh_spmm_f64 on the host doubles X [n, b]"""
    from pygrank_amd import _lib as L
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.full(X.shape, SENTINEL) if out is None else out
    status = L.entry("pgh_spmm_f64")(g._h, X.ctypes.data_as(C.c_void_p), X.shape[1] if b is None else b, Y.ctypes.data_as(C.c_void_p))
    return status, Y


# ------------------------------------------------------------------------------------------------------------------ 1. the product
def _product_graphs():
    """name -> (W, normalisation kind): (a) less than one tile, (b) the hub graph four ways, (c) RMAT"""
    rng = np.random.default_rng(64)
    hub_mult, hub_real = bc.hub_graph(rng, weights="mult")[0], bc.hub_graph(rng, weights="real")[0]
    rmat = sp.csr_array(rmat_np.rmat_csr(12, 8))
    return {"small50/col": (bc.small_graph(rng), "col"), "hub/col": (hub_mult, "col"), "hub/symmetric": (hub_mult, "symmetric"),
            "hub/col-valued": (hub_real, "col-valued"), "hub/symmetric-valued": (hub_real, "symmetric-valued"),
            "rmat12/col-valued": (rmat, "col-valued"), "rmat12/symmetric-valued": (rmat, "symmetric-valued")}


PRODUCT_GRAPHS = ["small50/col", "hub/col", "hub/symmetric", "hub/col-valued", "hub/symmetric-valued", "rmat12/col-valued",
                  "rmat12/symmetric-valued"]


@pytest.fixture(scope="module")
def product_graphs():
    return _product_graphs()


@pytest.mark.parametrize("name", PRODUCT_GRAPHS)
def test_product_is_held_to_f64_row_by_row(pg, product_graphs, name):
    W, kind = product_graphs[name]
    op, upload = bc.operator_of(W, kind)
    g = upload(pg)
    n = W.shape[0]
    rng = np.random.default_rng(len(name))
    if name.startswith("hub"):
        assert op.nnz_row.max() >= 6000 and (op.nnz_row == 0).sum() >= 400      # >= 11 tiles of one row; empty rows
    worst = 0.0
    for b in bc.WIDTHS:
        X = bc.draw_x(rng, n, b)
        status, Y = _spmm(g, X)
        assert status == 0, (name, b, status)
        ratio, zeros = bc.product_ratio(Y, op, X)
        print("pgh_spmm_f64 %s b=%d worst |err| / bound = %.3f" % (name, b, ratio))
        assert zeros, (name, b)                                   # empty rows and the zero column: exactly zero
        assert ratio <= 1.0, (name, b, ratio)
        worst = max(worst, ratio)
        status, again = _spmm(g, X)
        assert status == 0 and np.array_equal(Y.view(np.uint64), again.view(np.uint64)), (name, b)
    assert worst > 0.0                                            # (a result equal to the long-double reference would be no f64 product)


def test_product_refusals_and_declines(pg):
    from pygrank_amd import _lib as L
    rng = np.random.default_rng(3)
    W = bc.small_graph(rng)
    _, upload = bc.operator_of(W, "col")
    g = upload(pg)
    X = bc.draw_x(rng, 50, 3)
    entry = L.entry("pgh_spmm_f64")
    Y = np.full((50, 3), SENTINEL)
    for width in (0, 65, -1):
        assert entry(g._h, X.ctypes.data_as(C.c_void_p), width, Y.ctypes.data_as(C.c_void_p)) not in (0, L.DECLINED), width
    assert entry(g._h, None, 3, Y.ctypes.data_as(C.c_void_p)) not in (0, L.DECLINED)
    assert entry(g._h, X.ctypes.data_as(C.c_void_p), 3, None) not in (0, L.DECLINED)
    assert entry(None, X.ctypes.data_as(C.c_void_p), 3, Y.ctypes.data_as(C.c_void_p)) not in (0, L.DECLINED)
    assert np.all(Y == SENTINEL)
    # declined, nothing written: a graph without the blocked layout, a graph without entries, a matrix that is not square
    with fc.layout_env(PGH_FORMAT="csr"):
        row_major = upload(pg)
    assert "row-major" in row_major.format()
    from pygrank_amd.device import DeviceGraph, DeviceMatrix
    empty = pg.scipy_sparse_to_backend(sp.csr_array((6, 6), dtype=np.float64))
    wide = DeviceGraph.from_factored(sp.csr_array((np.ones(3), ([0, 1, 4], [1, 2, 6])), shape=(5, 7)))
    for graph in (row_major, empty, wide):
        assert _spmm(graph, X, out=Y)[0] == L.DECLINED and np.all(Y == SENTINEL)
        assert L.lib().pgh_last_error()
    # ... and the loops decline and refuse alike
    P, R = DeviceMatrix.from_host(np.abs(X)), DeviceMatrix.from_host(np.full((50, 3), SENTINEL))
    cfg = L.LoopCfg(alpha=0.85, use_quotient=1, err_kind=L.ERR_L1, tol=1e-10, max_iters=50, end_modulo=1, out_scale=1.0, in_norm=1.0,
                    start_from_p=1, reserved=0)
    results, ones = (L.LoopResult * 3)(), (C.c_double * 3)(1.0, 1.0, 1.0)
    norms = (C.c_double * 3)(*np.abs(X).sum(axis=0))
    ppr, poly = L.entry("pgh_ppr_run_batch_f64"), L.entry("pgh_poly_run_batch_f64")
    coeffs = np.array([1.0, 0.5, 0.25])
    for graph in (row_major, empty, wide):
        assert ppr(graph._h, P._h, R._h, C.byref(cfg), ones, results, norms) == L.DECLINED
        assert poly(graph._h, P._h, coeffs.ctypes.data_as(C.c_void_p), 3, R._h, C.byref(cfg), ones, results) == L.DECLINED
    assert np.all(R.numpy() == SENTINEL)
    assert ppr(g._h, P._h, R._h, C.byref(cfg), ones, results, None) not in (0, L.DECLINED)                 # null norms
    short = DeviceMatrix.from_host(np.zeros((50, 2)))
    assert ppr(g._h, P._h, short._h, C.byref(cfg), ones, results, norms) not in (0, L.DECLINED)            # shape mismatch
    bad = L.LoopCfg.from_buffer_copy(cfg)
    bad.alpha = float("nan")
    assert ppr(g._h, P._h, R._h, C.byref(bad), ones, results, norms) not in (0, L.DECLINED)                # a non-finite alpha
    coeffs[1] = float("inf")
    assert poly(g._h, P._h, coeffs.ctypes.data_as(C.c_void_p), 3, R._h, C.byref(cfg), ones, results) not in (0, L.DECLINED)
    assert np.all(R.numpy() == SENTINEL)


# ------------------------------------------------------------------------------------------------------------------ 2. golden cases
@pytest.fixture(scope="module")
def small_graphs():
    built = {}

    def get(key):
        if key not in built:
            built[key] = cases.GRAPHS[key]()
        return built[key]
    return get


def _column_factors(b):
    """c_j = a power of two (the normalised personalization of c_j p is that of p, bit for bit); column 2 is a zero column"""
    c = np.array([2.0 ** ((j % 5) - 2) for j in range(b)])
    if b > 2:
        c[2] = 0.0
    return c


def _call_kwargs(kwargs, n):
    return {"absorption": cases.absorption_vector(kwargs["_absorption"], n)} if kwargs.get("_absorption") is not None else {}


def _records(ranker):
    return [c for batch in ranker.last_batches for c in batch]


@pytest.mark.parametrize("b", CASE_WIDTHS)
@pytest.mark.parametrize("name,gkey,algo,kwargs", F64_CASES, ids=[c[0] for c in F64_CASES])
def test_golden_cases_through_the_f64_batch(pg, small_graphs, golden_vectors, name, gkey, algo, kwargs, b):
    A, directed, p = small_graphs(gkey)
    n = A.shape[0]
    want, want_iters = golden_vectors[name + "|ranks"], int(golden_vectors[name + "|iters"])
    c = _column_factors(b)
    ranker = build_ranker(pg, algo, dict(kwargs, f64_batch=True))
    out = np.asarray(ranker.propagate(pg.AdjacencyWrapper(A, directed=directed), pg.to_primitive(np.outer(p, c)), **_call_kwargs(kwargs, n)),
                     dtype=np.float64)
    assert out.shape == (n, b)
    assert hasattr(ranker, "last_batches") and [len(batch) for batch in ranker.last_batches] == ([64, 1] if b > 64 else [b])
    records = _records(ranker)
    assert all(r["f64"] is True for r in records)
    scale = 1.0 if kwargs.get("preserve_norm", True) else 0.0
    for j in range(b):
        if c[j] == 0:                                             # (a recursive loop is told the norms and leaves such a column out)
            assert np.all(out[:, j] == 0) and (records[j]["iterations"] == 0 or algo not in ("pagerank", "absorbing", "sarw")), j
            continue
        assert records[j]["iterations"] == want_iters, (j, records[j]["iterations"], want_iters)
        assert rel_linf(out[:, j], want * c[j] ** scale) <= tolerance_for(kwargs), j


# ------------------------------------------------------------------------------------------------------------------ 3. own stops
TOL = 1e-10
SIZES = [1, 2000, 40, 5, 300]


def _filters(pg, pre):
    rule = dict(preprocessor=pre, error_type=pg.L1, tol=TOL, max_iters=2000)
    return {
        "pagerank": (lambda **kw: pg.PageRank(0.85, **rule, **kw), lambda M, p, **kw: orc.pagerank(M, p, alpha=0.85, **kw)),
        "absorbing": (lambda **kw: pg.AbsorbingWalks(**rule, **kw), lambda M, p, **kw: orc.absorbing_walks(M, p, **kw)),
        "heat": (lambda **kw: pg.HeatKernel(5, **rule, **kw), lambda M, p, **kw: orc.heat_kernel(M, p, t=5, **kw)),
    }


def _clear_stop(oracle, M, p):
    """(iterations, clear): the f64 oracle's stopping iteration, and whether its L1 residual at the stopping check and at the check
    before each lie at least 1e-6 tol away from tol"""
    _, it = oracle(M, p, error_type="l1", tol=TOL, max_iters=2000)
    after = lambda m: oracle(M, p, error_type="iters", max_iters=m, preserve_norm=False)[0]      # noqa: E731
    x2, x1, x0 = after(it), after(it - 1), after(it - 2)
    at_stop, before = np.abs(x2 - x1).sum(), np.abs(x1 - x0).sum()
    return it, (at_stop <= TOL and before > TOL and min(abs(at_stop - TOL), abs(before - TOL)) >= 1e-6 * TOL)


@pytest.mark.parametrize("which", ["pagerank", "absorbing", "heat"])
def test_columns_stop_on_their_own(pg, which):
    A = rmat_np.rmat_csr(12, 8, seed=5)
    n = A.shape[0]
    Mn = sp.csr_array(orc.normalize(A, "col", True))
    graph = pg.AdjacencyWrapper(A, directed=True)
    make, oracle = _filters(pg, pg.preprocessor(assume_immutability=True))[which]
    feats, want_iters = np.zeros((n, 5)), []
    for j, size in enumerate(SIZES):
        for seed in range(j + 1, j + 40, 5):                      # the first seed set whose stop is clear of the tolerance
            column = np.zeros(n)
            column[rmat_np.seed_nodes(A, size, seed=seed)] = 1.0 + j
            it, clear = _clear_stop(oracle, Mn, column)
            if clear:
                break
        assert clear, (which, j)                                  # the premise of "no iteration apart"
        feats[:, j] = column
        want_iters.append(it)
    ranker = make(f64_batch=True)
    out = np.asarray(ranker.propagate(graph, pg.to_primitive(feats)), dtype=np.float64)
    records = _records(ranker)
    assert len(records) == 5 and all(r["f64"] is True and r["converged"] for r in records)
    assert which == "heat" or len(set(want_iters)) > 1            # the recursive filters' columns do stop at different iterations
    for j in range(5):
        single = make()
        got1 = np.asarray(single.rank(graph, feats[:, j].copy()).np, dtype=np.float64)
        assert single.convergence.iteration == want_iters[j], (j, single.convergence.iteration, want_iters[j])
        assert records[j]["iterations"] == want_iters[j], (j, records[j]["iterations"], want_iters[j])
        ulp = np.spacing(np.maximum(np.abs(out[:, j]), np.abs(got1)).astype(np.float32)).astype(np.float64)
        worst = float(np.max(np.abs(out[:, j] - got1) / ulp))
        print("%s column %d: %d iterations, worst difference from the single-vector run %.2f f32 ulp" % (which, j, want_iters[j], worst))
        assert np.all(np.abs(out[:, j] - got1) <= ulp), (j, worst)


# ------------------------------------------------------------------------------------------------------------------ 4. rules and options
def _one_ulp(a, b):
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    return bool(np.all(np.abs(a - b) <= ulp))


OPTIONS = {
    "mabs": dict(error_type="mabs", tol=1e-12),
    "linf": dict(error_type="linf", tol=1e-10),
    "iters": dict(error_type="iters", max_iters=17),
    "noquot": dict(use_quotient=False, tol=1e-10),
    "nonorm": dict(preserve_norm=False, tol=1e-10),
    "modulo": dict(end_modulo=3, tol=1e-10),
}


# (the closed-form filters have no quotient)
OPTION_CASES = [(algo, option) for algo in ("pagerank", "absorbing", "sarw", "heat") for option in OPTIONS if (algo, option) != ("heat", "noquot")]


@pytest.mark.parametrize("algo,option", OPTION_CASES, ids=["%s-%s" % c for c in OPTION_CASES])
def test_rules_and_options_match_the_column_loop(pg, small_graphs, algo, option):
    kwargs = dict(OPTIONS[option])
    kwargs.setdefault("max_iters", 2000)
    if algo == "heat":
        kwargs["t"] = 3
    if algo in ("pagerank", "absorbing"):
        kwargs["alpha"] = 0.85
    if option == "iters" or algo == "pagerank":
        # counting mode asks for f64 by dtype: no tolerance to go by; and PageRank's propagate keeps its f32 multi-seed loop below
        # fp32 eps unless the ranker promises f64 iterates: only then is today's route the column loop this test compares with
        kwargs["dtype"] = "float64"
    A, directed, p = small_graphs("rmat10_dir")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    rng = np.random.default_rng(7)
    F = np.outer(p, [1.0, 4.0, 0.0]) + np.where(rng.random((A.shape[0], 3)) < 0.01, 1.0, 0.0) * [1.0, 0.0, 0.0]
    on, off = build_ranker(pg, algo, dict(kwargs, f64_batch=True)), build_ranker(pg, algo, kwargs)
    assert on._f64_wanted()
    got = np.asarray(on.propagate(graph, pg.to_primitive(F)), dtype=np.float64)
    records = _records(on)
    assert len(records) == 3 and all(r["f64"] is True for r in records)
    assert not got[:, 2].any() and (records[2]["iterations"] == 0 or algo == "heat")
    for j in range(2):
        single = build_ranker(pg, algo, kwargs)
        want = np.asarray(single.rank(graph, F[:, j].copy()).np, dtype=np.float64)
        assert records[j]["iterations"] == single.convergence.iteration, (j, records[j]["iterations"], single.convergence.iteration)
        assert _one_ulp(got[:, j], want), j
    want = np.asarray(off.propagate(graph, pg.to_primitive(F)), dtype=np.float64)      # today's column loop as a whole
    assert not hasattr(off, "last_batches") and _one_ulp(got, want)


@pytest.mark.parametrize("make", [lambda pg, **kw: pg.HeatKernel(5, error_type=pg.L1, tol=1e-12, max_iters=4, **kw),
                                  lambda pg, **kw: pg.AbsorbingWalks(0.85, error_type=pg.L1, tol=1e-12, max_iters=3, **kw),
                                  lambda pg, **kw: pg.PageRank(0.85, error_type=pg.L1, tol=1e-12, max_iters=3, **kw)],
                         ids=["heat", "absorbing", "pagerank"])
def test_non_converging_column_raises_like_the_column_loop(pg, small_graphs, make):
    A, directed, p = small_graphs("rmat10_dir")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    X = pg.to_primitive(np.outer(p, [1.0, 0.0]))
    caught = []
    for kw in (dict(f64_batch=True), dict()):
        r = make(pg, **kw)
        with pytest.raises(Exception) as info:
            r.propagate(graph, X)
        caught.append(str(info.value))
    assert caught[0] == caught[1] and "converge" in caught[0]


def test_retire_takes_the_plain_f64_batch_and_dropout_todays_route(pg, small_graphs):
    A, directed, p = small_graphs("rmat10_dir")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    F = pg.to_primitive(np.outer(p, [1.0, 2.0, 3.0]))
    rule = dict(tol=1e-10, max_iters=2000)
    plain, retiring = pg.PageRank(0.85, f64_batch=True, **rule), pg.PageRank(0.85, f64_batch=True, retire=True, **rule)
    a, b = np.asarray(plain.propagate(graph, F)), np.asarray(retiring.propagate(graph, F))
    assert np.array_equal(a, b)
    assert all(r["f64"] is True and "stages" not in r for r in _records(retiring))
    # graph_dropout: the f32 multi-seed loop with its masks, as without f64_batch (a fresh mask per step: no tolerance is met)
    for kw in (dict(f64_batch=True), dict()):
        dropped = pg.PageRank(0.85, tol=1e-10, max_iters=6, **kw)
        assert dropped._f64_wanted()
        with pytest.raises(Exception):
            dropped.propagate(graph, F, graph_dropout=0.25)
        assert len(_records(dropped)) == 3 and all("f64" not in r for r in _records(dropped))
