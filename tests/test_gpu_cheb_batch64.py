"""The "chebyshev" form as an f64 multi-seed loop (include/pgh_cheb64.h, k_mm64_cheb_step in pygrank_amd/csrc/pgh_spmm64.hip) on the
MI355X: the golden cases through ``propagate(f64_batch=True)``, columns that stop on their own, the entry against the recurrence in
long double and the single-vector loop, the other rules, and what is declined, refused or left on the column loop."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import batch64_common as bc
import cases
import f64_common as fc
from oracle import ref_loops as orc
from oracle import rmat_np
from parity_common import build_ranker, rel_linf, tolerance_for
from test_gpu_batch64 import OPTIONS, SENTINEL, SIZES, _clear_stop, _column_factors, _one_ulp, _records, golden_vectors, pg, small_graphs  # noqa: F401

pytestmark = pytest.mark.gpu

CHEB_CASES = [c for c in cases.CASES if c[3].get("coefficient_type") == "chebyshev"]
SCHEDULE = np.array([1.0, 0.5, -0.75, 0.0, 0.25, 0.125])          # c_4 == 0: a zero coefficient after iteration 2


def _marked(ranker):
    return all(r["f64"] is True and r["form"] == "chebyshev" for r in _records(ranker))


@pytest.mark.parametrize("b", (1, 5, 64, 65))
@pytest.mark.parametrize("name,gkey,algo,kwargs", CHEB_CASES, ids=[c[0] for c in CHEB_CASES])
def test_golden_chebyshev_cases_through_the_f64_batch(pg, small_graphs, golden_vectors, name, gkey, algo, kwargs, b):
    A, directed, p = small_graphs(gkey)
    want, want_iters = golden_vectors[name + "|ranks"], int(golden_vectors[name + "|iters"])
    c = _column_factors(b)                                        # powers of two; column 2 is a zero column
    ranker = build_ranker(pg, algo, dict(kwargs, f64_batch=True))
    out = np.asarray(ranker.propagate(pg.AdjacencyWrapper(A, directed=directed), pg.to_primitive(np.outer(p, c))), dtype=np.float64)
    assert hasattr(ranker, "last_batches") and [len(batch) for batch in ranker.last_batches] == ([64, 1] if b > 64 else [b])
    assert out.shape == (A.shape[0], b) and _marked(ranker)
    for j, record in enumerate(_records(ranker)):
        if c[j] == 0:
            assert np.all(out[:, j] == 0), j
        else:
            assert record["iterations"] == want_iters and rel_linf(out[:, j], want * c[j]) <= tolerance_for(kwargs), (j, record)


def test_columns_stop_on_their_own(pg):
    A = rmat_np.rmat_csr(12, 8, seed=5)
    n, Mn, graph = A.shape[0], sp.csr_array(orc.normalize(A, "col", True)), pg.AdjacencyWrapper(A, directed=True)
    oracle = lambda M, p, **kw: orc.heat_kernel(M, p, t=5, coefficient_type="chebyshev", **kw)      # noqa: E731
    make = lambda **kw: pg.HeatKernel(5, coefficient_type="chebyshev", preprocessor=pg.preprocessor(assume_immutability=True),      # noqa: E731
                                      error_type=pg.L1, tol=1e-10, max_iters=2000, **kw)
    feats, want_iters = np.zeros((n, 5)), []
    for j, size in enumerate(SIZES):
        for seed in range(j + 1, j + 40, 5):                      # the first seed set whose stop is clear of the tolerance
            column = np.zeros(n)
            column[rmat_np.seed_nodes(A, size, seed=seed)] = 1.0 + j
            it, clear = _clear_stop(oracle, Mn, column)
            if clear:
                break
        assert clear, j                                           # the premise of "no iteration apart", checked on the f64 oracle
        feats[:, j] = column
        want_iters.append(it)
    ranker = make(f64_batch=True)
    out = np.asarray(ranker.propagate(graph, pg.to_primitive(feats)), dtype=np.float64)
    assert _marked(ranker) and all(r["converged"] for r in _records(ranker)) and len(set(want_iters)) > 1
    assert [r["iterations"] for r in _records(ranker)] == want_iters
    for j in range(5):
        single = make()
        got1 = np.asarray(single.rank(graph, feats[:, j].copy()).np, dtype=np.float64)
        assert single.convergence.iteration == want_iters[j] and _one_ulp(out[:, j], got1), j


def _call(g, P, R, coeffs=SCHEDULE, **cfg):
    """(status, results, cfg) of the entry under the "iters" rule over the whole schedule"""
    from pygrank_amd import _lib as L
    cfg = L.LoopCfg(**dict(dict(alpha=0.0, use_quotient=0, err_kind=L.ERR_ITERS, tol=0.0, max_iters=len(SCHEDULE) + 1, end_modulo=1,
                                out_scale=1.0, in_norm=1.0, start_from_p=1, reserved=0), **cfg))
    results, ones = (L.LoopResult * P.b)(), (C.c_double * P.b)(*([1.0] * P.b))
    entry = L.entry("pgh_cheb_run_batch_f64")
    return entry(g._h, P._h, coeffs.ctypes.data_as(C.c_void_p), len(coeffs), R._h, C.byref(cfg), ones, results), results, cfg


@pytest.mark.parametrize("which", ["small50", "hub"])
def test_entry_against_the_recurrence_and_the_single_vector_loop(pg, which):
    """No bound is fixed for the recurrence's amplification of noise: the batch is held to one f32 ulp of the single-vector loop
    (pgh_poly_run, form 1), and both deviations from the long-double recurrence are printed."""
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix, DeviceVector
    rng = np.random.default_rng(64)
    W = bc.small_graph(rng) if which == "small50" else bc.hub_graph(rng, weights="mult")[0]
    op, upload = bc.operator_of(W, "col")
    g, n, b, empty = upload(pg), W.shape[0], 5, op.nnz_row == 0
    assert which != "hub" or (op.nnz_row.max() >= 6000 and empty.sum() >= 400)      # >= 11 tiles of one row; empty rows
    X = bc.draw_x(rng, n, b)                                      # signed, thirteen binades, column 2 is zero
    X[empty] = 0.0                                                # (result_1 = c_1 p: an empty row then stays zero)
    P, R, again = DeviceMatrix.from_host(X), DeviceMatrix.from_host(np.full((n, b), SENTINEL)), DeviceMatrix.from_host(np.full((n, b), SENTINEL))
    status, results, cfg = _call(g, P, R)
    assert status == 0 and _call(g, P, again)[0] == 0 and [r.iterations for r in results] == [len(SCHEDULE) + 1] * b
    got = R.numpy()
    assert np.array_equal(got.view(np.uint64), again.numpy().view(np.uint64)) and not got[empty].any() and not got[:, 2].any()
    for j in range(b):
        term = X[:, j].astype(fc.LD)                              # sum_k c_k T_k in long double
        ref = fc.LD(SCHEDULE[0]) * term
        for k in range(2, len(SCHEDULE) + 1):
            term = fc.matvec_ld(op.MT, term) if k == 2 else 2 * fc.matvec_ld(op.MT, term) - term
            ref = ref + fc.LD(SCHEDULE[k - 1]) * term
        v, r, res = DeviceVector.from_host(X[:, j]), DeviceVector.empty(n), L.LoopResult()
        L.check(L.lib().pgh_poly_run(g._h, v._h, SCHEDULE.ctypes.data_as(C.c_void_p), len(SCHEDULE), 1, r._h, C.byref(cfg), C.byref(res)))
        dev = [float(np.max(np.abs(x.astype(fc.LD) - ref))) for x in (r.numpy(), got[:, j])]
        print("%s column %d: worst deviation from the long-double recurrence: single-vector %.3e, batch %.3e" % (which, j, *dev))
        assert res.iterations == results[j].iterations and _one_ulp(got[:, j], r.numpy()), j


@pytest.mark.parametrize("option", ["mabs", "linf", "iters", "nonorm", "modulo"])
def test_rules_and_options_match_rank_per_column(pg, small_graphs, option):
    kwargs = dict(dict(max_iters=2000), **OPTIONS[option], t=3, coefficient_type="chebyshev")
    A, directed, p = small_graphs("rmat10_dir")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    F = np.outer(p, [1.0, 4.0, 0.0]) + np.where(np.random.default_rng(7).random((A.shape[0], 3)) < 0.01, 1.0, 0.0) * [1.0, 0.0, 0.0]
    on = build_ranker(pg, "heat", dict(kwargs, f64_batch=True))
    got = np.asarray(on.propagate(graph, pg.to_primitive(F)), dtype=np.float64)
    assert len(_records(on)) == 3 and _marked(on) and not got[:, 2].any()
    for j in range(2):
        single = build_ranker(pg, "heat", kwargs)
        want = np.asarray(single.rank(graph, F[:, j].copy()).np, dtype=np.float64)
        assert _records(on)[j]["iterations"] == single.convergence.iteration and _one_ulp(got[:, j], want), j


def test_declines_errors_and_the_default_route(pg, small_graphs):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceGraph, DeviceMatrix
    rng = np.random.default_rng(3)
    _, upload = bc.operator_of(bc.small_graph(rng), "col")
    P, R = DeviceMatrix.from_host(np.abs(bc.draw_x(rng, 50, 3))), DeviceMatrix.from_host(np.full((50, 3), SENTINEL))
    with fc.layout_env(PGH_FORMAT="csr"):
        row_major = upload(pg)
    empty = pg.scipy_sparse_to_backend(sp.csr_array((6, 6), dtype=np.float64))
    wide = DeviceGraph.from_factored(sp.csr_array((np.ones(3), ([0, 1, 4], [1, 2, 6])), shape=(5, 7)))
    for graph in (row_major, empty, wide):                        # declined, nothing written
        assert "row-major" in row_major.format() and _call(graph, P, R)[0] == L.DECLINED and L.lib().pgh_last_error()
    P65, R65 = DeviceMatrix.from_host(np.ones((50, 65))), DeviceMatrix.from_host(np.full((50, 65), SENTINEL))
    assert _call(upload(pg), P, R, coeffs=np.array([1.0, float("nan")]))[0] not in (0, L.DECLINED)      # a non-finite coefficient
    assert _call(upload(pg), P65, R65)[0] not in (0, L.DECLINED)                                        # a width of 65 ...
    with pytest.raises(L.EngineError):                                                                  # ... and no slab is 0 wide
        DeviceMatrix.empty(50, 0)
    assert np.all(R.numpy() == SENTINEL) and np.all(R65.numpy() == SENTINEL)
    # without f64_batch=True the form keeps its column loop, and so it does under PGH_CHEB_F32=1
    A, directed, p = small_graphs("rmat10_dir")
    graph, F = pg.AdjacencyWrapper(A, directed=directed), pg.to_primitive(np.outer(p, [1.0, 2.0]))
    make = lambda **kw: pg.HeatKernel(3, coefficient_type="chebyshev", error_type="iters", max_iters=8, **kw)      # noqa: E731
    plain, batched, in_f32 = make(), make(f64_batch=True), make(f64_batch=True)
    want, got = np.asarray(plain.propagate(graph, F), dtype=np.float64), np.asarray(batched.propagate(graph, F), dtype=np.float64)
    with fc.layout_env(PGH_CHEB_F32="1"):
        in_f32.propagate(graph, F)
    assert _one_ulp(got, want) and _marked(batched) and not hasattr(plain, "last_batches") and not hasattr(in_f32, "last_batches")
