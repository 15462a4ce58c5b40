"""The retiring f64 multi-seed loops and the pair form of their product (include/pgh_retire64.h) on the MI355X: the pair product
against the long-double product and bound of batch64_common; columns of retiring runs whose premises (clear stops, the narrowings, an
ld == 2 tail) come from the f64 oracle alone; bit-identity where nothing narrows; the edges."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import batch64_common as bc
import f64_common as fc
from oracle import ref_loops as orc
from oracle import rmat_np

pytestmark = pytest.mark.gpu

SENTINEL, TOL, NARROWED = -7.25, 1e-10, 32
LEVELS = (32, 16, 8, 4, 2)
COLUMNS = {64: list(range(64)), 5: [0, 1, 39, 62, 63], 3: [0, 39, 62], 2: [39, 62]}
PRODUCT_GRAPHS = ["small50/col", "hub/col", "hub/symmetric", "hub/col-valued", "hub/symmetric-valued", "rmat12/col-valued",
                  "rmat12/symmetric-valued"]


@pytest.fixture(scope="module")
def pg():
    import pygrank_amd
    from pygrank_amd import _lib
    pygrank_amd.load_backend("hip")
    assert _lib.runtime_name().startswith("hip:") and all(_lib.entry(name) is not None for name in _lib.RETIRE64_SIGNATURES)
    return pygrank_amd


def _pair(g, X, b=None, out=None):
    from pygrank_amd import _lib as L
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.full(X.shape, SENTINEL) if out is None else out
    return L.entry("pgh_spmm_f64_pair")(g._h, X.ctypes.data_as(C.c_void_p), X.shape[1] if b is None else b, Y.ctypes.data_as(C.c_void_p)), Y


@pytest.mark.parametrize("name", PRODUCT_GRAPHS)
def test_pair_product_is_held_to_f64_row_by_row(pg, name):
    from pygrank_amd import _lib as L
    rng = np.random.default_rng(64)
    which, kind = name.split("/")
    W = {"small50": lambda: bc.small_graph(rng), "rmat12": lambda: sp.csr_array(rmat_np.rmat_csr(12, 8)),
         "hub": lambda: bc.hub_graph(rng, weights="real" if kind.endswith("valued") else "mult")[0]}[which]()
    op, upload = bc.operator_of(W, kind)
    g = upload(pg)
    if which == "hub":
        assert op.nnz_row.max() >= 6000 and (op.nnz_row == 0).sum() >= 400      # >= 11 tiles of one row; empty rows
    worst = 0.0
    for b in (1, 2):
        X = bc.draw_x(rng, W.shape[0], b)                         # (b == 2: column 1 is the zero column)
        status, Y = _pair(g, X)
        assert status == 0, (name, b, status)
        ratio, zeros = bc.product_ratio(Y, op, X)
        print("pgh_spmm_f64_pair %s b=%d worst |err| / bound = %.3f" % (name, b, ratio))
        assert zeros and ratio <= 1.0, (name, b, ratio)           # empty rows and the zero column: exactly zero
        worst = max(worst, ratio)
        assert np.array_equal(Y.view(np.uint64), _pair(g, X)[1].view(np.uint64)), (name, b)
    assert worst > 0.0
    for width in (0, 3):
        status, Y = _pair(g, bc.draw_x(rng, W.shape[0], 3), b=width)
        assert status not in (0, L.DECLINED) and np.all(Y == SENTINEL), width


def _clear_stop(oracle, M, p):
    """(iterations, clear): the f64 oracle's stopping iteration, and whether its L1 residual at the stopping check and at the check
    before each lie at least 1e-6 tol away from tol (tests/test_gpu_batch64.py's premise)"""
    _, it = oracle(M, p, error_type="l1", tol=TOL, max_iters=2000)
    x2, x1, x0 = (oracle(M, p, error_type="iters", max_iters=m, preserve_norm=False)[0] for m in (it, it - 1, it - 2))
    at_stop, before = np.abs(x2 - x1).sum(), np.abs(x1 - x0).sum()
    return it, (at_stop <= TOL and before > TOL and min(abs(at_stop - TOL), abs(before - TOL)) >= 1e-6 * TOL)


@pytest.fixture(scope="module", params=["pagerank", "absorbing", "sarw"])
def run(pg, request):
    """One family on RMAT scale 12 at L1 tol 1e-10; 64 columns: 39 dense ones stop first, 23 sets of 1000 seeds a step later, two single
    seeds four to ten steps after them.  Per column the oracle's (iterations, clear) and the single f64 rank()'s (values, iterations)."""
    A = rmat_np.rmat_csr(12, 8, seed=5)
    n = A.shape[0]
    Mn, graph = sp.csr_array(orc.normalize(A, "col", True)), pg.AdjacencyWrapper(A, directed=True)
    rng = np.random.default_rng(64)
    F = np.zeros((n, 64))
    F[:, :39] = ((np.diff(A.indptr) + np.bincount(A.indices, minlength=n))[:, None] * rng.uniform(0.5, 1.5, (n, 39))).astype(np.float32)
    for j in range(39, 62):
        F[rmat_np.seed_nodes(A, 1000, seed=j), j] = 1.0
    F[[207, 1006], [62, 63]] = 1.0
    rule = dict(preprocessor=pg.preprocessor(assume_immutability=True), error_type=pg.L1, tol=TOL, max_iters=2000)
    make, oracle = {
        "pagerank": (lambda **kw: pg.PageRank(0.85, **dict(rule, **kw)), lambda M, p, **kw: orc.pagerank(M, p, alpha=0.85, **kw)),
        "absorbing": (lambda **kw: pg.AbsorbingWalks(0.85, **dict(rule, **kw)), lambda M, p, **kw: orc.absorbing_walks(M, p, alpha=0.85, **kw)),
        "sarw": (lambda **kw: pg.SymmetricAbsorbingRandomWalks(**dict(rule, **kw)), orc.symmetric_absorbing_walks)}[request.param]
    singles = []
    for j in range(64):
        single = make()
        singles.append((np.asarray(single.rank(graph, F[:, j].copy()).np, dtype=np.float64), single.convergence.iteration))

    def propagate(cols, F=F, **kw):
        ranker = make(f64_batch=True, **kw)
        out = np.asarray(ranker.propagate(graph, pg.to_primitive(F[:, cols])), dtype=np.float64)
        return out, [c for batch in ranker.last_batches for c in batch]
    return dict(F=F, propagate=propagate, stops=[_clear_stop(oracle, Mn, F[:, j]) for j in range(64)], singles=singles)


def _stages_of(steps, width, last_step):
    """The rule of include/pgh_retire64.h under the default levels: the (ld, live, first_step) stages of `width` columns of which
    column j stops at the close of step steps[j], over `last_step` executed steps, and the sum of ld over those steps"""
    ld = (width + 1) & ~1
    out, streamed = [(ld, width, 1)], 0
    for k in range(1, last_step + 1):
        streamed += ld
        live = sum(1 for s in steps if s > k)
        below = [level for level in LEVELS if level < ld]
        if below and len(out) < 8 and 0 < live <= min(max(below), ld - 2):
            ld = (live + 1) & ~1
            out.append((ld, live, k + 1))
    return out, streamed


def _one_ulp(a, b):
    return bool(np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)))


def _report(records):
    stages = records[0]["stages"]
    assert all(r["stages"] == stages for r in records)
    return list(zip(stages["ld"], stages["live"], stages["first_step"])), stages["column_steps"]


@pytest.mark.parametrize("width", [64, 5, 3])
def test_columns_of_a_retiring_run(run, width):
    cols = COLUMNS[width]
    # the premises, from the f64 oracle alone
    assert all(run["stops"][j][1] for j in cols)
    its = [run["stops"][j][0] for j in cols]
    implied, _ = _stages_of([it - 1 for it in its], width, max(its) - 1)
    assert len(implied) - 1 >= (2 if width == 64 else 1), implied
    assert implied[-1][0] == 2 and max(its) - implied[-1][2] >= 3, implied       # the last stage: ld == 2, steps first .. max(its) - 1
    out, records = run["propagate"](cols, f64_retire=True)
    assert len(records) == width and all(r["f64"] is True and r["converged"] and r["flags"] & NARROWED for r in records)
    for i, j in enumerate(cols):
        assert records[i]["iterations"] == its[i] == run["singles"][j][1], (j, records[i]["iterations"], its[i], run["singles"][j][1])
        assert _one_ulp(out[:, i], run["singles"][j][0]), j
    print("width %d: stages %s, column_steps %d" % ((width,) + _report(records)))
    assert _report(records) == _stages_of([r["spmv"] for r in records], width, max(r["spmv"] for r in records))


def test_bit_identity_where_nothing_narrows(run):
    bits = lambda x: np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)      # noqa: E731
    for width, levels in ((2, True), (64, [])):
        (a, plain), (b, records) = run["propagate"](COLUMNS[width]), run["propagate"](COLUMNS[width], f64_retire=levels)
        assert np.array_equal(bits(a), bits(b)) and [r["iterations"] for r in plain] == [r["iterations"] for r in records], width
        assert _report(records)[0] == [((width + 1) & ~1, width, 1)] and not any(r["flags"] & NARROWED for r in records)
    b, records = run["propagate"](COLUMNS[64], f64_retire=True)
    stages = _report(records)[0]
    first = [j for j in range(64) if records[j]["spmv"] < stages[1][2]]          # stopped when the run first narrowed
    assert first and len(first) == 64 - stages[1][1] and np.array_equal(bits(a[:, first]), bits(b[:, first]))


def test_edges(pg, run, monkeypatch):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceGraph, DeviceMatrix
    # a zero column beside live ones
    X = run["F"].copy()
    X[:, 39] = 0.0
    out, records = run["propagate"](COLUMNS[3], F=X, f64_retire=True)
    assert not out[:, 1].any() and records[1]["iterations"] == 0 and len(records[0]["stages"]["ld"]) > 1
    for i, j in ((0, 0), (2, 62)):
        assert records[i]["iterations"] == run["stops"][j][0] and _one_ulp(out[:, i], run["singles"][j][0])
    caught = []                                   # no convergence within max_iters: the plain f64 batch's message; bad levels
    for kw in (dict(f64_retire=True), dict()):
        with pytest.raises(Exception) as info:
            run["propagate"](COLUMNS[5], max_iters=5, **kw)
        caught.append(str(info.value))
    assert caught[0] == caught[1] and "converge" in caught[0]
    with pytest.raises(L.EngineError):
        run["propagate"](COLUMNS[5], f64_retire=[4, 8])
    # PGH_MM64_PAIR=0: the four-lane product in the ld == 2 stages
    a, pair = run["propagate"](COLUMNS[5], f64_retire=True)
    monkeypatch.setenv("PGH_MM64_PAIR", "0")
    b, four = run["propagate"](COLUMNS[5], f64_retire=True)
    monkeypatch.delenv("PGH_MM64_PAIR")
    assert [r["iterations"] for r in pair] == [r["iterations"] for r in four] and _one_ulp(a, b) and _report(pair) == _report(four)
    # declined, nothing written: a graph without the blocked layout, a graph without entries, a matrix that is not square
    rng = np.random.default_rng(3)
    _, upload = bc.operator_of(bc.small_graph(rng), "col")
    with fc.layout_env(PGH_FORMAT="csr"):
        row_major = upload(pg)
    empty = pg.scipy_sparse_to_backend(sp.csr_array((6, 6), dtype=np.float64))
    wide = DeviceGraph.from_factored(sp.csr_array((np.ones(3), ([0, 1, 4], [1, 2, 6])), shape=(5, 7)))
    X = np.abs(bc.draw_x(rng, 50, 3))
    P, R = DeviceMatrix.from_host(X), DeviceMatrix.from_host(np.full((50, 3), SENTINEL))
    cfg = L.LoopCfg(alpha=0.85, use_quotient=1, err_kind=L.ERR_L1, tol=TOL, max_iters=50, end_modulo=1, out_scale=1.0, in_norm=1.0,
                    start_from_p=1, reserved=0)
    results, ones, norms = (L.LoopResult * 3)(), (C.c_double * 3)(1.0, 1.0, 1.0), (C.c_double * 3)(*X.sum(axis=0))
    Y, report = np.full((50, 2), SENTINEL), L.RetireReport()
    for declined in (row_major, empty, wide):
        assert L.entry("pgh_ppr_run_batch_f64_retire")(declined._h, P._h, R._h, C.byref(cfg), ones, results, norms, None, -1,
                                                       C.byref(report)) == L.DECLINED
        assert _pair(declined, X[:, :2], out=Y)[0] == L.DECLINED
    assert np.all(R.numpy() == SENTINEL) and np.all(Y == SENTINEL) and report.num_stages == 0
