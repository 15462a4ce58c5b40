"""The mixed batches of include/pgh_mixed.h called directly: pgh_ppr_run_batch_mixed (an alpha per column) and
pgh_poly_run_batch_mixed (a coefficient schedule per column).

Every column is held against the fp64 oracle (oracle/ref_loops.py through parity_common.run_oracle) run on that column's own
parameters: ranks within parity_common.tolerance_for (1e-6 relative L-inf) and equal iteration counts -- a stop one check apart is
accepted only when the oracle's own residual at the stopping check the two disagree on (the earlier stop) lies within 2 % of the
tolerance (the rule of tests/test_gpu_batch_filters.py _stop_margin_ok, which has the engine as the earlier one).

Widths 1, 5, 17 and 64: a lone column, a part-filled float4 group, a part-filled lane group, every lane.

A [n, 0] slab cannot be built through the C-ABI (pgh_mat_alloc refuses it), so the b = 0 refusal is checked where it arises."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cases
from oracle import ref_loops as orc
from parity_common import EPS32, rel_linf, run_oracle, tolerance_for

pytestmark = pytest.mark.gpu

WIDTHS = (1, 5, 17, 64)
ERR = {"mabs": 0, "l1": 1, "linf": 2, "iters": 3}
L1 = dict(error_type="l1", tol=1e-6, max_iters=3000)


@pytest.fixture(scope="module")
def pg():
    import pygrank_amd
    from pygrank_amd import _lib
    pygrank_amd.load_backend("hip")
    assert _lib.runtime_name().startswith("hip:")
    for name in _lib.MIXED_SIGNATURES:
        assert _lib.entry(name) is not None, name
    return pygrank_amd


def _holes(A):
    """rmat10_dir with every 17th node isolated (no edges at all) on top of its dangling rows."""
    keep = (np.arange(A.shape[0]) % 17 != 3).astype(float)
    A = sp.csr_array(sp.diags(keep) @ sp.csr_array(A, dtype=np.float64) @ sp.diags(keep))
    A.eliminate_zeros()
    A.sort_indices()
    return A


@pytest.fixture(scope="module")
def graphs(pg):
    built = {}

    def get(key):
        if key not in built:
            A, directed, _ = cases.GRAPHS["rmat10_dir" if key == "holes" else key]()
            if key == "holes":
                A = _holes(A)
                assert (np.diff(A.indptr) == 0).sum() > A.shape[0] // 17      # dangling rows beside the isolated nodes
            g = pg.DeviceGraph.from_adjacency(A, "col" if directed else "symmetric")
            built[key] = dict(A=A, directed=directed, g=g, n=A.shape[0])
        return built[key]
    return get


def _columns(n, b, seed=0, zero=None):
    """b non-negative personalizations of different norms on different seed sets, rounded through f32; column `zero` all zeros."""
    rng = np.random.default_rng(100 + seed)
    P = np.zeros((n, b))
    for j in range(b):
        idx = rng.choice(n, int(rng.integers(3, 12)), replace=False)
        P[idx, j] = rng.uniform(0.5, 1.5, len(idx)) * (1 + j % 7)
    if zero is not None:
        P[:, zero] = 0.0
    return P.astype(np.float32).astype(np.float64)


def _cfg(rule, use_quotient=True, start_from_p=True):
    from pygrank_amd import _lib as L
    tol = rule.get("tol", 1e-6)
    return L.LoopCfg(alpha=-7.0, use_quotient=1 if use_quotient else 0, err_kind=ERR[rule.get("error_type", "mabs")],
                     tol=max(float(tol), EPS32), max_iters=int(rule.get("max_iters", 100)), end_modulo=int(rule.get("end_modulo", 1)),
                     out_scale=1.0, in_norm=0.0, start_from_p=1 if start_from_p else 0)


def _normalised(P):
    norms = np.abs(P).sum(axis=0)
    return P / np.where(norms > 0, norms, 1.0), norms


def _run_ppr(pg, G, P, alphas, rule, use_quotient=True, start=None, scales="norms", entry="pgh_ppr_run_batch_mixed"):
    """-> (status, ranks [n, b], results).  The slab handed in holds `start` (a warm start) or 7s (output only)."""
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix
    b = P.shape[1]
    Pn, norms = _normalised(P)
    Pd = DeviceMatrix.from_host(Pn)
    R = DeviceMatrix.from_host(start if start is not None else np.full(P.shape, 7.0))
    cfg = _cfg(rule, use_quotient, start is None)
    results = (L.LoopResult * b)()
    sc = (C.c_double * b)(*norms) if scales == "norms" else None
    if entry == "pgh_ppr_run_batch_mixed":
        al = (C.c_double * b)(*alphas) if alphas is not None else None
        status = L.entry(entry)(G["g"]._h, Pd._h, R._h, C.byref(cfg), al, sc, results)
    else:
        cfg.alpha = float(alphas[0])
        status = L.lib().pgh_ppr_run_batch(G["g"]._h, Pd._h, R._h, C.byref(cfg), sc, results)
    return status, R.numpy(), results


def _run_poly(pg, G, P, schedules, rule):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix
    b = P.shape[1]
    Pn, norms = _normalised(P)
    Pd = DeviceMatrix.from_host(Pn)
    R = DeviceMatrix.from_host(np.full(P.shape, 7.0))
    terms = max(len(s) for s in schedules)
    coeffs = np.zeros((terms, b))                           # shorter schedules zero-padded
    for j, s in enumerate(schedules):
        coeffs[:len(s), j] = s
    cfg = _cfg(rule, False, True)
    results = (L.LoopResult * b)()
    sc = (C.c_double * b)(*norms)
    status = L.entry("pgh_poly_run_batch_mixed")(G["g"]._h, Pd._h, coeffs.ctypes.data_as(C.c_void_p), terms, R._h, C.byref(cfg),
                                                 sc, results)
    return status, R.numpy(), results


def _oracle_at(G, p, algo, kwargs, iters):
    """The oracle's UN-scaled result after exactly `iters` iterations."""
    kw = {k: v for k, v in kwargs.items() if k not in ("tol", "error_type", "max_iters", "end_modulo")}
    return run_oracle(G["A"], G["directed"], p, algo, dict(kw, error_type="iters", max_iters=iters, preserve_norm=False), eps=EPS32)[0]


def _check_column(G, p, algo, kwargs, got, result, j):
    """Column j against the oracle on its own parameters (see the module docstring)."""
    assert result.converged == 1 or kwargs.get("error_type") == "iters", (j, result.iterations)
    want, it = run_oracle(G["A"], G["directed"], p, algo, kwargs, eps=EPS32)
    print(f"column {j}: {algo} {({k: v for k, v in kwargs.items() if k in ('alpha', 't')})} iterations {result.iterations} oracle {it}")
    if result.iterations != it:
        assert abs(result.iterations - it) == 1, (j, result.iterations, it)
        kind, tol = kwargs.get("error_type", "mabs"), max(kwargs.get("tol", 1e-6), EPS32)
        assert kind != "iters", (j, result.iterations, it)
        # the check the two disagree on is the one of the earlier stop: there one of them found the change above the tolerance and the
        # other did not (with the engine the earlier, this is _stop_margin_ok of tests/test_gpu_batch_filters.py)
        stop = min(result.iterations, it)
        residual = orc.RESIDUALS[kind](_oracle_at(G, p, algo, kwargs, stop - 1), _oracle_at(G, p, algo, kwargs, stop))
        print(f"column {j}: oracle residual at the check of iteration {stop} {residual:.6e} (tolerance {tol:.1e})")
        assert abs(residual - tol) <= 0.02 * tol, (j, result.iterations, it, residual)
        want = _oracle_at(G, p, algo, kwargs, result.iterations) * np.abs(p).sum()
    err = rel_linf(got, want)
    print(f"column {j}: rel linf {err:.3e}")
    assert err <= tolerance_for(kwargs), (j, err)


def _spread(b):
    """alphas over 0.5 ... 0.99: the columns freeze many steps apart"""
    return [0.99] if b == 1 else list(np.linspace(0.5, 0.99, b))


@pytest.mark.parametrize("b", WIDTHS)
def test_equal_alphas_match_the_uniform_batch(pg, graphs, b):
    G = graphs("rmat10_dir")
    P = _columns(G["n"], b, seed=b)
    status, got, res = _run_ppr(pg, G, P, [0.85] * b, L1)
    assert status == 0
    status, uni, res_u = _run_ppr(pg, G, P, [0.85] * b, L1, entry="pgh_ppr_run_batch")
    assert status == 0
    assert [r.iterations for r in res] == [r.iterations for r in res_u]
    assert [r.converged for r in res] == [1] * b
    for j in range(b):
        assert rel_linf(got[:, j], uni[:, j]) <= tolerance_for(L1), j
    for j in sorted({0, b // 2, b - 1}):
        _check_column(G, P[:, j], "pagerank", dict(alpha=0.85, **L1), got[:, j], res[j], j)


@pytest.mark.parametrize("use_quotient", [True, False], ids=["quotient", "noquotient"])
@pytest.mark.parametrize("b", WIDTHS)
def test_spread_alphas_stop_at_their_own_iteration(pg, graphs, b, use_quotient):
    """On this graph the oracle takes 10 / 14 iterations at alpha = 0.5 / 0.99 with the quotient and 16 / 312 without it: without the
    quotient the last column runs for hundreds of steps after the first has frozen."""
    G = graphs("rmat10_dir")
    P = _columns(G["n"], b, seed=10 + b)
    alphas = _spread(b)
    rule = L1
    status, got, res = _run_ppr(pg, G, P, alphas, rule, use_quotient=use_quotient)
    assert status == 0
    iters = [r.iterations for r in res]
    if b > 1:
        assert iters[-1] > (1 if use_quotient else 10) * iters[0], iters
    for j in (range(b) if b <= 17 else (0, 1, 13, 31, 32, 47, 62, 63)):
        _check_column(G, P[:, j], "pagerank", dict(alpha=alphas[j], use_quotient=use_quotient, **rule), got[:, j], res[j], j)


RULES = {
    "l1": L1,
    "mabs": dict(error_type="mabs", tol=1e-7, max_iters=3000),
    "linf": dict(error_type="linf", tol=1e-6, max_iters=3000),
    "iters": dict(error_type="iters", max_iters=23),
    "modulo3": dict(error_type="l1", tol=1e-6, max_iters=3000, end_modulo=3),
}


@pytest.mark.parametrize("use_quotient", [True, False], ids=["quotient", "noquotient"])
@pytest.mark.parametrize("rule", sorted(RULES))
def test_stopping_rules_and_the_quotient(pg, graphs, rule, use_quotient):
    G = graphs("weighted300")
    b = 5
    P = _columns(G["n"], b, seed=3)
    alphas = [0.5, 0.7, 0.85, 0.9, 0.95]
    status, got, res = _run_ppr(pg, G, P, alphas, RULES[rule], use_quotient=use_quotient)
    assert status == 0
    for j in range(b):
        _check_column(G, P[:, j], "pagerank", dict(alpha=alphas[j], use_quotient=use_quotient, **RULES[rule]), got[:, j], res[j], j)


def test_warm_start(pg, graphs):
    G = graphs("rmat10_dir")
    b, n = 5, G["n"]
    P = _columns(n, b, seed=4)
    alphas = _spread(b)
    Pn, _ = _normalised(P)
    start = (0.5 * Pn + 0.5 / n).astype(np.float32).astype(np.float64)
    status, got, res = _run_ppr(pg, G, P, alphas, L1, start=start)
    assert status == 0
    status, cold, res_cold = _run_ppr(pg, G, P, alphas, L1)
    assert status == 0
    assert [r.iterations for r in res] != [r.iterations for r in res_cold]
    for j in range(b):
        _check_column(G, P[:, j], "pagerank", dict(alpha=alphas[j], warm_start=start[:, j], **L1), got[:, j], res[j], j)


def test_only_the_slow_column_hits_max_iters(pg, graphs):
    G = graphs("rmat10_dir")
    alphas = [0.5, 0.85, 0.99, 0.9, 0.7]
    P = _columns(G["n"], 5, seed=5)
    rule = dict(error_type="l1", tol=1e-6, max_iters=200, use_quotient=False)     # (without the quotient: 0.99 needs about 300 iterations)
    status, got, res = _run_ppr(pg, G, P, alphas, rule, use_quotient=False)
    assert status == 0
    assert [r.converged for r in res] == [1, 1, 0, 1, 1]
    assert res[2].iterations == 200
    for j in (0, 1, 3, 4):
        _check_column(G, P[:, j], "pagerank", dict(alpha=alphas[j], **rule), got[:, j], res[j], j)
    with pytest.raises(Exception, match="Could not converge"):
        run_oracle(G["A"], G["directed"], P[:, 2], "pagerank", dict(alpha=0.99, **rule), eps=EPS32)
    want = _oracle_at(G, P[:, 2], "pagerank", dict(alpha=0.99, use_quotient=False), 200) * np.abs(P[:, 2]).sum()
    assert rel_linf(got[:, 2], want) <= tolerance_for(rule)


@pytest.mark.parametrize("use_quotient", [True, False], ids=["quotient", "noquotient"])
def test_zero_column_dangling_rows_and_isolated_nodes(pg, graphs, use_quotient):
    G = graphs("holes")
    b, n = 17, G["n"]
    P = _columns(n, b, seed=6, zero=2)
    isolated = np.flatnonzero(np.arange(n) % 17 == 3)
    P[isolated[:3], 4] = 1.0                                 # seeds on isolated nodes: their mass stays where it is
    alphas = _spread(b)
    status, got, res = _run_ppr(pg, G, P, alphas, L1, use_quotient=use_quotient)
    assert status == 0
    assert np.all(got[:, 2] == 0)
    for j in range(b):
        if j != 2:
            _check_column(G, P[:, j], "pagerank", dict(alpha=alphas[j], use_quotient=use_quotient, **L1), got[:, j], res[j], j)


def test_out_scales_per_column(pg, graphs):
    G = graphs("weighted300")
    P = _columns(G["n"], 5, seed=7)
    alphas = _spread(5)
    status, scaled, _ = _run_ppr(pg, G, P, alphas, L1)
    assert status == 0
    status, plain, _ = _run_ppr(pg, G, P, alphas, L1, scales=None)       # cfg.out_scale = 1 for every column
    assert status == 0
    norms = np.abs(P).sum(axis=0)
    assert len(set(norms.round(3))) > 1
    for j in range(5):
        assert rel_linf(scaled[:, j], plain[:, j] * norms[j]) <= 2 * EPS32, j
        assert abs(plain[:, j].sum() - 1.0) <= 1e-5, j


def _schedule(coeff, count):
    out, prev = [], None
    for it in range(1, count + 1):
        prev = coeff(prev, it)
        out.append(float(prev))
    return out


# The closed-form loops stop on the exact change of an f32 accumulator.  Its L1 mass is the sum of the schedule (at most 44.5, for
# HeatKernel t = 7 as the reference draws its coefficients), and one step's roundings move the measured change by up to mass * 2^-24 =
# 2.7e-6: the L1 tolerance is one the 2 % margin of _check_column is wider than that (at 1e-6 the engine stops HeatKernel t = 7 one
# step after the oracle, whose change there is 11 % below the tolerance).  The Mabs rule, clamped at fp32 eps, is an L1 change of
# 1.2e-4 on this graph: the engine's own floor, kept as a case.
POLY_RULES = {"l1": dict(error_type="l1", tol=2e-4, max_iters=200), "mabs": dict(error_type="mabs", tol=1e-8, max_iters=200),
              "iters": dict(error_type="iters", max_iters=12)}


@pytest.mark.parametrize("rule", sorted(POLY_RULES))
@pytest.mark.parametrize("b", WIDTHS)
def test_poly_batch_of_different_filters(pg, graphs, b, rule):
    """HeatKernel t = 1 / 3 / 7, PageRankClosed 0.85 and a three-weight GenericGraphFilter side by side: schedules of unequal length."""
    G = graphs("rmat10_dir")
    kw = POLY_RULES[rule]
    terms = kw["max_iters"] - 1
    family = [("heat", dict(t=1), _schedule(orc.heat_kernel_coefficient(1), terms)),
              ("heat", dict(t=3), _schedule(orc.heat_kernel_coefficient(3), terms)),
              ("heat", dict(t=7), _schedule(orc.heat_kernel_coefficient(7), terms)),
              ("pagerank_closed", dict(alpha=0.85), _schedule(orc.pagerank_closed_coefficient(0.85), terms)),
              ("generic", dict(weights=[1.0, 0.5, 0.25]), [1.0, 0.5, 0.25])]
    members = [family[(j + (3 if b == 1 else 0)) % len(family)] for j in range(b)]
    mass = max(sum(abs(c) for c in schedule) for _, _, schedule in family)
    assert rule != "l1" or mass * 2.0 ** -24 <= 0.02 * kw["tol"], mass
    P = _columns(G["n"], b, seed=20 + b)
    status, got, res = _run_poly(pg, G, P, [m[2] for m in members], kw)
    assert status == 0
    if b > 1 and rule != "iters":
        assert len({r.iterations for r in res}) > 2
    for j in (range(b) if b <= 17 else (0, 1, 2, 3, 4, 31, 32, 59, 60, 61, 62, 63)):
        algo, params, _ = members[j]
        _check_column(G, P[:, j], algo, dict(params, **kw), got[:, j], res[j], j)


def test_poly_l1_tolerance_below_the_accumulator_resolution(pg, graphs):
    """The family above under an L1 tolerance of 1e-6, below what one step's roundings of the f32 accumulator come to (see POLY_RULES):
    a column may then stop one check away from an f64 run without the oracle's change being within 2 % of the tolerance (so may the
    uniform entry and the single-vector f32 loop, which measure the change the same way).  Held to: every column converges, no stop is
    more than one check from the oracle's, and the ranks are within tolerance_for of the oracle run for the engine's iteration count."""
    G = graphs("rmat10_dir")
    kw = dict(error_type="l1", tol=1e-6, max_iters=200)
    family = [("heat", dict(t=1), _schedule(orc.heat_kernel_coefficient(1), 199)),
              ("heat", dict(t=3), _schedule(orc.heat_kernel_coefficient(3), 199)),
              ("heat", dict(t=7), _schedule(orc.heat_kernel_coefficient(7), 199)),
              ("pagerank_closed", dict(alpha=0.85), _schedule(orc.pagerank_closed_coefficient(0.85), 199)),
              ("generic", dict(weights=[1.0, 0.5, 0.25]), [1.0, 0.5, 0.25])]
    P = _columns(G["n"], 5, seed=25)
    status, got, res = _run_poly(pg, G, P, [m[2] for m in family], kw)
    assert status == 0
    for j, (algo, params, _) in enumerate(family):
        _, it = run_oracle(G["A"], G["directed"], P[:, j], algo, dict(params, **kw), eps=EPS32)
        print(f"column {j}: {algo} {params} iterations {res[j].iterations} oracle {it}")
        assert res[j].converged == 1 and abs(res[j].iterations - it) <= 1, (j, res[j].iterations, it)
        want = _oracle_at(G, P[:, j], algo, dict(params, **kw), res[j].iterations) * np.abs(P[:, j]).sum()
        assert rel_linf(got[:, j], want) <= tolerance_for(kw), j


def test_poly_schedules_with_zeros(pg, graphs):
    """A zero in the middle of a schedule changes nothing and counts as a change of 0 (the column stops there under a tolerance rule, as
    the single run does); a schedule that is zero after its first term stops at the first check after it."""
    G = graphs("weighted300")
    kw = dict(error_type="l1", tol=1e-6, max_iters=50)
    family = [("generic", dict(weights=[1.0, 0.5, 0.0, 0.25, 0.1]), [1.0, 0.5, 0.0, 0.25, 0.1]),
              ("generic", dict(weights=[1.0]), [1.0]),
              ("heat", dict(t=3), _schedule(orc.heat_kernel_coefficient(3), 49)),
              ("pagerank_closed", dict(alpha=0.5), _schedule(orc.pagerank_closed_coefficient(0.5), 49)),
              ("generic", dict(weights=[1.0, 0.5, 0.0, 0.25, 0.1]), [1.0, 0.5, 0.0, 0.25, 0.1])]
    P = _columns(G["n"], 5, seed=9)
    status, got, res = _run_poly(pg, G, P, [m[2] for m in family], kw)
    assert status == 0
    for j, (algo, params, _) in enumerate(family):
        _check_column(G, P[:, j], algo, dict(params, **kw), got[:, j], res[j], j)
    # the same schedules where nothing stops early: every term of the schedule with a hole is added
    kw = dict(error_type="iters", max_iters=9)
    status, got, res = _run_poly(pg, G, P, [m[2] for m in family], kw)
    assert status == 0
    for j, (algo, params, _) in enumerate(family):
        _check_column(G, P[:, j], algo, dict(params, **kw), got[:, j], res[j], j)


def _last_error():
    from pygrank_amd import _lib as L
    return (L.lib().pgh_last_error() or b"").decode()


def test_refusals(pg, graphs):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix
    # a non-square graph: declined, nothing written
    rng = np.random.default_rng(0)
    M = sp.random(300, 200, density=0.05, random_state=rng, format="csr")
    rect = dict(g=pg.DeviceGraph.from_scipy(M), n=200)
    P = _columns(200, 3, seed=1)
    status, out, _ = _run_ppr(pg, rect, P, [0.5, 0.85, 0.9], L1)
    assert status == L.DECLINED and "square" in _last_error()
    assert np.all(out == 7.0)
    status, out, _ = _run_poly(pg, rect, P, [[1.0, 0.5]] * 3, L1)
    assert status == L.DECLINED and "square" in _last_error()
    assert np.all(out == 7.0)
    # a row-major graph (PGH_FORMAT=csr at upload): declined, nothing written
    A, directed, _ = cases.GRAPHS["rmat10_dir"]()
    saved = os.environ.get("PGH_FORMAT")
    os.environ["PGH_FORMAT"] = "csr"
    try:
        g = pg.DeviceGraph.from_adjacency(A, "col")
    finally:
        if saved is None:
            os.environ.pop("PGH_FORMAT", None)
        else:
            os.environ["PGH_FORMAT"] = saved
    assert "row-major" in g.format()
    rm = dict(g=g, n=A.shape[0])
    P = _columns(A.shape[0], 3, seed=2)
    status, out, _ = _run_ppr(pg, rm, P, [0.5, 0.85, 0.9], L1)
    assert status == L.DECLINED and "blocked layout" in _last_error()
    assert np.all(out == 7.0)
    status, out, _ = _run_poly(pg, rm, P, [[1.0, 0.5]] * 3, L1)
    assert status == L.DECLINED and "blocked layout" in _last_error()
    assert np.all(out == 7.0)
    # errors, not declines: 65 columns, no columns, null alphas, a non-finite alpha
    G = graphs("rmat10_dir")
    status, out, _ = _run_ppr(pg, G, _columns(G["n"], 65, seed=3), [0.85] * 65, L1)
    assert status not in (0, L.DECLINED) and "[1, 64]" in _last_error()
    assert np.all(out == 7.0)
    status, out, _ = _run_poly(pg, G, _columns(G["n"], 65, seed=3), [[1.0, 0.5]] * 65, L1)
    assert status not in (0, L.DECLINED) and "[1, 64]" in _last_error()
    with pytest.raises(L.EngineError):                      # b = 0: no such slab exists for the entries to be handed
        DeviceMatrix.empty(G["n"], 0)
    P = _columns(G["n"], 3, seed=4)
    status, out, _ = _run_ppr(pg, G, P, None, L1)
    assert status not in (0, L.DECLINED) and "null" in _last_error()
    assert np.all(out == 7.0)
    status, out, _ = _run_ppr(pg, G, P, [0.5, float("nan"), 0.9], L1)
    assert status not in (0, L.DECLINED) and "non-finite" in _last_error()
    assert np.all(out == 7.0)
    # ... and the same inputs with their alphas run
    status, out, res = _run_ppr(pg, G, P, [0.5, 0.85, 0.9], L1)
    assert status == 0 and [r.converged for r in res] == [1, 1, 1] and not np.any(out == 7.0)
