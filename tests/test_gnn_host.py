"""pygrank_amd.gnn without a GPU: the coefficient mappings of include/pgh_gnn.h pgh_linear_run_batch against explicit transposes on dense
matrices, and differentiable_propagate on the host double, which lacks the entries of include/pgh_gnn.h."""
import os
import re

import numpy as np
import pytest

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_table_and_declined():
    from pygrank_amd import _lib
    assert _lib.TABLES["pgh_gnn.h"] is _lib.GNN_SIGNATURES and all(_lib.TABLES[header] is table for header, table in _lib.OPTIONAL.items())
    assert set(_lib.GNN_SIGNATURES) == {"pgh_graph_transposed", "pgh_linear_run_batch", "pgh_mat_wrap"}
    for header, other in [("pgh.h", _lib.SIGNATURES), *_lib.OPTIONAL.items()]:
        assert set(_lib.GNN_SIGNATURES).isdisjoint(other), header
    text = open(os.path.join(ROOT, "include", "pgh_gnn.h")).read()
    assert int(re.search(r"#define\s+PGH_GNN_DECLINED\s+(\d+)", text).group(1)) == _lib.DECLINED == 2
    for name in _lib.GNN_SIGNATURES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert "pgh_gnn" not in open(os.path.join(ROOT, "include", "pgh.h")).read()


def test_host_double_has_no_gnn_entry(host_engine):
    from pygrank_amd import _lib
    for name in _lib.GNN_SIGNATURES:
        assert _lib.entry(name) is None, name
    assert _lib.entry("pgh_linear_run_batch") is None


def test_gnn_entries_bind_per_library(oracle_build_dir):
    """The three names are bound on the HIP library (dlopen only), None once the host double is installed, and bound again once it is
    removed -- what tests/test_fused_plumbing.py holds the thirteen older headers to."""
    import host_double
    from pygrank_amd import _lib
    lib_path = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")
    if not os.path.exists(lib_path):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pygrank_amd", "csrc")])
    assert not host_double.active()
    try:
        hip = _lib.lib()
        for name, (restype, argtypes) in _lib.GNN_SIGNATURES.items():
            assert _lib.entry(name) is not None and _lib.entry(name).argtypes == argtypes and _lib.entry(name).restype is restype, name
        assert set(hip._pgh_gnn_entries) == set(_lib.GNN_SIGNATURES)
        host_double.install(os.path.join(oracle_build_dir, "libpgh_host_oracle.so"))
        assert _lib.lib() is not hip and all(_lib.entry(name) is None for name in _lib.GNN_SIGNATURES)
        host_double.remove()
        assert all(_lib.entry(name) is not None for name in _lib.GNN_SIGNATURES)
    finally:
        host_double.remove()


@pytest.mark.parametrize("K", [0, 1, 6, 10])
def test_linear_plans_against_explicit_transposes(K):
    """K distinct random matrices A_1 .. A_K keyed by their seeds (f64): the forward plans reproduce the PageRank recurrence and the
    taylor sum, the backward plans -- run on the explicit transposes, which is what the transposed graph applies for a seed -- the adjoint
    <F x, w> = <x, F^T w> and, more strictly, F^T as a matrix."""
    from pygrank_amd.gnn import linear_plan, run_plan
    rng = np.random.default_rng(40 + K)
    n, seed0, alpha = 7, 1234, 0.9
    mats = {seed0 + k: rng.standard_normal((n, n)) for k in range(K)}
    coeffs = list(rng.standard_normal(K + 1))
    if K >= 6:
        coeffs[2] = 0.0
    eye = np.eye(n)
    fwd = lambda seed, s: mats[seed] @ s
    bwd = lambda seed, s: mats[seed].T @ s
    # the maps as matrices, written out product by product
    x, F_ppr = eye.copy(), None
    for k in range(K):
        x = alpha * mats[seed0 + k] @ x + (1 - alpha) * eye
    F_ppr = x
    term, F_tay = eye.copy(), coeffs[0] * eye
    for k in range(1, K + 1):
        term = mats[seed0 + k - 1] @ term
        F_tay = F_tay + coeffs[k] * term
    for kind, params, F in (("pagerank", alpha, F_ppr), ("taylor", coeffs, F_tay)):
        plan = linear_plan(kind, params, K, seed0)
        assert plan[4] == seed0 and plan[5] == 1 and len(plan[1]) == len(plan[2]) == K and len(plan[3]) == K + 1
        assert np.max(np.abs(run_plan(fwd, eye, plan) - F)) <= 1e-12 * max(1.0, np.max(np.abs(F))), kind
        back = linear_plan(kind, params, K, seed0, backward=True)
        assert back[4] == seed0 + K - 1 and back[5] == -1 and len(back[1]) == len(back[2]) == K and len(back[3]) == K + 1
        assert np.max(np.abs(run_plan(bwd, eye, back) - F.T)) <= 1e-12 * max(1.0, np.max(np.abs(F))), kind
        X, W = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
        lhs, rhs = np.sum(run_plan(fwd, X, plan) * W), np.sum(X * run_plan(bwd, W, back))
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), kind
    with pytest.raises(Exception):
        linear_plan("taylor", coeffs + [1.0], K, seed0)
    with pytest.raises(Exception):
        linear_plan("chebyshev", coeffs, K, seed0)


@pytest.fixture()
def host_pg(host_engine):
    """The host double, and every graph built on it freed while it is still installed: the transposed operator refers to itself
    (_pygrank_preprocessed), so only the cycle collector frees it -- later, with whatever library is bound then."""
    import gc
    yield host_engine
    gc.collect()


def _setup(pg, use_quotient=False, **kwargs):
    A, directed, _ = cases.GRAPHS["rmat10_dir"]()
    graph = pg.AdjacencyWrapper(A, directed=directed)
    pre = pg.preprocessor(assume_immutability=True)
    ranker = pg.PageRank(0.9, preprocessor=pre, use_quotient=use_quotient, error_type="iters", max_iters=6, **kwargs)
    return A.shape[0], graph, ranker


def test_graph_dropout_needs_the_header(host_pg):
    import torch
    from pygrank_amd.gnn import differentiable_propagate
    from pygrank_amd.backend import hip
    n, graph, ranker = _setup(host_pg)
    X = torch.rand((n, 3), dtype=torch.float32, requires_grad=True)
    before = hip.peek_dropout_seed()
    with pytest.raises(Exception, match=r"include/pgh_gnn\.h"):
        differentiable_propagate(ranker, graph, X, graph_dropout=0.5)
    assert hip.peek_dropout_seed() == before                  # nothing ran: no seed is spent


def test_bad_rates_and_non_linear_rankers_raise(host_pg):
    import torch
    from pygrank_amd.gnn import differentiable_propagate
    pg = host_pg
    n, graph, ranker = _setup(pg)
    X = torch.rand((n, 2), dtype=torch.float32)
    for rate in (1.0, -0.1, 1.5):
        with pytest.raises(Exception, match="graph_dropout"):
            differentiable_propagate(ranker, graph, X, graph_dropout=rate)
    for bad in (pg.PageRank(0.9), _setup(pg, use_quotient=True)[2]):
        for rate in (0, 0.5):
            with pytest.raises(Exception, match="fixed number of steps"):
                differentiable_propagate(bad, graph, X, graph_dropout=rate)


def test_rate_zero_is_the_call_without_the_argument(host_pg):
    import torch
    from pygrank_amd import gnn
    pg = host_pg
    n, graph, ranker = _setup(pg)
    rng = np.random.default_rng(8)
    base = torch.tensor(rng.random((n, 3)), dtype=torch.float32)
    W = torch.tensor(rng.random((n, 3)), dtype=torch.float32)
    outs = []
    for kwargs in ({}, dict(graph_dropout=0), dict(graph_dropout=0, fused=False)):
        X = base.clone().requires_grad_(True)
        Y = gnn.differentiable_propagate(ranker, graph, X, **kwargs)
        (Y * W).sum().backward()
        outs.append((Y.detach().numpy().copy(), X.grad.numpy().copy()))
        assert gnn.last_call["route"] == "host" and gnn.last_call["widths"] == [3] and gnn.last_call["seed0"] == []
        assert gnn.last_call["staged_bytes"] == 2 * n * 3 * 4 and gnn.last_call["backward"]["route"] == "host"
    for Y, G in outs[1:]:
        assert np.array_equal(Y, outs[0][0]) and np.array_equal(G, outs[0][1])
    assert np.any(outs[0][0] != 0) and np.any(outs[0][1] != 0)
