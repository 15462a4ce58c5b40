"""The Krylov-space filters through the public API on the engine against the reference's recorded results
(tests/golden/golden_krylov.npz), with fused=True (include/pgh_krylov.h) and fused=False (backend primitives).

The bars are those of tests/test_krylov_host.py: ranks within 1e-6 rel-Linf and equal iteration counts; V, H and V^T V - I at most 8
times the deviation of the generator's f32 evaluation, up to 10 dimensions.  Bases are not compared at 20 or more dimensions: Lanczos
without reorthogonalisation loses orthogonality in f32 storage there (the generator's f32 evaluation on er10k at 20 dimensions: V^T V - I
reaches 0.081 and H deviates by 0.022, while the ranks stay within 1.3e-7 of the reference's)."""
import warnings

import numpy as np
import pytest

import krylov_common as kc

pytestmark = pytest.mark.gpu

SMALL = [name for name, case in kc.CASES.items() if case[4] <= kc.BASIS_DIMS]


@pytest.mark.parametrize("name", list(kc.CASES))
def test_golden_case_both_routes(gpu_engine, name):
    from pygrank_amd import _lib as L
    assert L.entry("pgh_lanczos_close") is not None and L.entry("pgh_krylov_residuals") is not None
    dims = kc.CASES[name][4]
    fused, a = kc.check(gpu_engine, name, fused=True)
    assert fused.last_loop["spmv"] == dims and fused.last_loop["residual_passes"] >= 1 and fused.last_loop["converged"]
    assert fused.last_loop["dims"] == dims and fused.last_loop["iterations"] == fused.convergence.iteration
    plain, b = kc.check(gpu_engine, name, fused=False)
    assert plain.last_loop["spmv"] == dims and plain.last_loop["residual_passes"] == 0
    assert fused.convergence.iteration == plain.convergence.iteration
    assert kc.rel_linf(a, b) <= kc.BAR
    again, c = kc.run(gpu_engine, name, fused=True)
    assert np.array_equal(a, c) and again.last_loop["iterations"] == fused.last_loop["iterations"]     # deterministic sums: equal bits


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", SMALL)
def test_basis(gpu_engine, name, fused):
    kc.check_basis(gpu_engine, name, fused)


@pytest.mark.parametrize("fused", [True, False])
def test_too_rough_and_breakdown_raise(gpu_engine, fused):
    pg = gpu_engine
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for dims in kc.RAISING_DIMS:
            algo = pg.HeatKernel(t=3, krylov_dims=dims, normalization="symmetric", tol=1e-6, max_iters=kc.MAX_ITERS, fused=fused)
            with pytest.raises(Exception, match="is too rough to be meaningful") as raised:
                algo.rank(kc.path_graph(12), {0: 1})
            want = float(kc.fixture()[f"path12/bound/{dims}"])
            assert abs(float(str(raised.value).split("relative error ")[1].split(" ")[0]) - want) <= 1e-6 * want
        with pytest.raises(Exception, match="Krylov space of this personalization is exhausted"):
            pg.HeatKernel(t=3, krylov_dims=5, normalization="symmetric", fused=fused).rank(kc.path_graph(4), {0: 1})


def test_widest_slab_converges(gpu_engine):
    """krylov_dims = 64 on er10k: the widest slab the residual pass takes.  H is tridiagonal, so the first column of its first nine
    powers -- all that HeatKernel(t=3) adds up before it stops at iteration 10 -- touches the first ten Lanczos vectors only, and those
    do not depend on how many follow: the ranks and the iteration count are those of the 10-dimension case."""
    pg = gpu_engine
    A, directed, _ = kc.graph_of("er10k")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    algo = pg.HeatKernel(t=3, krylov_dims=64, normalization="symmetric", tol=1e-6, max_iters=kc.MAX_ITERS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ranks = np.asarray(algo.rank(graph, pg.to_signal(graph, kc.seeds_of("er10k"))).np, dtype=np.float64)
    assert algo.last_loop["converged"] and algo.last_loop["spmv"] == 64 and algo.last_loop["residual_passes"] >= 1
    assert algo.convergence.iteration == int(kc.fixture()["er10k/heat3/10/iters"])
    assert np.all(np.isfinite(ranks)) and kc.rel_linf(ranks, kc.fixture()["er10k/heat3/10/ranks"]) <= kc.BAR


def test_cached_basis_costs_no_product(gpu_engine):
    pg = gpu_engine
    name = "rmat12_sym/heat3/5"
    key = kc.CASES[name][0]
    A, directed, _ = kc.graph_of(key)
    graph = pg.AdjacencyWrapper(A, directed=directed)
    signal = pg.to_signal(graph, kc.seeds_of(key))
    pre = pg.preprocessor(normalization="symmetric", assume_immutability=True)
    store = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        first = kc.make_filter(pg, name, optimization_dict=store, preprocessor=pre)
        a = np.asarray(first.rank(graph, signal).np, dtype=np.float64)
        second = kc.make_filter(pg, name, optimization_dict=store, preprocessor=pre)
        b = np.asarray(second.rank(graph, signal).np, dtype=np.float64)
    assert first.last_loop["spmv"] == 5 and second.last_loop["spmv"] == 0 and np.array_equal(a, b)
    assert kc.rel_linf(a, kc.fixture()[name + "/ranks"]) <= kc.BAR


def test_inside_seed_oversampling(gpu_engine):
    """The setting of the reference's test_krylov_space_oversampling: a filter with krylov_dims inside pg.SeedOversampling."""
    pg = gpu_engine
    A, directed, _ = kc.graph_of("rmat12_sym")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    algorithm = pg.HeatKernel(t=5, krylov_dims=5, normalization="symmetric", renormalize=True)
    seeds = dict(list(kc.seeds_of("rmat12_sym").items())[:10])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ranks = np.asarray(pg.Normalize(pg.SeedOversampling(algorithm))(graph, seeds).np, dtype=np.float64)
    assert ranks.shape == (A.shape[0],) and np.all(np.isfinite(ranks)) and ranks.max() == 1.0
