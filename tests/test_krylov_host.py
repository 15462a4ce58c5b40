"""The Krylov-space filters on the host test double (no GPU) against the reference's recorded results (tests/golden/golden_krylov.npz).
The double lacks include/pgh_krylov.h, so every run here takes the backend-primitive route, whatever `fused` says.

Bases are compared up to 10 dimensions only: Lanczos without reorthogonalisation loses orthogonality in f32 storage from about 20
dimensions on (the generator's f32 evaluation on er10k at 20 dimensions: V^T V - I reaches 0.081 and H deviates by 0.022, while the ranks stay
within 1.3e-7 of the reference's; the reference's own f64 basis drifts the same way later, and its docstring warns "not stable yet").
At 5 and 10 dimensions V, H and V^T V - I are held to 8 times the deviation that the generator's f32 evaluation of the engine's route
recorded in the fixture (V 2.4e-8 to 2.7e-7, H 1.9e-9 to 7.5e-8)."""
import warnings

import numpy as np
import pytest

import krylov_common as kc

SMALL = [name for name, case in kc.CASES.items() if case[4] <= kc.BASIS_DIMS]


@pytest.mark.parametrize("name", list(kc.CASES))
def test_golden_case(host_engine, name):
    from pygrank_amd import _lib as L
    assert L.entry("pgh_lanczos_close") is None and L.entry("pgh_krylov_residuals") is None
    algo, _ = kc.check(host_engine, name)
    dims = kc.CASES[name][4]
    assert algo.last_loop["spmv"] == dims and algo.last_loop["dims"] == dims and algo.last_loop["converged"]
    assert algo.last_loop["residual_passes"] == 0 and algo.last_loop["iterations"] == algo.convergence.iteration
    for leftover in ("krylov_base", "krylov_H", "krylov_result", "Mpower", "coefficient", "prev_term"):
        assert not hasattr(algo, leftover)


@pytest.mark.parametrize("name", SMALL)
def test_basis(host_engine, name):
    kc.check_basis(host_engine, name)


def test_h_keeps_the_reference_quirk(host_engine):
    """krylov_space.py:35: base_norms[1:] on BOTH off-diagonals -- the last off-diagonal entry is the norm of the vector the loop
    never normalises, and the first norm appears nowhere."""
    _, H = kc.basis_of(host_engine, "weighted300/heat3/10")
    assert np.array_equal(np.diag(H, 1), np.diag(H, -1))
    want = kc.fixture()["weighted300/heat3/10/H"]
    assert np.allclose(np.diag(H, 1), np.diag(want, 1), rtol=1e-5, atol=0) and np.count_nonzero(np.triu(H, 2)) == 0


def test_warns_not_stable_yet(host_engine):
    pg = host_engine
    A, directed, _ = kc.graph_of("weighted300")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    with pytest.warns(UserWarning, match="not stable yet"):
        pg.HeatKernel(krylov_dims=5, normalization="symmetric").rank(graph, pg.to_signal(graph, kc.seeds_of("weighted300")))


@pytest.mark.parametrize("dims", kc.RAISING_DIMS)
def test_too_rough_raises(host_engine, dims):
    pg = host_engine
    algo = pg.HeatKernel(t=3, krylov_dims=dims, normalization="symmetric", tol=1e-6, max_iters=kc.MAX_ITERS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(Exception, match="is too rough to be meaningful") as raised:
            algo.rank(kc.path_graph(12), {0: 1})
    message, want = str(raised.value), float(kc.fixture()[f"path12/bound/{dims}"])
    assert message.startswith("Krylov approximation with estimated relative error ") and message.endswith(
        " > 0.01 is too rough to be meaningful (try on lager graphs)")
    assert abs(float(message.split("relative error ")[1].split(" ")[0]) - want) <= 1e-6 * want


def test_breakdown_raises(host_engine):
    """A 4-node path spans at most 4 Krylov dimensions: the fifth Lanczos vector vanishes.  (The reference divides by zero there.)"""
    pg = host_engine
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(Exception, match="Krylov space of this personalization is exhausted"):
            pg.HeatKernel(t=3, krylov_dims=5, normalization="symmetric").rank(kc.path_graph(4), {0: 1})


def test_powers_stay_under_the_bound(host_engine):
    """The contract of the reference's test_krylov_space (tests/test_filter_optimization.py:36-53) on rmat12_sym: with V, H of 5
    dimensions the bound lies under 0.01 and the errors of the first 100 powers of the (L2-normalised) personalization stay under the
    bound.  On this graph the reference's own later powers exceed its ONE-power bound (0.0010512 against 0.0013930 at the fourth
    power, measured with the reference under numpy), so "the bound" is krylov_error_bound(max_powers=100), held to the reference's
    value, and every power stays under it and under 0.01."""
    pg = host_engine
    A, directed, _ = kc.graph_of("rmat12_sym")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    M = pg.preprocessor(normalization="symmetric")(graph)
    signal = pg.to_signal(graph, kc.seeds_of("rmat12_sym"))
    p = signal.np / pg.sum(pg.abs(signal.np))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        V, H = pg.krylov_base(M, p, 5)
    one = pg.krylov_error_bound(V, H, M, p)
    many = pg.krylov_error_bound(V, H, M, p, max_powers=100)
    want = float(kc.fixture()["rmat12_sym/heat3/5/bound"])
    assert abs(one - want) <= 1e-4 * want and one < 0.01
    assert abs(many - 0.0013929787752659604) <= 1e-4 * many and one <= many < 0.01
    power, vec = np.eye(5), p / pg.dot(p, p) ** 0.5
    for _ in range(100):
        power, vec = power @ H, pg.conv(vec, M)
        approx = pg.krylov2original(V, power, 5)
        assert pg.Mabs(vec)(approx) <= many                 # the very evaluations krylov_error_bound took its maximum over
        assert pg.length(approx) == pg.length(p)


def test_scalar_v_quirk(host_engine):
    pg = host_engine
    H = np.diag(np.arange(1.0, 6.0))
    assert pg.sum(pg.krylov2original(0, H, 5)) == 0
    assert pg.sum(pg.krylov2original(2.0, H, 5)) == 10
    assert pg.length(pg.krylov2original(1, H, 5)) == 5


def test_arnoldi_iteration(host_engine):
    """pg.arnoldi_iteration against a numpy f64 restatement of the reference's loop on the downloaded operator.  The port runs in f32
    primitives: every axpy rounds to 2^-24 relative, a step takes up to five of them and a quotient by a norm of about 0.1 to 1, six
    steps chain -- some 6 * 5 * 10 * 6e-8 = 2e-5 at worst against unit-norm columns; 1e-5 is asked."""
    pg = host_engine
    A, directed, p = kc.graph_of("weighted300")
    M = pg.preprocessor(normalization="symmetric")(pg.AdjacencyWrapper(A, directed=directed))
    steps = 6
    Q, h = pg.arnoldi_iteration(M, p, steps)
    Q, h = np.asarray(Q, dtype=np.float64), np.asarray(h, dtype=np.float64)
    assert Q.shape == (300, steps) and h.shape == (steps + 1, steps)
    # the reference normalises the first vector by its L1 norm (self_normalize), every later one by its L2 norm
    assert abs(np.abs(Q[:, 0]).sum() - 1.0) <= 1e-6
    gram = Q[:, 1:].T @ Q[:, 1:]
    assert np.abs(gram - np.eye(steps - 1)).max() <= 1e-5
    # numpy restatement of the loop on the downloaded operator
    T = np.asarray(pg.preprocessor(normalization="symmetric")(pg.AdjacencyWrapper(A, directed=directed)).array.download_transposed().todense(),
                   dtype=np.float64)
    want_Q, want_h = [p / np.abs(p).sum()], np.zeros((steps + 1, steps))
    for k in range(1, steps):
        v = T @ want_Q[k - 1]
        for j in range(k):
            want_h[j, k - 1] = want_Q[j] @ v
            v = v - want_h[j, k - 1] * want_Q[j]
        want_h[k, k - 1] = (v @ v) ** 0.5
        want_Q.append(v / want_h[k, k - 1])
    assert np.abs(Q - np.stack(want_Q, axis=1)).max() <= 1e-5
    assert np.abs(h - want_h).max() <= 1e-5 * np.abs(want_h).max()
    # A Q[:, :n-1] = Q h on the columns the loop fills
    assert np.abs(T @ Q[:, :steps - 1] - Q @ h[:steps, :steps - 1]).max() <= 1e-5


def test_references(host_engine):
    pg = host_engine
    line = "Lanczos acceleration \\cite{susnjara2015accelerated} in the5-dimensional Krylov space"
    assert pg.HeatKernel(krylov_dims=5).references()[-1] == line
    assert line not in pg.HeatKernel().references()
    refs = pg.PageRankClosed(krylov_dims=5, coefficient_type="chebyshev", optimization_dict={}).references()
    assert refs.index("Chebyshev recurrence of the terms") < refs.index(line) < len(refs) - 1
    assert pg.HeatKernel(krylov_dims=5).cite().endswith(line)


@pytest.mark.parametrize("name", ["weighted300/heat3/10", "er10k/heat5cheb/10"])
def test_fused_flag_changes_nothing_on_the_double(host_engine, name):
    on, a = kc.run(host_engine, name, fused=True)
    off, b = kc.run(host_engine, name, fused=False)
    assert np.array_equal(a, b) and on.convergence.iteration == off.convergence.iteration
    assert on.last_loop == off.last_loop or (np.isnan(on.last_loop["last_error"]) and np.isnan(off.last_loop["last_error"]))


def test_cached_basis_costs_no_product(host_engine):
    pg = host_engine
    name = "rmat12_sym/heat3/5"
    key = kc.CASES[name][0]
    A, directed, _ = kc.graph_of(key)
    graph = pg.AdjacencyWrapper(A, directed=directed)
    signal = pg.to_signal(graph, kc.seeds_of(key))
    pre = pg.preprocessor(normalization="symmetric", assume_immutability=True)      # one graph object for both runs
    store = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        first = kc.make_filter(pg, name, optimization_dict=store, preprocessor=pre)
        a = np.asarray(first.rank(graph, signal).np, dtype=np.float64)
        assert first.last_loop["spmv"] == 5
        second = kc.make_filter(pg, name, optimization_dict=store, preprocessor=pre)
        b = np.asarray(second.rank(graph, signal).np, dtype=np.float64)
        plain, c = kc.run(pg, name)
    assert second.last_loop["spmv"] == 0 and np.array_equal(a, b) and np.array_equal(a, c)
    assert first.convergence.iteration == second.convergence.iteration == plain.convergence.iteration
    kept = store[pg.obj2id(signal)]["krylov"][5]
    assert sorted(kept["powers"]) == list(range(1, first.convergence.iteration)) and kept["powers"][1].shape == (5, 5)


def test_other_convergence_managers_step_one_at_a_time(host_engine):
    """A convergence manager of another class takes the hook protocol: one gemv and one has_converged per iteration."""
    pg = host_engine
    name = "weighted300/heat3/10"

    class Counting(pg.ConvergenceManager):
        calls = 0

        def has_converged(self, new_ranks):
            Counting.calls += 1
            return super().has_converged(new_ranks)
    algo, got = kc.run(pg, name, convergence=Counting(tol=1e-6, max_iters=kc.MAX_ITERS))
    assert Counting.calls == algo.convergence.iteration == int(kc.fixture()[name + "/iters"])
    assert kc.rel_linf(got, kc.fixture()[name + "/ranks"]) <= kc.BAR
    assert algo.last_loop["residual_passes"] == 0 and algo.last_loop["spmv"] == 10


def test_refusals(host_engine):
    pg = host_engine
    with pytest.raises(Exception):
        pg.PageRank(krylov_dims=5)                              # a recursive filter (tests/core_checks.py)
    A, directed, _ = kc.graph_of("weighted300")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    base = pg.HeatKernel(krylov_dims=5, optimization_dict={}, normalization="symmetric")
    with pytest.raises(Exception, match="krylov_dims"):
        base.rank_many(graph, kc.seeds_of("weighted300"), [pg.HeatKernel(t=2, normalization="symmetric")])
    with pytest.raises(Exception, match="krylov_dims"):
        pg.HeatKernel(optimization_dict={}, normalization="symmetric").probe_coefficients(
            graph, kc.seeds_of("weighted300"), [pg.HeatKernel(t=2, krylov_dims=5, normalization="symmetric")])


class _NumpyEntries:
    """Installs numpy stand-ins for the two entries of include/pgh_krylov.h on the host test double and counts their calls."""

    def __init__(self, decline_close_at=None, decline_residuals=False):
        self.calls = dict(pgh_lanczos_close=0, pgh_krylov_residuals=0)
        self.decline_close_at, self.decline_residuals = decline_close_at, decline_residuals

    def __enter__(self):
        from pygrank_amd import _lib as L
        self.lib = L.lib()
        assert L.entry("pgh_lanczos_close") is None
        entries = kc.numpy_entries(self.lib)

        def close(*args):
            self.calls["pgh_lanczos_close"] += 1
            return 2 if self.calls["pgh_lanczos_close"] == self.decline_close_at else entries["pgh_lanczos_close"](*args)

        def residuals(*args):
            self.calls["pgh_krylov_residuals"] += 1
            return 2 if self.decline_residuals else entries["pgh_krylov_residuals"](*args)
        self.saved = self.lib._pgh_krylov_entries
        self.lib._pgh_krylov_entries = dict(pgh_lanczos_close=close, pgh_krylov_residuals=residuals)
        return self

    def __exit__(self, *exc):
        self.lib._pgh_krylov_entries = self.saved


@pytest.mark.parametrize("name", list(kc.CASES))
def test_fused_route_with_numpy_entries(host_engine, name):
    """The fused route's host side on the double's resident iterates, the two entries replaced by numpy evaluations of their header:
    one close per Lanczos step, one residual pass per 64 iterations."""
    dims = kc.CASES[name][4]
    with _NumpyEntries() as entries:
        algo, fused = kc.check(host_engine, name)
        passes = -(-(algo.convergence.iteration - 1) // 64)
        assert entries.calls == dict(pgh_lanczos_close=dims, pgh_krylov_residuals=passes)
        assert algo.last_loop["spmv"] == dims and algo.last_loop["residual_passes"] == passes and algo.last_loop["converged"]
    plain, primitive = kc.run(host_engine, name, fused=False)
    assert algo.convergence.iteration == plain.convergence.iteration and kc.rel_linf(fused, primitive) <= kc.BAR


@pytest.mark.parametrize("name", SMALL)
def test_fused_basis_with_numpy_entries(host_engine, name):
    with _NumpyEntries() as entries:
        kc.check_basis(host_engine, name)
        assert entries.calls["pgh_lanczos_close"] == kc.CASES[name][4]


def test_second_chunk_of_residuals(host_engine):
    """A run of more than 64 iterations takes further residual passes, one per 64 iterations: PageRankClosed(0.95) at tol 1e-9."""
    pg = host_engine
    A, directed, _ = kc.graph_of("rmat12_sym")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    signal = pg.to_signal(graph, kc.seeds_of("rmat12_sym"))
    make = lambda fused: pg.PageRankClosed(0.95, krylov_dims=10, normalization="symmetric", tol=1e-9, max_iters=kc.MAX_ITERS, fused=fused)  # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with _NumpyEntries() as entries:
            fused = make(True)
            a = np.asarray(fused.rank(graph, signal).np, dtype=np.float64)
            passes = -(-(fused.convergence.iteration - 1) // 64)
            assert fused.convergence.iteration > 65 and entries.calls["pgh_krylov_residuals"] == passes >= 2
            assert fused.last_loop["residual_passes"] == passes
        plain = make(False)
        b = np.asarray(plain.rank(graph, signal).np, dtype=np.float64)
    assert plain.convergence.iteration == fused.convergence.iteration and kc.rel_linf(a, b) <= kc.BAR


def test_max_iters_and_end_modulo(host_engine):
    """The stopping rule of ConvergenceManager on the fused loop: out of iterations raises, end_modulo postpones the stop."""
    pg = host_engine
    name = "weighted300/heat3/10"
    want = int(kc.fixture()[name + "/iters"])
    with _NumpyEntries():
        with pytest.raises(Exception, match="Could not converge within 7 iterations"):
            kc.run(pg, name, convergence=pg.ConvergenceManager(tol=1e-6, max_iters=7))
        algo, _ = kc.run(pg, name, convergence=pg.ConvergenceManager(tol=1e-6, max_iters=kc.MAX_ITERS, end_modulo=7))
        assert algo.convergence.iteration == -(-want // 7) * 7
        counted, _ = kc.run(pg, name, convergence=pg.ConvergenceManager(error_type="iters", max_iters=12))
        assert counted.convergence.iteration == 12 and counted.last_loop["residual_passes"] == 0
    plain, _ = kc.run(pg, name, fused=False, convergence=pg.ConvergenceManager(tol=1e-6, max_iters=kc.MAX_ITERS, end_modulo=7))
    assert plain.convergence.iteration == algo.convergence.iteration


@pytest.mark.parametrize("at", [1, 3])
def test_close_declining_restarts_in_primitives(host_engine, at):
    name = "weighted300/heat3/10"
    with _NumpyEntries(decline_close_at=at) as entries:
        algo, got = kc.check(host_engine, name)
        assert entries.calls["pgh_lanczos_close"] == at          # nothing fused in the basis after the decline
    plain, want = kc.run(host_engine, name, fused=False)
    assert algo.convergence.iteration == plain.convergence.iteration and np.array_equal(got, want)


def test_residuals_declining_goes_on_one_iteration_at_a_time(host_engine):
    name = "weighted300/heat3/10"
    with _NumpyEntries(decline_residuals=True):
        algo, got = kc.check(host_engine, name)
        assert algo.last_loop["residual_passes"] == 0
