"""The first step of a seed-set PageRank run over the seeds' out-edges (pygrank_amd/csrc/pgh_push.hip) on graphs small enough to
enumerate: RMAT scales 10-14 uploaded with PGH_PB_FORCE=1 and run with the general launch sequence (PGH_SMALL_TAIL=0: up to 12 288
rows a step is otherwise one one-workgroup launch, which the pushed step does not replace), one scale-12 graph under the defaults.
PGH_PB_FORCE lifts the size heuristics of the cold image, but a block of fewer sources than the LDS hot cache holds (29 696) has no
cold entry to put into one: on scales 10-14 the dense step is k_bsf_partial + k_bsf_combine with the separate residual, and the
pushed step closes with res_mode 0.  Two scale-16 graphs (65 536 sources) therefore stand beside them: the smallest RMAT size
at which the cold image exists, so that the pushed step is also held against k_pb_finish and closes into the in-kernel residual.

Every case is held to
  * oracle/ref_loops.pagerank on the engine's own stored matrix (download_transposed): rel-Linf <= 1e-6, equal iteration counts
    (the bounds of the existing parity tests),
  * the same run with PGH_SEED_PUSH=0: equal iteration counts, equal SpMV counts, rel-Linf <= 1e-6,
  * a second run of the same path: the same bits,
and says which path it expects: bit 3 of pgh_loop_result::flags is set by a run whose step 1 went over the out-edges.  One check
looks at step 1 alone: a run stopped after one step against numpy a * M^T x0 + b * p and against the dense step of the resident-iterate
entry points (pgh_resident_in / pgh_resident_step / pgh_resident_out)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ref_loops as orc, rmat_np

pytestmark = pytest.mark.gpu

PUSHED = 8                                     # flags: step 1 went over the seeds' out-edges
ENV = ("PGH_PB", "PGH_PB_FORCE", "PGH_PB_HEAVY", "PGH_PB_HUBMAX", "PGH_BLOCKS", "PGH_SEED_PUSH", "PGH_SEED_PUSH_K", "PGH_SEED_PUSH_C", "PGH_SMALL_TAIL")
MAX_SEEDS = 4096                               # K of pgh_push.hip
ALPHA = 0.85


@pytest.fixture(scope="module")
def pg():
    import pygrank_amd
    from pygrank_amd import _lib
    pygrank_amd.load_backend("hip")
    assert _lib.runtime_name().startswith("hip:")
    return pygrank_amd


@contextlib.contextmanager
def _env(**values):
    saved = {k: os.environ.get(k) for k in ENV}
    try:
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(values)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def _adjacency(g):
    from pygrank_amd.preprocessing import Adjacency
    from pygrank_amd.signals import _IdentityMap
    adj = Adjacency(g)
    adj._pygrank_preprocessed = {"hip": adj}
    adj._pygrank_node2id = _IdentityMap(g.shape[0])
    adj.is_directed = lambda: True
    return adj


class Graph:
    """An uploaded graph, its raw adjacency and its stored matrix as the oracle takes it."""

    def __init__(self, scale, normalization="col", weights="few", force_image=True, seed=2):
        """weights: "rmat" = the generator's multiplicities (value-free or valued, as the engine's census of them decides), "few" =
        multiplicities 1, 2 and 3 thinned until the value-free image is sure to take them (expanded entries <= 1.25 nnz), "real" =
        uniform in [0.5, 2)."""
        from pygrank_amd.device import DeviceGraph
        self.A = rmat_np.rmat_csr(scale, 16, seed=seed)          # duplicate edges are summed: weights are multiplicities
        if weights == "real":
            rng = np.random.default_rng(5)
            self.A = sp.csr_array((rng.uniform(0.5, 2.0, self.A.nnz), self.A.indices, self.A.indptr), shape=self.A.shape)
        elif weights == "few":
            data = np.ones(self.A.nnz)
            data[::7], data[::31] = 2.0, 3.0
            self.A = sp.csr_array((data, self.A.indices, self.A.indptr), shape=self.A.shape)
        with _env(**(dict(PGH_PB="1", PGH_PB_FORCE="1") if force_image else {})):
            self.g = DeviceGraph.from_adjacency(self.A, normalization)
        self.general = force_image                               # run with PGH_SMALL_TAIL=0
        self.fmt = self.g.format()
        self.weights = weights
        self.adj = _adjacency(self.g)
        self.MT = sp.csr_array(self.g.download_transposed().astype(np.float64))
        self.M = self.MT.T
        self.n = self.A.shape[0]
        self.out_deg = np.diff(self.A.indptr)
        self.in_deg = np.bincount(self.A.indices, minlength=self.n)

    def seeds(self, count, seed=1, among=None):
        cand = np.flatnonzero(self.out_deg > 0) if among is None else among
        p = np.zeros(self.n)
        p[np.sort(np.random.default_rng(seed).choice(cand, count, replace=False))] = 1.0
        return p


@pytest.fixture(scope="module")
def graphs(pg):
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = {"col10": lambda: Graph(10), "col13": lambda: Graph(13), "col14": lambda: Graph(14),
                          "sym12": lambda: Graph(12, "symmetric"), "real12": lambda: Graph(12, weights="real"),
                          "rmat11": lambda: Graph(11, weights="rmat"), "plain12": lambda: Graph(12, force_image=False),
                          "cold16": lambda: Graph(16), "coldsym16": lambda: Graph(16, "symmetric", weights="real")}[key]()
        return cache[key]
    return get


def _run(pg, G, p, push=True, **kw):
    kw = dict(dict(error_type=pg.L1, tol=1e-6, max_iters=500), **kw)
    ranker = pg.PageRank(ALPHA, **kw)
    switches = {k: v for k, v in os.environ.items() if k in ("PGH_SEED_PUSH_K", "PGH_SEED_PUSH_C")}
    if G.general:
        switches["PGH_SMALL_TAIL"] = "0"
    with _env(PGH_SEED_PUSH="1" if push else "0", **switches):
        ranks = ranker.rank(G.adj, p.copy())
        got = np.asarray(ranks.np, dtype=np.float64)
    return got, int(ranker.convergence.iteration), dict(ranker.last_loop)


def _check(pg, G, p, pushed, oracle_kw=None, **kw):
    """The four checks of the module docstring for one (graph, personalization, stopping rule); returns the pushed run's figures."""
    got, iters, loop = _run(pg, G, p, **kw)
    assert bool(loop["flags"] & PUSHED) == pushed, (loop, G.fmt)
    okw = oracle_kw if oracle_kw is not None else dict(error_type="l1", tol=1e-6, max_iters=500)
    want, want_iters = orc.pagerank(G.M, p, alpha=ALPHA, **okw)
    err = _rel(got, want)
    print(f"seed push: pushed={pushed} iterations={iters} (oracle {want_iters}) rel-Linf={err:.3e} loop={loop}")
    assert iters == want_iters, (iters, want_iters)
    assert err <= 1e-6, err
    got0, iters0, loop0 = _run(pg, G, p, push=False, **kw)
    assert not (loop0["flags"] & PUSHED)
    assert iters0 == iters and loop0["spmv"] == loop["spmv"], (loop0, loop)
    assert _rel(got, got0) <= 1e-6, _rel(got, got0)
    again, iters2, _ = _run(pg, G, p, **kw)
    assert iters2 == iters and np.array_equal(again, got)
    return got, iters, loop


@pytest.mark.parametrize("key", ["col10", "col13", "col14", "cold16"])
def test_one_seed(pg, graphs, key):
    G = graphs(key)
    _check(pg, G, G.seeds(1, seed=3), True)


@pytest.mark.parametrize("key", ["col10", "col13", "col14", "sym12", "real12", "rmat11", "cold16", "coldsym16"])
def test_hundred_seeds(pg, graphs, key):
    """"col" and "symmetric" normalisation; value-free multigraphs, the generator's multiplicities as values, real weights."""
    G = graphs(key)
    _, _, loop = _check(pg, G, G.seeds(100), True)
    if key.startswith("cold"):                               # bits 0-2 are the dense form's: the in-kernel residual, never paused
        assert loop["flags"] & 7 == 6, loop


def test_weighted_personalization(pg, graphs):
    G = graphs("sym12")
    p = G.seeds(37, seed=9) * np.random.default_rng(3).uniform(0.1, 5.0, G.n)
    _check(pg, G, p, True)


def test_seed_without_out_edges(pg, graphs):
    G = graphs("col13")
    dangling = np.flatnonzero((G.out_deg == 0) & (G.in_deg > 0))
    assert len(dangling) >= 3
    p = G.seeds(20)
    p[dangling[:3]] = 1.0
    _check(pg, G, p, True)
    only = np.zeros(G.n)
    only[dangling[0]] = 1.0                                  # no out-edge at all: step 1 is b * p
    _check(pg, G, only, True)


def test_isolated_seed(pg, graphs):
    G = graphs("col13")
    isolated = np.flatnonzero((G.out_deg == 0) & (G.in_deg == 0))
    assert len(isolated) >= 2
    p = G.seeds(20)
    p[isolated[:2]] = 1.0
    _check(pg, G, p, True)


def test_more_seeds_than_the_list_takes_the_dense_step(pg, graphs):
    G = graphs("col13")
    _check(pg, G, G.seeds(MAX_SEEDS, seed=4, among=np.arange(G.n)), True)
    _check(pg, G, G.seeds(MAX_SEEDS + 1, seed=4, among=np.arange(G.n)), False)


def test_hub_seed_takes_the_dense_step(pg, graphs):
    """The seeds' out-degrees against C: the graph's largest out-degree is far below the default, so the test lowers the bound to it."""
    G = graphs("col13")
    hub = int(np.argmax(G.out_deg))
    p = np.zeros(G.n)
    p[hub] = 1.0
    saved = os.environ.get("PGH_SEED_PUSH_C")
    try:
        os.environ["PGH_SEED_PUSH_C"] = str(int(G.out_deg[hub]))
        _check(pg, G, p, True)
        os.environ["PGH_SEED_PUSH_C"] = str(int(G.out_deg[hub]) - 1)
        _check(pg, G, p, False)
    finally:
        if saved is None:
            os.environ.pop("PGH_SEED_PUSH_C", None)
        else:
            os.environ["PGH_SEED_PUSH_C"] = saved


def test_signed_personalization_takes_the_dense_step(pg, graphs):
    G = graphs("col13")
    p = G.seeds(50)
    p[np.flatnonzero(p)[::7]] = -0.25
    _check(pg, G, p, False)


def test_max_iters_reached_at_step_one(pg, graphs):
    G = graphs("col13")
    got, iters, loop = _check(pg, G, G.seeds(100), True, oracle_kw=dict(error_type="iters", max_iters=2), error_type="iters", max_iters=2)
    assert iters == 2 and loop["spmv"] == 1


def test_loose_tolerance_converges_at_step_one(pg, graphs):
    G = graphs("col13")
    got, iters, loop = _check(pg, G, G.seeds(100), True, oracle_kw=dict(error_type="l1", tol=10.0, max_iters=500), tol=10.0)
    assert iters == 2 and loop["spmv"] == 1 and loop["converged"]


def test_graph_without_a_cold_image(pg, graphs):
    """Scale 12 under the default heuristics: one column block, no cold image -- step, residual and close of such a graph are one
    one-workgroup launch, which the pushed step does not replace: the run takes the dense step, with the same results."""
    G = graphs("plain12")
    assert "propagation-blocking image" not in G.fmt, G.fmt
    _check(pg, G, G.seeds(100), False)


def test_step_one_alone(pg, graphs):
    """One step of the pushed path (max_iters = 2) against numpy fp64 a * M^T x0 + b * p on the stored matrix, row by row, and against
    the dense step of the resident-iterate entry points.

    The bound, per row, relative to the sum of |terms|: the image's value against the stored one (source scale: 1 rounding, the stored
    value: 1), x0 times the source scale (1), times the multiplicity (1), the row sum as f32 (1; the fixed-point sum itself keeps 41
    bits), alpha and 1 - alpha as f32 (2), the two products and the sum of the epilogue (3), the quotient as f32 and its product
    on the way out (2): 12 roundings of eps32 / 2 each = 6 eps32.  Two evaluations of that kind differ by at most twice as much."""
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceVector
    G = graphs("col10")
    eps32 = float(np.finfo(np.float32).eps)
    for p in (G.seeds(1, seed=3), G.seeds(100), G.seeds(300, seed=8) * np.random.default_rng(1).uniform(0.2, 3.0, G.n)):
        got, iters, loop = _run(pg, G, p, error_type="iters", max_iters=2)
        assert iters == 2 and loop["spmv"] == 1 and loop["flags"] & PUSHED, loop
        norm = np.abs(p).sum()
        x0 = (p.astype(np.float32) / np.float32(norm)).astype(np.float64)
        y = ALPHA * (G.MT @ x0) + (1 - ALPHA) * x0
        want = y / y.sum() * norm                            # the quotient of the step, preserve_norm
        bound = 6 * eps32 * (ALPHA * (abs(G.MT) @ x0) + (1 - ALPHA) * x0) / y.sum() * norm + 1e-30
        assert np.all(np.abs(got - want) <= bound), float(np.max(np.abs(got - want) / bound))
        assert np.array_equal(got == 0, want == 0)           # exactly the seeds and their out-neighbours
        # the dense step on the same operands
        g = G.g
        assert g._resident_lengths()
        x_res = g._resident_copy(pg.to_array(x0))
        y_int = DeviceVector.empty(g._n_int)
        yg = DeviceVector.empty(g._n_gather) if g._n_gather else None
        s = C.c_double()
        L.check(L.lib().pgh_resident_step(g._h, 1, x_res.y._h, x_res.xg._h if x_res.xg is not None else None, ALPHA, x_res.y._h, 1 - ALPHA,
                                          None, None, y_int._h, yg._h if yg is not None else None, C.byref(s)))
        out = DeviceVector.empty(G.n)
        L.check(L.lib().pgh_resident_out(g._h, y_int._h, norm / s.value, out._h))
        dense = np.asarray(out, dtype=np.float64)
        assert np.all(np.abs(got - dense) <= 2 * bound), float(np.max(np.abs(got - dense) / bound))


def test_which_graphs_have_a_cold_image(graphs):
    for key in ("col10", "col13", "col14", "sym12", "real12", "rmat11"):
        assert "propagation-blocking image" not in graphs(key).fmt, (key, graphs(key).fmt)
    for key in ("cold16", "coldsym16"):
        assert "propagation-blocking image" in graphs(key).fmt, (key, graphs(key).fmt)
    for key in ("col10", "col13", "col14", "sym12", "real12", "cold16", "coldsym16"):      # value-free and valued images where meant
        assert ("f32-valued" in graphs(key).fmt) == (graphs(key).weights == "real"), (key, graphs(key).fmt)
