"""Step 2's cold tail of a seed-set PageRank run over the out-edges (pygrank_amd/csrc/pgh_push.hip: k_push_plan2, k_push_expand2,
k_push_accum2; pgh_bsf.hip: k_bsf_combine_tail) on RMAT scale 16 / ef 16 uploaded with PGH_PB=1 PGH_PB_FORCE=1 and run with
PGH_SMALL_TAIL=0: the smallest size at which the cold image exists, so the smallest at which step 2 has a cold tail to push.  One
value-free graph ("few": multiplicities 1, 2, 3, column-normalised) and one valued graph ("real": uniform weights, symmetric
normalisation), the shapes and the bounds of tests/test_gpu_seed_push.py.

A run is held to
  * oracle/ref_loops.pagerank on the engine's own stored matrix (download_transposed): rel-Linf <= 1e-6, equal iteration counts,
  * the same run with PGH_SEED_PUSH2=0: equal iteration counts, equal SpMV counts, rel-Linf <= 1e-6,
  * a second run of the same path: the same bits,
and says which path it expects: bit 4 of pgh_loop_result::flags is set by a run whose step 2 pushed its cold tail (bit 3: step 1
went over the seeds' out-edges).  Which sources are cold is read off the engine: the resident form of 1 .. n gives the internal id of
every node, pgh_graph_gather_layout the block size, pgh_graph_hot_prefix the slots of a block that stay in the hot cache."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ref_loops as orc
from test_gpu_seed_push import ALPHA, PUSHED, Graph, _rel, _run as _run_push

pytestmark = pytest.mark.gpu

TAIL = 16                                      # flags: step 2's cold tail went over the out-edges
ENV2 = ("PGH_SEED_PUSH2", "PGH_SEED_PUSH_C2", "PGH_SEED_PUSH_C", "PGH_SEED_PUSH_K")


@pytest.fixture(scope="module")
def pg():
    import pygrank_amd
    from pygrank_amd import _lib
    pygrank_amd.load_backend("hip")
    assert _lib.runtime_name().startswith("hip:")
    return pygrank_amd


@contextlib.contextmanager
def _env2(**values):
    saved = {k: os.environ.get(k) for k in ENV2}
    try:
        for k in ENV2:
            os.environ.pop(k, None)
        os.environ.update(values)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Layout:
    """Where the engine put every node of a graph: internal id, and whether that slot lies beyond the hot part of its block."""

    def __init__(self, pg, G):
        from pygrank_amd import _lib as L
        g = G.g
        assert g._resident_lengths()
        ids = g._resident_copy(pg.to_array(np.arange(1, G.n + 1, dtype=np.float64)))      # n = 65 536: exact in f32
        y = np.asarray(ids.y, dtype=np.float64)
        at = np.flatnonzero(y)
        self.new_id = np.full(G.n, -1, dtype=np.int64)
        self.new_id[np.rint(y[at]).astype(np.int64) - 1] = at
        assert np.all(self.new_id >= 0)
        nb, blk, hot = C.c_int32(), C.c_int64(), C.c_int32()
        L.check(L.lib().pgh_graph_gather_layout(g._h, C.byref(nb), C.byref(blk), None))
        L.check(L.lib().pgh_graph_hot_prefix(g._h, C.byref(hot)))
        assert hot.value > 0, G.fmt                          # a hot-only stream: every cold entry lives in the cold image
        self.cold = (self.new_id % blk.value) >= hot.value
        self.cold_source = self.cold & (G.out_deg > 0)


@pytest.fixture(scope="module")
def graphs(pg):
    cache = {}

    def get(key):
        if key not in cache:
            G = {"few16": lambda: Graph(16), "real16": lambda: Graph(16, "symmetric", weights="real"),
                 "plain12": lambda: Graph(12, force_image=False)}[key]()
            if key != "plain12":
                assert "propagation-blocking image" in G.fmt, G.fmt
                G.layout = Layout(pg, G)
                G.AT = G.A.T.tocsr()                          # in-edges (rows of the transpose)
            cache[key] = G
        return cache[key]
    return get


def _run(pg, G, p, tail=True, c2=None, c=None, **kw):
    env = {"PGH_SEED_PUSH2": "1" if tail else "0"}
    if c2 is not None:
        env["PGH_SEED_PUSH_C2"] = str(c2)
    if c is not None:
        env["PGH_SEED_PUSH_C"] = str(c)
    with _env2(**env):
        return _run_push(pg, G, p, push=True, **kw)


def _twin(pg, G, p, tail_expected, got, iters, loop, **kw):
    """The same run with PGH_SEED_PUSH2=0: never bit 4, equal counts, rel-Linf <= 1e-6."""
    assert bool(loop["flags"] & TAIL) == tail_expected, (loop, G.fmt)
    got0, iters0, loop0 = _run(pg, G, p, tail=False, **kw)
    assert not (loop0["flags"] & TAIL), loop0
    assert (loop0["flags"] & PUSHED) == (loop["flags"] & PUSHED), (loop0, loop)
    assert iters0 == iters and loop0["spmv"] == loop["spmv"] and loop0["converged"] == loop["converged"], (loop0, loop)
    err = _rel(got, got0)
    print(f"seed push 2: tail={tail_expected} iterations={iters} spmv={loop['spmv']} against PGH_SEED_PUSH2=0 rel-Linf={err:.3e} loop={loop}")
    assert err <= 1e-6, err
    return got0


def _check(pg, G, p, tail_expected=True, pushed=True, oracle_kw=None, **kw):
    got, iters, loop = _run(pg, G, p, **kw)
    assert bool(loop["flags"] & PUSHED) == pushed, (loop, G.fmt)
    okw = oracle_kw if oracle_kw is not None else dict(error_type="l1", tol=1e-6, max_iters=500)
    want, want_iters = orc.pagerank(G.M, p, alpha=ALPHA, **okw)
    err = _rel(got, want)
    print(f"seed push 2: iterations={iters} (oracle {want_iters}) rel-Linf={err:.3e}")
    assert iters == want_iters, (iters, want_iters)
    assert err <= 1e-6, err
    got0 = _twin(pg, G, p, tail_expected, got, iters, loop, **kw)
    again, iters2, loop2 = _run(pg, G, p, **kw)
    assert iters2 == iters and np.array_equal(again, got) and loop2["flags"] == loop["flags"]
    return got, got0, iters, loop


# ---- 1. parity of a whole run
@pytest.mark.parametrize("key", ["few16", "real16"])
@pytest.mark.parametrize("count", [1, 5, 100])
def test_whole_run(pg, graphs, key, count):
    G = graphs(key)
    _, _, _, loop = _check(pg, G, G.seeds(count, seed=3 if count == 1 else 1))
    assert loop["flags"] & 7 == 6, loop                       # the in-kernel residual is the rule of the dense steps, never paused


# ---- 2. step 2 alone
@pytest.mark.parametrize("key", ["few16", "real16"])
def test_step_two_alone(pg, graphs, key):
    """Two steps of the pushed path (max_iters = 3) against numpy fp64: two applications of a * M^T x + b * p on the stored matrix with
    the L1 quotient between them, row by row, within the per-row bound of test_gpu_seed_push.test_step_one_alone (6 eps32 of the sum
    of |terms| of the step), and against two dense steps of the resident-iterate entry points within twice that."""
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceVector
    G = graphs(key)
    eps32 = float(np.finfo(np.float32).eps)
    for p in (G.seeds(1, seed=3), G.seeds(100), G.seeds(300, seed=8) * np.random.default_rng(1).uniform(0.2, 3.0, G.n)):
        got, iters, loop = _run(pg, G, p, error_type="iters", max_iters=3)
        assert iters == 3 and loop["spmv"] == 2 and loop["flags"] & PUSHED and loop["flags"] & TAIL, loop
        norm = np.abs(p).sum()
        x0 = (p.astype(np.float32) / np.float32(norm)).astype(np.float64)
        y1 = ALPHA * (G.MT @ x0) + (1 - ALPHA) * x0
        x1 = y1 / y1.sum()
        y2 = ALPHA * (G.MT @ x1) + (1 - ALPHA) * x0
        want = y2 / y2.sum() * norm
        bound = 6 * eps32 * (ALPHA * (abs(G.MT) @ x1) + (1 - ALPHA) * x0) / y2.sum() * norm + 1e-30
        worst = float(np.max(np.abs(got - want) / bound))
        print(f"seed push 2: step 2 alone on {key}: worst row at {worst:.3f} of the bound")
        assert np.all(np.abs(got - want) <= bound), worst
        assert np.array_equal(got == 0, want == 0)
        # two dense steps on the same operands
        g = G.g
        assert g._resident_lengths()
        x_res = g._resident_copy(pg.to_array(x0))
        ya, yb = DeviceVector.empty(g._n_int), DeviceVector.empty(g._n_int)
        ga = DeviceVector.empty(g._n_gather) if g._n_gather else None
        gb = DeviceVector.empty(g._n_gather) if g._n_gather else None
        s1, s2 = C.c_double(), C.c_double()
        L.check(L.lib().pgh_resident_step(g._h, 1, x_res.y._h, x_res.xg._h if x_res.xg is not None else None, ALPHA, x_res.y._h, 1 - ALPHA,
                                          None, None, ya._h, ga._h if ga is not None else None, C.byref(s1)))
        L.check(L.lib().pgh_resident_step(g._h, 1, ya._h, ga._h if ga is not None else None, ALPHA * (1.0 / s1.value), x_res.y._h, 1 - ALPHA,
                                          None, None, yb._h, gb._h if gb is not None else None, C.byref(s2)))
        out = DeviceVector.empty(G.n)
        L.check(L.lib().pgh_resident_out(g._h, yb._h, norm / s2.value, out._h))
        dense = np.asarray(out, dtype=np.float64)
        assert np.all(np.abs(got - dense) <= 2 * bound), float(np.max(np.abs(got - dense) / bound))


# ---- 3. the edges of the decision
@pytest.mark.parametrize("key", ["few16", "real16"])
def test_bound_of_one_item_takes_the_dense_tail(pg, graphs, key):
    G = graphs(key)
    p = G.seeds(100)
    got, iters, loop = _run(pg, G, p, c2=1)
    assert loop["flags"] & PUSHED and not (loop["flags"] & TAIL), loop
    got0, iters0, loop0 = _run(pg, G, p, tail=False)
    assert iters0 == iters and loop0["spmv"] == loop["spmv"] and np.array_equal(got, got0), (loop, loop0)
    # ... and the exact count of the items decides
    lay = G.layout
    x1 = (G.MT @ p) + p
    stored_out = np.bincount(G.MT.indices, minlength=G.n)    # entries of the stored matrix by source
    items = int(stored_out[(x1 != 0) & lay.cold].sum())
    assert items > 1
    _, _, loop = _run(pg, G, p, c2=items)
    assert loop["flags"] & TAIL, (items, loop)
    got1, _, loop = _run(pg, G, p, c2=items - 1)
    assert not (loop["flags"] & TAIL) and np.array_equal(got1, got0), (items, loop)


def test_seed_set_too_large_for_step_one(pg, graphs):
    G = graphs("few16")
    p = G.seeds(4097, seed=4, among=np.arange(G.n))          # more seeds than k_push_plan sorts
    got, got0, _, loop = _check(pg, G, p, tail_expected=False, pushed=False)
    assert not (loop["flags"] & (PUSHED | TAIL)) and np.array_equal(got, got0), loop


@pytest.mark.parametrize("key", ["few16", "real16"])
def test_out_neighbours_all_hot(pg, graphs, key):
    """Seeds that are hot sources and point at hot sources only: the list stays empty and the tail qualifies with zero items."""
    G = graphs(key)
    lay = G.layout
    cold_targets = G.A @ lay.cold.astype(np.float64)         # out-neighbours that are cold
    cand = np.flatnonzero((G.out_deg > 0) & (cold_targets == 0) & ~lay.cold)
    assert len(cand) >= 3, len(cand)
    p = np.zeros(G.n)
    p[cand[:3]] = 1.0
    x1 = (G.MT @ p) + p
    assert not np.any((x1 != 0) & lay.cold)
    _check(pg, G, p)


@pytest.mark.parametrize("key", ["few16", "real16"])
def test_seed_without_in_edges(pg, graphs, key):
    G = graphs(key)
    cand = np.flatnonzero((G.in_deg == 0) & (G.out_deg > 0))
    assert len(cand) >= 2
    p = G.seeds(20)
    p[cand[:2]] = 1.0
    _check(pg, G, p)
    only = np.zeros(G.n)
    only[cand[0]] = 1.0
    _check(pg, G, only)


@pytest.mark.parametrize("key", ["few16", "real16"])
def test_seed_that_is_a_cold_source(pg, graphs, key):
    G = graphs(key)
    cand = np.flatnonzero(G.layout.cold_source)
    assert len(cand) >= 4
    p = np.zeros(G.n)
    p[cand[[0, len(cand) // 3, len(cand) // 2, -1]]] = 1.0
    _check(pg, G, p)


# ---- 4. a run that ends at step 2
@pytest.mark.parametrize("key", ["few16", "real16"])
def test_run_ends_at_step_two(pg, graphs, key):
    G = graphs(key)
    p = G.seeds(100)
    # the L1 residuals of steps 1 and 2 of this run, to put a tolerance between them
    x0 = p / p.sum()
    y1 = ALPHA * (G.MT @ x0) + (1 - ALPHA) * x0
    x1 = y1 / y1.sum()
    y2 = ALPHA * (G.MT @ x1) + (1 - ALPHA) * x0
    x2 = y2 / y2.sum()
    r1, r2 = np.abs(x1 - x0).sum(), np.abs(x2 - x1).sum()
    assert r2 < 0.95 * r1, (r1, r2)
    tol = float(np.sqrt(r1 * r2))
    _, _, iters, loop = _check(pg, G, p, oracle_kw=dict(error_type="l1", tol=tol, max_iters=500), tol=tol)
    assert iters == 3 and loop["spmv"] == 2 and loop["converged"], loop
    _, _, iters, loop = _check(pg, G, p, oracle_kw=dict(error_type="iters", max_iters=3), error_type="iters", max_iters=3)
    assert iters == 3 and loop["spmv"] == 2, loop
    # max_iters = 2: the run never reaches step 2 and nothing of the tail is enqueued
    _, _, iters, loop = _check(pg, G, p, tail_expected=False, oracle_kw=dict(error_type="iters", max_iters=2), error_type="iters",
                               max_iters=2)
    assert iters == 2 and loop["spmv"] == 1, loop


# ---- 5. nothing left behind
@pytest.mark.parametrize("key", ["few16", "real16"])
def test_nothing_left_behind(pg, graphs, key):
    G = graphs(key)
    pa, pb = G.seeds(100, seed=11), G.seeds(37, seed=12) * np.random.default_rng(2).uniform(0.1, 5.0, G.n)
    twins = {}
    first = {}
    for turn, (name, p) in enumerate([("a", pa), ("b", pb), ("a", pa), ("b", pb)]):
        got, iters, loop = _run(pg, G, p)
        assert loop["flags"] & TAIL, (turn, loop)
        if name not in twins:
            twins[name] = _twin(pg, G, p, True, got, iters, loop)
            first[name] = got
        assert np.array_equal(got, first[name]), (turn, name)
        assert _rel(got, twins[name]) <= 1e-6
    # a seed set whose tail does not qualify finds the scratch and the list re-armed ...
    got, iters, loop = _run(pg, G, pa, c2=1)
    assert not (loop["flags"] & TAIL)
    _twin(pg, G, pa, False, got, iters, loop)
    big = G.seeds(4097, seed=4, among=np.arange(G.n))
    got, iters, loop = _run(pg, G, big)
    _twin(pg, G, big, False, got, iters, loop)
    # ... and so does the next one that does
    got, iters, loop = _run(pg, G, pa)
    assert loop["flags"] & TAIL and np.array_equal(got, first["a"])


# ---- 6. no cold image
def test_graph_without_a_cold_image(pg, graphs):
    G = graphs("plain12")
    assert "propagation-blocking image" not in G.fmt, G.fmt
    for count in (1, 100):
        p = G.seeds(count)
        got, iters, loop = _run(pg, G, p)
        got0, iters0, loop0 = _run(pg, G, p, tail=False)
        assert not (loop["flags"] & TAIL) and not (loop0["flags"] & TAIL)
        assert iters == iters0 and loop["spmv"] == loop0["spmv"] and np.array_equal(got, got0)
    G = Graph(12)                                            # the forced image of a graph too small for a cold entry: the general sequence
    assert "propagation-blocking image" not in G.fmt, G.fmt
    p = G.seeds(100)
    got, iters, loop = _run(pg, G, p)
    got0, iters0, loop0 = _run(pg, G, p, tail=False)
    assert loop["flags"] & PUSHED and not (loop["flags"] & TAIL)
    assert iters == iters0 and loop["spmv"] == loop0["spmv"] and np.array_equal(got, got0)
