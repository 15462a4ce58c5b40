"""Conductance and Density on the GPU: the reference's recorded values (tests/golden/golden_unsupervised.json, relative 1e-6), the
slab route against the per-column route, and evaluate_many over the 64 columns of a propagate result.

The two routes see the same f32 scores and differ in the f32 rounding of the entries of M^T s and M^T c and in the order of the f64
sums.  Each form is held to 4 * 2^-24 of the exact value (tests/test_gpu_cut_forms.py) and both measures are a ratio of two forms:
the routes agree within 8 * 2^-24, relative.  Density's denominator (sum s)^2 - sum s^2 does not cancel on the recorded vectors:
the fixture script asserts sum s^2 <= (sum s)^2 / 2 for every one of them."""
import math

import numpy as np
import pytest

import unsupervised_common as uc

pytestmark = pytest.mark.gpu

ROUTES_TOL = 8 * 2.0 ** -24
GRAPHS = ["er10k", "rmat10_dir", "weighted300"]


@pytest.fixture(scope="module")
def fx():
    return uc.fixture()


@pytest.fixture(scope="module")
def bases(gpu_engine, fx):
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = uc.Bases(gpu_engine, fx, key)
        return cache[key]
    return get


@pytest.fixture()
def per_column():
    """Sends the measures down the per-column route for the duration of the test."""
    from pygrank_amd import measures

    class Switch:
        def __enter__(self):
            measures._FORCE_PER_COLUMN = True

        def __exit__(self, *exc):
            measures._FORCE_PER_COLUMN = False
            return False
    yield Switch()
    measures._FORCE_PER_COLUMN = False


def _agree(a, b, bound=ROUTES_TOL):
    if math.isinf(a) or math.isinf(b) or a == 0 or b == 0:
        return a == b
    return abs(a - b) <= bound * max(abs(a), abs(b))


@pytest.mark.parametrize("key", GRAPHS)
def test_golden_cases_on_the_gpu(gpu_engine, fx, bases, key):
    uc.replay(bases(key))
    uc.replay(bases(key), graph_at_construction=True)


@pytest.mark.parametrize("key", GRAPHS)
def test_slab_route_agrees_with_the_per_column_route(gpu_engine, fx, bases, per_column, key):
    pg = gpu_engine
    B = bases(key)
    worst = 0.0
    for case in B.record["cases"]:
        if "raises" in case:
            continue
        scores = B.scores(case)
        measure = B.measure(case)
        slab = measure.evaluate(scores)
        assert measure.last_route == "slab", (key, case["name"])
        with per_column:
            columns = measure.evaluate(scores)
            assert measure.last_route == "columns"
        if not (math.isinf(slab) or slab == 0):
            worst = max(worst, abs(slab - columns) / abs(columns))
        print(f"{key}/{case['measure']}/{case['name']}: slab {slab!r} columns {columns!r}")
        assert _agree(slab, columns), (key, case["measure"], case["name"], slab, columns)
    print(f"{key}: largest relative difference between the routes {worst:.3e} (bound {ROUTES_TOL:.3e})")
    # the whole list at once, one slab per measure
    for name in ("Conductance", "Density"):
        plain = [c for c in B.record["cases"] if c["measure"] == name and not c["kwargs"]]
        measure = getattr(pg, name)()
        many = measure.evaluate_many([B.scores(c) for c in plain])
        assert measure.last_route == "slab"
        for case, got in zip(plain, many):
            assert uc.close(got, uc.decode(case["value"])), (key, name, case["name"], got)


def test_evaluate_many_over_a_propagate_result(gpu_engine, per_column):
    pg = gpu_engine
    import cases
    from oracle import rmat_np
    A, directed, _ = cases.GRAPHS["rmat12_sym"]()
    graph = pg.AdjacencyWrapper(A, directed=directed)
    n = A.shape[0]
    F = np.zeros((n, 64))
    for j in range(64):
        F[rmat_np.seed_nodes(A, 20, seed=100 + j), j] = 1.0
    ranks = pg.PageRank(0.85, tol=1e-6, max_iters=1000).propagate(graph, pg.to_primitive(F))
    assert isinstance(ranks, pg.DeviceMatrix) and ranks.shape == (n, 64)
    top = np.asarray(ranks, dtype=np.float64).max(axis=0)
    scaled = ranks.div_cols(top)                             # Normalize("max") of every column
    once = pg.preprocessor(normalization="none", assume_immutability=True)      # one upload for the test's ~400 evaluations
    for measure in (pg.Conductance(graph, preprocessor=once), pg.Density(graph, preprocessor=once),
                    pg.Conductance(graph, cut_ratio_only=True, preprocessor=once)):
        many = measure.evaluate_many(scaled)
        assert measure.last_route == "slab" and len(many) == 64 and all(isinstance(v, float) for v in many)
        assert all(0 < v < float("inf") for v in many)
        singles = [measure.evaluate(pg.to_signal(graph, scaled.column(j))) for j in range(64)]
        assert measure.last_route == "slab"
        with per_column:
            columns = measure.evaluate_many(scaled)
            assert measure.last_route == "columns"
        worst = max(abs(a - b) / abs(b) for a, b in zip(many, columns))
        print(f"{type(measure).__name__}: evaluate_many against per-column evaluate, largest relative difference {worst:.3e}")
        for a, b, c in zip(many, singles, columns):
            assert _agree(a, b) and _agree(a, c), (type(measure).__name__, a, b, c)
    # autofix per column: every column scaled by 1 / its maximum is the slab above
    raw = pg.Conductance(graph, autofix=True).evaluate_many(ranks)
    fixed = pg.Conductance(graph).evaluate_many(scaled)
    for j in range(64):
        if top[j] > 1:
            assert uc.close(raw[j], fixed[j], 1e-6), (j, raw[j], fixed[j])
    # the first column above max_rank raises, as a loop over evaluate would
    tall = np.ones(64)
    tall[37] = 0.25                                          # column 37 becomes 4 times its maximum-normalised self
    tall[50] = 0.5
    with pytest.raises(Exception, match="Normalize scores to be <= 1 for non-negative conductance"):
        pg.Conductance(graph).evaluate_many(scaled.div_cols(tall))
    assert pg.Conductance(graph, max_rank=4).evaluate_many(scaled.div_cols(tall))[37] > 0
    with pytest.raises(Exception, match="Normalize scores to be <= 2 for non-negative conductance"):
        pg.Conductance(graph, max_rank=2).evaluate_many(scaled.div_cols(tall))
