"""NDCG, SpearmanCorrelation and the measure combinations on the GPU: the reference's recorded values
(tests/golden/golden_ranking.json) through the real library on the slab route (include/pgh_rank.h) and, under
measures._FORCE_PER_COLUMN, on the columns route.

Bounds (rank_common): against the fixture NDCG is held to 16 * 2^-24 relative and Spearman's rho to n' * 2^-50 absolute on either route,
the combinations to 64 * 2^-24 absolute; the two PageRank bases get, on top, the order slack derived from this run's own near-ties.
The two routes read the same f32 vectors, so against each other no slack applies: NDCG within 16 * 2^-24 relative (the columns route
forms its terms in f32, the slab route in f64), rho within n' * 2^-50 (both routes sum exact integers' products in f64)."""
import math

import numpy as np
import pytest

import rank_common as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return rc.fixture()


@pytest.fixture(scope="module")
def rankings(gpu_engine, fx):
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = rc.Ranking(gpu_engine, fx, key)
        return cache[key]
    return get


@pytest.fixture()
def per_column():
    from pygrank_amd import measures

    def force(value):
        measures._FORCE_PER_COLUMN = value
    yield force
    measures._FORCE_PER_COLUMN = False


@pytest.mark.parametrize("key", rc.GRAPHS)
def test_golden_cases_on_both_routes(gpu_engine, fx, rankings, per_column, key):
    from pygrank_amd import _lib as L
    assert all(L.entry(name) is not None for name in L.RANK_SIGNATURES)
    ranking = rankings(key)
    for excluded in (False, True):
        per_column(False)
        slab = rc.check_fixture_measures(ranking, fx, "slab", excluded)
        per_column(True)
        cols = rc.check_fixture_measures(ranking, fx, "columns", excluded)
        per_column(False)
        kept = ranking.kept if excluded else ranking.n
        for case, values in slab.items():
            for a, b in zip(values, cols[case]):
                if math.isfinite(a) and math.isfinite(b):
                    bound = rc.NDCG_TOL * max(abs(a), abs(b)) if case[0] == "NDCG" else rc.spearman_tol(kept)
                    assert abs(a - b) <= bound, (key, case, a, b)
                else:
                    assert rc.same(a, b), (key, case, a, b)


@pytest.mark.parametrize("key", rc.GRAPHS)
def test_evaluate_is_the_one_column_case(gpu_engine, fx, rankings, key):
    pg = gpu_engine
    ranking = rankings(key)
    columns = ranking.columns()
    slab = pg.DeviceMatrix.from_columns([column.np for column in columns])
    for excluded in (None, ranking.exclude):
        for measure in (pg.NDCG(ranking.knowns["graded"], excluded, k=10), pg.NDCG(ranking.knowns["binary"], excluded),
                        pg.SpearmanCorrelation(ranking.knowns["graded"], excluded)):
            many = measure.evaluate_many(columns)
            assert measure.last_route == "slab"
            plan = measure._plan_cache[4]
            singles = [measure.evaluate(column) for column in columns]
            assert measure._plan_cache[4] is plan                              # one plan serves every call
            assert all(rc.same(a, b) for a, b in zip(many, singles)), (type(measure).__name__, many, singles)
            assert all(rc.same(a, b) for a, b in zip(measure.evaluate_many(slab), many))
            assert all(rc.same(a, b) for a, b in zip(measure.evaluate_many([c.np for c in columns]), many))
            measure.exclude = None if excluded is not None else ranking.exclude
            measure.evaluate(columns[0])
            assert measure._plan_cache[4] is not plan                          # another exclude object: another plan


@pytest.mark.parametrize("pair", ["auc_prule", "ndcg_cos"])
@pytest.mark.parametrize("key", rc.GRAPHS)
def test_combinations(gpu_engine, fx, rankings, key, pair):
    """Every recorded combination against the fixture, and evaluate_many against evaluate TO THE BIT.

    A combination folds its members' values with the same scalar code on both entry points, so it is bit-equal when every member's
    value is.  AUC, NDCG and SpearmanCorrelation score all columns in one pass and are bit-equal to their evaluate (tested above and
    in test_gpu_supervised.py).  Cos and pRule are not on the engine -- Cos.evaluate is three pgh_dot reductions, Cos.evaluate_many one
    pgh_pair_forms pass, whose order of summation depends on the slab's width -- so the default evaluate_many scores such members
    column by column; one pass over all columns for them differed by one ulp on the PageRank bases (er10k, Disparity / weights:
    0.2772133636666198 against 0.27721336366661986).  evaluate_many(exact=False) takes that pass for every member and is held to the
    fixture's bound, not to the bit."""
    ranking = rankings(key)
    for excluded in (False, True):
        rc.check_fixture_combinations(ranking, fx, excluded, pairs=[pair])
    exact = rc.combination(gpu_engine, "AM", pair, "weights", ranking.knowns["binary"], None)
    exact.evaluate_many(ranking.columns())
    assert exact.last_batched == [0]                          # AUC resp. NDCG in one pass, pRule resp. Cos column by column


def test_more_than_64_columns_and_per_column_known_scores(gpu_engine, fx, rankings):
    pg = gpu_engine
    ranking = rankings("weighted300")
    columns = [ranking.signals["pagerank_max"] * (0.25 + 0.01 * j) + ranking.signals["seeds"] * (0.001 * (j % 7)) for j in range(65)]
    slab = pg.DeviceMatrix.from_columns([column.np for column in columns])
    for measure in (pg.NDCG(ranking.knowns["graded"], ranking.exclude, k=10), pg.SpearmanCorrelation(ranking.knowns["binary"], ranking.exclude)):
        many = measure.evaluate_many(slab)
        assert len(many) == 65 and measure.last_route == "slab"
        assert many == [measure.evaluate(column) for column in columns]
    few = columns[:3]
    per_known = pg.DeviceMatrix.from_columns([ranking.knowns["graded"].np for _ in few])
    for cls, extra in ((pg.NDCG, dict(k=10)), (pg.SpearmanCorrelation, {})):
        measure = cls(per_known, **extra)
        got = measure.evaluate_many(few)
        assert measure.last_route == "columns"
        want = cls(ranking.knowns["graded"], **extra).evaluate_many(few)
        bound = rc.NDCG_TOL if cls is pg.NDCG else rc.spearman_tol(ranking.n)
        assert all(abs(a - b) <= bound * max(abs(b), 1) for a, b in zip(got, want)), (cls.__name__, got, want)


def test_selection_and_tuning_under_ndcg(gpu_engine, fx, rankings):
    """pg.NDCG as the measure of AlgorithmSelection and ParameterTuner, through their generic routes; no tuned quality is asserted."""
    pg = gpu_engine
    ranking = rankings("weighted300")
    seeds = ranking.signals["seeds"]
    selected = pg.AlgorithmSelection(measure=pg.NDCG)(ranking.graph, seeds)
    assert isinstance(selected, pg.GraphSignal) and np.isfinite(np.asarray(selected.np, dtype=np.float64)).all()
    tuner = pg.ParameterTuner(lambda params: pg.PageRank(alpha=params[0]), measure=pg.NDCG, deviation_tol=0.05, max_vals=[0.99],
                              min_vals=[0.5], verbose=False)
    tuned = tuner(ranking.graph, seeds)
    assert isinstance(tuned, pg.GraphSignal) and 0.5 <= tuner.last_params[0] <= 0.99
