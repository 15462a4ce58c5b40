"""NDCG, SpearmanCorrelation and the measure combinations on the host test double (no GPU) against the reference's recorded values
(tests/golden/golden_ranking.json).  The double lacks include/pgh_rank.h, so both measures take their columns route: NDCG is
filter_out, DeviceVector.ordinals() and one masked sum of f32 terms, SpearmanCorrelation ranks the two downloaded vectors with numpy.

Bounds (rank_common): NDCG -- a ratio of two sums of at most k non-negative terms, each known / log2(.) formed from exact f32 ordinals
and an f32 logarithm: below 5 f32 ulps per term, hence per sum, twice that for the ratio, held at 16 * 2^-24 relative.  Spearman on this
route is f64 throughout: n' * 2^-50 absolute.  Combinations: 64 * 2^-24 absolute.  The two PageRank bases are rebuilt by an f32 run and
get, on top, the order slack rank_common.Ranking derives from this run's own near-ties (0 for the three tie-laden bases)."""
import numpy as np
import pytest

import rank_common as rc
import supervised_common as sc


@pytest.fixture(scope="module")
def fx():
    return rc.fixture()


def test_fixture_holds_every_case(fx):
    assert sorted(fx["graphs"]) == sorted(rc.GRAPHS) and fx["bases"] == sc.BASES
    for record in fx["graphs"].values():
        ndcg = {(c["base"], c["known"], c["k"], c["excluded"]) for c in record["cases"] if c["measure"] == "NDCG"}
        assert ndcg == {(b, kn, k, e) for b in sc.BASES for kn in fx["knowns"] for k in rc.KS for e in (False, True)}
        rho = {(c["base"], c["known"], c["excluded"]) for c in record["cases"] if c["measure"] == "SpearmanCorrelation"}
        assert rho == {(b, kn, e) for b in sc.BASES for kn in fx["knowns"] for e in (False, True)}
        combos = {(c["measure"], c["pair"], c["mode"], c["base"], c["excluded"]) for c in record["cases"] if "pair" in c}
        assert combos == {(m, p, mode, b, e) for m in fx["combinations"] for p in fx["pairs"] for mode in rc.modes_of(fx, m, p)
                          for b in sc.BASES for e in (False, True)}
        assert all(sum(k in c for k in ("value", "nonfinite", "raises")) == 1 for c in record["cases"])
        assert sorted(sum(record["graded"].values(), [])) == record["known"]
    assert any("nonfinite" in c for r in fx["graphs"].values() for c in r["cases"])


@pytest.mark.parametrize("key", rc.GRAPHS)
def test_golden_cases_on_the_host_double(host_engine, fx, key):
    pg = host_engine
    ranking = rc.Ranking(pg, fx, key)
    columns = ranking.columns()
    for excluded in (False, True):
        many = rc.check_fixture_measures(ranking, fx, "columns", excluded)
        exclude = ranking.exclude if excluded else None
        # evaluate_many is the list of evaluate results, to the bit
        for (name, known_name, label), values in many.items():
            known = ranking.knowns[known_name]
            measure = pg.NDCG(known, exclude, k=ranking.k_of(label, known_name)) if name == "NDCG" else pg.SpearmanCorrelation(known, exclude)
            singles = [measure.evaluate(column) for column in columns]
            assert all(rc.same(a, b) for a, b in zip(values, singles)), (name, known_name, label, values, singles)
        rc.check_fixture_combinations(ranking, fx, excluded)
    # a slab and plain vectors in place of the signals (the known scores lend their graph)
    slab = pg.DeviceMatrix.from_columns([column.np for column in columns])
    for measure in (pg.NDCG(ranking.knowns["graded"], ranking.exclude, k=10), pg.SpearmanCorrelation(ranking.knowns["graded"], ranking.exclude),
                    rc.combination(pg, "AM", "ndcg_cos", "zero", ranking.knowns["binary"], ranking.exclude)):
        want = measure.evaluate_many(columns)
        assert all(rc.same(a, b) for a, b in zip(measure.evaluate_many(slab), want))
        assert all(rc.same(a, b) for a, b in zip(measure.evaluate_many([c.np for c in columns]), want))
        assert measure.evaluate_many([]) == []
    # known scores and exclude values per column
    excluded_signal = pg.to_signal(ranking.graph, {v: 1.0 for v in ranking.exclude})
    per_known = pg.DeviceMatrix.from_columns([ranking.knowns["graded"].np for _ in columns])
    per_exclude = pg.DeviceMatrix.from_columns([excluded_signal.np for _ in columns])
    for cls, extra in ((pg.NDCG, dict(k=10)), (pg.SpearmanCorrelation, {})):
        want = cls(ranking.knowns["graded"], ranking.exclude, **extra).evaluate_many(columns)
        measure = cls(per_known, per_exclude, **extra)
        got = measure.evaluate_many(columns)
        assert measure.last_route == "columns" and all(rc.same(a, b) for a, b in zip(got, want)), (cls.__name__, got, want)


def test_more_than_64_columns(host_engine, fx):
    pg = host_engine
    ranking = rc.Ranking(pg, fx, "weighted300")
    columns = [ranking.signals["pagerank_max"] * (0.25 + 0.01 * j) + ranking.signals["seeds"] * (0.001 * (j % 7)) for j in range(65)]
    slab = pg.DeviceMatrix.from_columns([column.np for column in columns])
    for measure in (pg.NDCG(ranking.knowns["graded"], ranking.exclude, k=10), pg.SpearmanCorrelation(ranking.knowns["binary"], ranking.exclude)):
        many = measure.evaluate_many(slab)
        assert len(many) == 65 and measure.last_route == "columns"
        assert many == [measure.evaluate(column) for column in columns]
    combo = rc.combination(pg, "GM", "auc_prule", "weights", ranking.knowns["binary"], ranking.exclude)
    assert combo.evaluate_many(slab) == [combo.evaluate(column) for column in columns]


def test_edges_do_what_the_reference_does(host_engine, fx):
    pg = host_engine
    ranking = rc.Ranking(pg, fx, "weighted300")
    n, graph, edges = ranking.n, ranking.graph, fx["edges"]
    ones, nothing = pg.to_signal(graph, np.ones(n)), pg.to_signal(graph, np.zeros(n))
    some = pg.to_signal(graph, {0: 1.0, 5: 0.5})
    assert edges["ndcg_idcg_zero"] == {"nonfinite": "nan"} and np.isnan(pg.NDCG(nothing).evaluate(ones))
    assert edges["ndcg_relevant_all_excluded"] == {"nonfinite": "nan"} and np.isnan(pg.NDCG(some, [0, 5]).evaluate(ones))
    assert np.isnan(pg.NDCG(some, [0, 5]).evaluate_many([ones, ones])).all()
    assert edges["ndcg_nothing_kept"]["raises"].startswith("ZeroDivisionError")
    everybody = {v: 1.0 for v in range(n)}
    with pytest.raises(ZeroDivisionError):
        pg.NDCG(some, everybody).evaluate(ones)
    with pytest.raises(ZeroDivisionError):
        pg.NDCG(some, everybody).evaluate_many([ones])
    assert "cannot be computed for k greater" in edges["ndcg_k_too_large"]["raises"]
    with pytest.raises(Exception, match="NDCG@k cannot be computed for k greater than the number of known scores"):
        pg.NDCG(some, k=n + 1)
    assert pg.NDCG(some).k == n and pg.NDCG(some, k=n).k == n and pg.NDCG([1, 0, 0]).k == 3
    # k is not reduced by the exclusion: with n' < k the slice is simply shorter
    exclude = ranking.exclude
    assert pg.NDCG(some, exclude, k=n).evaluate(ones) == pg.NDCG(some, exclude, k=n - len(exclude)).evaluate(ones)
    assert edges["spearman_constant_known"] == {"nonfinite": "nan"} and np.isnan(pg.SpearmanCorrelation(nothing).evaluate(some))
    assert np.isnan(pg.SpearmanCorrelation(some).evaluate(ones))
    assert pg.SpearmanCorrelation([1, 2, 3]).evaluate([1, 2, 3]) == 1 and pg.SpearmanCorrelation([1, 2, 3]).evaluate([3, 2, 1]) == -1
    assert pg.NDCG([1, 0]).best_direction() == 1 and pg.SpearmanCorrelation([1, 0]).best_direction() == 1
    # exclude needs a graph signal on either side
    for cls in (pg.NDCG, pg.SpearmanCorrelation):
        with pytest.raises(Exception, match="Needs to parse graph signal scores or known_scores"):
            cls(np.asarray(some.np), exclude).evaluate(np.asarray(ones.np))


def test_combination_rules(host_engine):
    pg = host_engine
    inf = float("inf")

    class Fixed(pg.measures.Measure):
        def __init__(self, value):
            self.value, self.calls = value, 0

        def evaluate(self, scores):
            self.calls += 1
            return self.value

    # the two threshold defaults
    assert pg.AM([Fixed(2.0)]).thresholds == [(0., 1.)] and pg.AM().add(Fixed(2.0)).thresholds == [(-inf, inf)]
    assert pg.AM([Fixed(2.0), Fixed(-1.0)]).evaluate(None) == 0.5 and pg.AM().add(Fixed(2.0)).add(Fixed(-1.0)).evaluate(None) == 0.5
    assert pg.AM().add(Fixed(2.0)).add(Fixed(-1.0), weight=3.).evaluate(None) == (2.0 - 3.0) / 4
    # members of weight 0 are not evaluated; the sign of Disparity and Parity alternates with the position all the same
    skipped = Fixed(0.3)
    combo = pg.Disparity([Fixed(0.9), skipped, Fixed(0.5), Fixed(0.2)], weights=[1., 0., 1., 2.])
    assert combo.evaluate(None) == abs(0.9 + 0.5 - 2 * 0.2) and skipped.calls == 0
    assert pg.Parity([Fixed(0.9), skipped, Fixed(0.5), Fixed(0.2)], weights=[1., 0., 1., 2.]).evaluate(None) == 1 - abs(0.9 + 0.5 - 2 * 0.2)
    assert pg.Disparity([Fixed(0.2), Fixed(0.9)]).evaluate(None) == 0.9 - 0.2
    # GM takes no value below epsilon
    eps = pg.epsilon()
    assert pg.GM([Fixed(0.0), Fixed(1.0)]).evaluate(None) == float(np.exp((np.log(eps) + np.log(1.0)) / 2))
    assert abs(pg.GM([Fixed(0.25), Fixed(1.0)]).evaluate(None) - 0.5) < 1e-15
    # the differentiable hinge: only against finite thresholds
    hinge = pg.AM([Fixed(0.5)], thresholds=[(0, inf)], differentiable=True)
    x = 0.5
    assert hinge.evaluate(None) == x + float(np.log(1 + np.exp(-x * 30))) / 30
    assert pg.AM().add(Fixed(0.5)).evaluate(None) == 0.5 and pg.AM([Fixed(0.5)], differentiable=True).differentiable
    # members without evaluate_many are evaluated column by column
    assert pg.AM([Fixed(0.5), Fixed(1.5)]).evaluate_many([[1, 0], [0, 1], [1, 1]]) == [0.75] * 3
    assert pg.AM([Fixed(0.5)]).evaluate_many([]) == []
    assert issubclass(pg.AM, pg.MeasureCombination) and issubclass(pg.MeasureCombination, pg.measures.Measure)

    # which members are scored in one pass: by default those that declare that pass bit-equal to evaluate, with exact=False all
    class Many(Fixed):
        passes = 0

        def evaluate_many(self, columns):
            self.passes += 1
            return [self.value for _ in columns]

    class ExactMany(Many):
        _MANY_IS_EXACT = True

    loose, tight, skipped = Many(0.5), ExactMany(1.0), ExactMany(0.3)
    combo = pg.AM([loose, tight, skipped], weights=[1., 1., 0.])
    columns = [[1, 0], [0, 1], [1, 1]]
    assert combo.evaluate_many(columns) == [0.75] * 3 and combo.last_batched == [1]
    assert (loose.passes, loose.calls, tight.passes, tight.calls, skipped.passes, skipped.calls) == (0, 3, 1, 0, 0, 0)
    assert combo.evaluate_many(columns, exact=False) == [0.75] * 3 and combo.last_batched == [0, 1]
    assert (loose.passes, loose.calls, tight.passes, tight.calls, skipped.passes, skipped.calls) == (1, 3, 2, 0, 0, 0)
    nested = pg.GM([combo, tight])
    assert nested.evaluate_many(columns, exact=False) == [nested.evaluate(c) for c in columns] and nested.last_batched == [0, 1]
    assert loose.passes == 2                                  # exact=False reaches the inner combination
    for name in ("AUC", "MannWhitneyParity", "NDCG", "SpearmanCorrelation", "AM", "GM", "Disparity", "Parity"):
        assert getattr(pg, name)._MANY_IS_EXACT is True, name
    for name in ("Cos", "pRule", "Dot", "Accuracy", "KLDivergence"):
        assert not getattr(getattr(pg, name), "_MANY_IS_EXACT", False), name
