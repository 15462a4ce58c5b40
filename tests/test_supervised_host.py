"""The supervised measures on the host test double (no GPU) against the reference's recorded values
(tests/golden/golden_supervised.json).  The double lacks include/pgh_supervised.h and include/pgh_tune.h, so every measure takes its
columns route here: the reference's own sequence of backend primitives over f32 vectors.

Bound against the fixture (supervised_common.TOL): inputs are stored as f32 and, for the recorded cases, each measure is a ratio or a
sum of same-signed f64 sums -- 16 * 2^-24 relative.  KLDivergence / MKLDivergence, PearsonCorrelation and TNR subtract sums of like
size; the generator asserts a conditioning floor for every case of theirs it records (KL >= 1e-2; variance >= 1e-3 mean square;
denominator >= 1e-3 n) and their bound is 16 * 2^-24 divided by that floor.  Where the double happens to be closer than that, the
derived bound is kept.  No other case has a bound of its own: BinaryCrossEntropy on pagerank_max is held to 16 * 2^-24 too, on a base
built as the reference builds it (supervised_common.Bases: x / max x, the largest entry exactly 1)."""
import numpy as np
import pytest

import supervised_common as sc

GRAPHS = ["er10k", "rmat10_dir", "weighted300"]


@pytest.fixture(scope="module")
def fx():
    return sc.fixture()


def test_fixture_holds_every_case(fx):
    assert sorted(fx["graphs"]) == sorted(GRAPHS)
    assert fx["epsilon"] == float(np.finfo(np.float32).eps)
    assert sorted(fx["measures"]) == sorted(sc.NEW + sc.EXISTING)
    for record in fx["graphs"].values():
        seen = {(c["measure"], c["base"], c["excluded"]) for c in record["cases"]}
        assert seen == {(m, b, e) for m in sc.NEW + sc.EXISTING for b in sc.BASES for e in (False, True)}
        assert all(sum(k in c for k in ("value", "nonfinite", "raises")) == 1 for c in record["cases"])
        assert set(record["known"]) - set(record["exclude"]) and set(record["exclude"])


@pytest.mark.parametrize("key", GRAPHS)
def test_golden_cases_on_the_host_double(host_engine, fx, key):
    pg = host_engine
    bases = sc.Bases(pg, fx, key)
    columns = [bases.signals[base] for base in sc.BASES]
    for excluded in (False, True):
        for name in sc.NEW + sc.EXISTING:
            many = sc.check_many(bases, fx, name, excluded, "columns")
            # evaluate_many is the list of evaluate results, to the bit
            measure = bases.measure(name, excluded)
            singles = [measure.evaluate(column) for column in columns]
            assert all(sc.same(a, b) for a, b in zip(many, singles)), (name, many, singles)
    # a slab and plain vectors in place of the signals (the known scores lend their graph)
    slab = pg.DeviceMatrix.from_columns([column.np for column in columns])
    for name in ("TPR", "KLDivergence", "Mabs", "AUC"):
        for excluded in (False, True):
            want = bases.measure(name, excluded).evaluate_many(columns)
            assert all(sc.same(a, b) for a, b in zip(bases.measure(name, excluded).evaluate_many(slab), want))
            assert all(sc.same(a, b) for a, b in zip(bases.measure(name, excluded).evaluate_many([c.np for c in columns]), want))
    # known scores and exclude values per column
    excluded_signal = pg.to_signal(bases.graph, {v: 1.0 for v in bases.exclude})
    per_known = pg.DeviceMatrix.from_columns([bases.known.np for _ in columns])
    per_exclude = pg.DeviceMatrix.from_columns([excluded_signal.np for _ in columns])
    for name in ("PPV", "BinaryCrossEntropy", "L1", "MannWhitneyParity"):
        want = bases.measure(name, True).evaluate_many(columns)
        got = getattr(pg, name)(per_known, per_exclude).evaluate_many(columns)
        assert all(sc.same(a, b) for a, b in zip(got, want)), (name, got, want)
    assert pg.TPR(bases.known).evaluate_many([]) == []


def test_more_than_64_columns(host_engine, fx):
    pg = host_engine
    bases = sc.Bases(pg, fx, "weighted300")
    columns = [bases.signals["pagerank_max"] * (0.25 + 0.01 * j) for j in range(65)]
    slab = pg.DeviceMatrix.from_columns([column.np for column in columns])
    for name in ("Accuracy", "KLDivergence", "Cos", "AUC"):
        measure = bases.measure(name, True)
        many = measure.evaluate_many(slab)
        assert len(many) == 65 and measure.last_route == "columns"
        assert many == [measure.evaluate(column) for column in columns]


def test_raising_cases(host_engine, fx):
    pg = host_engine
    bases = sc.Bases(pg, fx, "weighted300")
    n = len(bases.graph)
    scores = bases.signals["pagerank_max"]
    nobody, everybody = pg.to_signal(bases.graph, np.zeros(n)), pg.to_signal(bases.graph, np.ones(n))
    for cls in (pg.AUC, pg.MannWhitneyParity):
        for single in (nobody, everybody):
            with pytest.raises(Exception, match="Cannot evaluate"):
                cls(single).evaluate(scores)
            with pytest.raises(Exception, match="Cannot evaluate"):
                cls(single).evaluate_many([scores, scores])
    # exclude needs a graph signal on either side
    plain_known, plain_scores = np.asarray(bases.known.np), np.asarray(scores.np)
    for cls in (pg.TPR, pg.Mabs, pg.AUC):
        with pytest.raises(Exception, match="Needs to parse graph signal scores or known_scores"):
            cls(plain_known, bases.exclude).evaluate_many([plain_scores])
        with pytest.raises(Exception, match="Needs to parse graph signal scores or known_scores"):
            cls(plain_known, bases.exclude).evaluate(plain_scores)
        assert cls(plain_known).evaluate_many([plain_scores]) == [cls(bases.known).evaluate(scores)]
    # columns of two graphs
    other = sc.Bases(pg, fx, "weighted300")
    for cls in (pg.pRule, pg.Cos):
        with pytest.raises(Exception, match="belong to different graphs"):
            cls(bases.known).evaluate_many([scores, other.signals["seeds"]])
    # a slab whose rows do not match the known scores
    short = pg.DeviceMatrix.from_host(np.ones((n - 1, 3)))
    for cls in (pg.Accuracy, pg.Dot, pg.AUC):
        with pytest.raises(Exception, match="cannot be built from 299 values"):
            cls(bases.known).evaluate_many(short)
        with pytest.raises(Exception, match="a slab of 299 rows cannot be scored against known scores of 300 nodes"):
            cls(plain_known).evaluate_many(short)
    # known scores per column must come one per score column
    with pytest.raises(Exception, match="holds 2 columns for 3 score columns"):
        pg.TPR(pg.DeviceMatrix.from_columns([bases.known.np] * 2)).evaluate_many([scores] * 3)


def test_best_direction_of_every_class(host_engine, fx):
    pg = host_engine
    for name in sc.NEW + sc.EXISTING:
        assert getattr(pg, name)([1, 0]).best_direction() == fx["best_direction"][name], name
        assert issubclass(getattr(pg, name), pg.Supervised)
    assert pg.L2Disparity([1, 0], target_pRule=0.5).target_pRule == 0.5 and pg.L2Disparity([1, 0]).target_pRule == 0.8
