"""Conductance and Density on the host test double (no GPU) against the reference's recorded values
(tests/golden/golden_unsupervised.json).  The double lacks include/pgh_measure.h, so both measures take their per-column route here:
the reference's own sequence of backend primitives."""
import numpy as np
import pytest

import unsupervised_common as uc

GRAPHS = ["er10k", "rmat10_dir", "weighted300"]


@pytest.fixture(scope="module")
def fx():
    return uc.fixture()


def test_fixture_holds_every_case(fx):
    assert sorted(fx["graphs"]) == sorted(GRAPHS)
    for record in fx["graphs"].values():
        names = {(c["measure"], c["name"]) for c in record["cases"]}
        for name in ("seeds", "pagerank_max", "pagerank_autofix", "pagerank_strict", "cut_ratio_only", "max_rank_2", "zeros", "full"):
            assert ("Conductance", name) in names
        for name in ("seeds", "pagerank_max", "zeros", "full"):
            assert ("Density", name) in names
        assert any("raises" in c for c in record["cases"])
        for c in record["cases"]:
            if c["name"] in ("zeros", "full") and c["measure"] == "Conductance":
                assert c["value"] == "inf"
            if c["name"] == "zeros" and c["measure"] == "Density":
                assert c["value"] == 0


@pytest.mark.parametrize("key", GRAPHS)
def test_golden_cases_on_the_host_double(host_engine, fx, key):
    pg = host_engine
    bases = uc.Bases(pg, fx, key)
    from_signal = uc.replay(bases)
    at_construction = uc.replay(bases, graph_at_construction=True)
    assert from_signal == at_construction               # the same graph either way: the same arithmetic
    # evaluate_many is the list of evaluate results (the raising cases apart: they get a test of their own)
    for measure_name in ("Conductance", "Density"):
        plain = [c for c in bases.record["cases"] if c["measure"] == measure_name and not c["kwargs"] and "raises" not in c]
        measure = getattr(pg, measure_name)()
        columns = [bases.scores(c) for c in plain]
        many = measure.evaluate_many(columns)
        assert measure.last_route == "columns"
        assert isinstance(many, list) and many == [measure.evaluate(s) for s in columns]
        assert getattr(pg, measure_name)(bases.graph).evaluate_many([s.np for s in columns]) == many
        slab = pg.DeviceMatrix.from_columns([s.np for s in columns])
        assert getattr(pg, measure_name)(bases.graph).evaluate_many(slab) == many
    assert pg.Conductance().evaluate_many([]) == []


def test_evaluate_many_raises_on_the_first_column_above_max_rank(host_engine, fx):
    pg = host_engine
    bases = uc.Bases(pg, fx, "weighted300")
    fine, above = bases.signals["pagerank_max"], bases.signals["pagerank_max"] * 3
    with pytest.raises(Exception, match="Normalize scores to be <= 1 for non-negative conductance"):
        pg.Conductance().evaluate_many([fine, above, fine])
    fixed = pg.Conductance(autofix=True).evaluate_many([fine, above])
    assert uc.close(fixed[1], fixed[0], 1e-6)
    with pytest.raises(Exception):
        pg.Conductance().evaluate_many(pg.DeviceMatrix.from_columns([fine.np]))      # a slab needs the measure's graph
    with pytest.raises(Exception):
        pg.Conductance().evaluate_many([fine, uc.Bases(pg, fx, "weighted300").signals["seeds"]])     # two graphs


def test_best_direction_and_empty_graphs(host_engine, fx):
    pg = host_engine
    assert pg.Conductance().best_direction() == fx["best_direction"]["Conductance"] == -1
    assert pg.Density().best_direction() == fx["best_direction"]["Density"] == 1
    import scipy.sparse as sp
    empty = pg.AdjacencyWrapper(sp.csr_array((0, 0)), directed=True)
    assert pg.Conductance(empty).evaluate([]) == float("inf")
    assert pg.Density(empty).evaluate([]) == 0
    assert issubclass(pg.Conductance, pg.Unsupervised) and issubclass(pg.Density, pg.Unsupervised)


def test_normalization_reaches_the_preprocessor(host_engine, fx):
    pg = host_engine
    bases = uc.Bases(pg, fx, "weighted300")
    scores = bases.signals["pagerank_max"]
    seen = []

    def spy(graph):
        seen.append(graph)
        return pg.preprocessor(normalization="col")(graph)
    by_name = pg.Conductance(normalization="col").evaluate(scores)
    by_hand = pg.Conductance(preprocessor=spy).evaluate(scores)
    assert seen == [bases.graph] and by_name == by_hand
    # the value is the reference's formula on the column-normalised matrix, and it is not the unnormalised one
    import cases
    A, _, _ = cases.GRAPHS["weighted300"]()
    deg = np.asarray(A.sum(axis=1)).ravel()
    M = A.multiply(np.where(deg != 0, 1.0 / np.where(deg != 0, deg, 1), 0.0)[:, None]).tocsr()
    s = np.asarray(scores.np, dtype=np.float64)
    c = 1 - s
    N, Cc = M.T @ s, M.T @ c
    want = float(N @ c) / min(float(N @ s), float(Cc @ c))
    assert uc.close(by_name, want)
    assert not uc.close(by_name, pg.Conductance().evaluate(scores), 1e-3)
