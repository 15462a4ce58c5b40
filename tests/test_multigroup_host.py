"""LinkAssessment, ClusteringCoefficient, Modularity, MultiSupervised and MultiUnsupervised on the host test double (no GPU) against the
reference's recorded values (tests/golden/golden_multigroup.json).  The double has no include/pgh_link.h entry, so LinkAssessment and
ClusteringCoefficient score the downloaded slab with numpy, and it has neither pgh_cut_forms nor pgh_pair_forms, so Modularity takes its
backend-primitive route.

Bounds.
  LinkAssessment         num_pairs * 2^-52 absolute: the pair counts are identical to the reference's (asserted: pairs, positives, first
                         draws); only sklearn's sequential trapezoid sum rounds, once per threshold at most.
  Modularity             PARITY = 1e-6 (the project's bound for f32 storage) times (w^T P w + (sum w d)^2 / 2m) / 2m: the value is a
                         difference, the bound is relative to its two terms.
  ClusteringCoefficient  PARITY relative.
  Multi*                 PARITY relative; exact=False against the loop within the same bound (the members' own).
"""
import warnings

import numpy as np
import pytest

import link_common as lc

GRAPHS = ["weighted300", "rmat10_dir", "rmat12_sym", "er10k"]


@pytest.fixture(scope="module")
def fx():
    return lc.fixture()


def test_fixture_holds_every_case(fx):
    assert sorted(fx["graphs"]) == sorted(GRAPHS)
    for key, record in fx["graphs"].items():
        link = {(c["hops"], c["similarity"], c["seed"]) for c in record["link"]}
        assert {(h, s, r) for h in (1, 2) for s in ("cos", "dot") for r in (0, 7)} <= link, key
        assert {c["similarity"] for c in record["clustering"]} == {"cos", "dot"}
        assert {c["max_rank"] for c in record["modularity"]} == {1, 2} and len(record["modularity"]) == 4
        assert {(c["measure"], c.get("excluded")) for c in record["multi"]} == \
            {(m, e) for m in lc.SUPERVISED for e in (False, True)} | {(m, None) for m in lc.UNSUPERVISED}
    assert any(c["max_positive"] == 2000 and c["max_negative"] == 2000 for c in fx["graphs"]["er10k"]["link"])
    # both branches of the sample are recorded
    assert all(c["max_positive"] > 300 for c in fx["graphs"]["weighted300"]["link"])
    assert all(c["max_positive"] < 10000 for c in fx["graphs"]["er10k"]["link"])


@pytest.mark.parametrize("key", GRAPHS)
def test_golden_cases_on_the_host_double(host_engine, fx, key):
    inputs = lc.Inputs(host_engine, fx, key)
    state = np.random.get_state()
    lc.replay_link(inputs, "host")
    lc.replay_clustering(inputs, "host")
    for measure, _ in lc.replay_modularity(inputs):
        assert measure.last_route == "columns"
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]     # numpy's global generator is untouched
    lc.replay_multi(inputs)


def test_inputs_in_every_accepted_form_agree(host_engine, fx):
    """A dict of signals, a dict of {node: score} with missing nodes, a list of vectors and a DeviceMatrix are one slab; a networkx
    graph and a bare scipy matrix are the AdjacencyWrapper's graph."""
    import networkx as nx
    pg = host_engine
    inputs = lc.Inputs(pg, fx, "weighted300")
    S = inputs.S
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = pg.LinkAssessment(inputs.graph).evaluate(inputs.signals)
        sparse = {f"g{j}": {v: float(S[v, j]) for v in range(inputs.n) if S[v, j] != 0} for j in range(lc.GROUPS)}
        assert pg.LinkAssessment(inputs.graph).evaluate(sparse) == want
        assert pg.LinkAssessment(inputs.graph).evaluate([S[:, j].copy() for j in range(lc.GROUPS)]) == want
        assert pg.LinkAssessment(inputs.graph)(inputs.slab()) == want
        G = nx.from_scipy_sparse_array(inputs.A, create_using=nx.DiGraph)
        assert pg.LinkAssessment(G, nodes=[0, 1]).evaluate(sparse) == want
        assert pg.LinkAssessment(inputs.A).evaluate(inputs.slab()) == want
        assert pg.ClusteringCoefficient(G).evaluate(sparse) == pg.ClusteringCoefficient(inputs.graph).evaluate(inputs.slab())
        assert pg.Modularity(G).evaluate(sparse["g0"]) == pg.Modularity(inputs.graph).evaluate(inputs.signals["g0"])
    with pytest.raises(Exception, match="expected cos or dot"):
        pg.LinkAssessment(inputs.graph, similarity="jaccard")


def test_one_plan_serves_every_evaluation_and_other_measures_get_the_predictions(host_engine, fx):
    pg = host_engine
    inputs = lc.Inputs(pg, fx, "weighted300")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        seen = []

        def progress(candidates):
            seen.append(len(candidates))
            return candidates
        measure = pg.LinkAssessment(inputs.graph, hops=2, progress=progress)
        first = measure.evaluate(inputs.signals)
        assert measure.evaluate(inputs.signals) == first and measure.plans_built == 1 and seen == [inputs.n]
        mine = lc.pairs(inputs.A, 2, 2000, 2000, 0)
        plan = measure.plan()
        assert np.array_equal(plan.first, mine["first"]) and np.array_equal(plan.second, mine["second"])
        assert np.array_equal(plan.label, mine["label"])
        predicted, real = measure.predictions(inputs.signals)
        assert np.array_equal(predicted, lc.predictions(inputs.S, mine["first"], mine["second"], "cos"))
        assert first == lc.auc(predicted, real)
        # measure(real)(predicted), as the reference: Cos of the labels and the similarities
        other = pg.LinkAssessment(inputs.graph, hops=2, measure=pg.Cos).evaluate(inputs.signals)
        real = real.astype(np.float64)
        want = float(np.dot(real, predicted) / np.sqrt(np.dot(real, real) * np.dot(predicted, predicted)))
        assert lc.close(other, want)


def test_edges(host_engine, fx):
    import scipy.sparse as sp
    pg = host_engine
    edges = fx["edges"]
    empty = pg.AdjacencyWrapper(sp.csr_array((5, 5)), directed=False)
    S = lc.group_scores(5, seed=9)
    groups = {f"g{j}": pg.to_signal(empty, S[:, j].copy()) for j in range(lc.GROUPS)}
    with pytest.raises(Exception) as raised:
        pg.LinkAssessment(empty).evaluate(groups)
    assert str(raised.value) == edges["link_no_edges_raises"] == "Cannot evaluate AUC when all labels are the same"
    assert pg.Modularity(empty).evaluate(groups["g0"]) == edges["modularity_no_edges"] == 0
    assert pg.ClusteringCoefficient(empty).evaluate(groups) == edges["clustering_no_edges"] == 0
    import cases
    A, directed, _ = cases.GRAPHS["weighted300"]()
    graph = pg.AdjacencyWrapper(A, directed=directed)
    S1 = lc.group_scores(A.shape[0], groups=1, seed=5)
    for case in edges["single_group"]:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = pg.LinkAssessment(graph, similarity=case["similarity"]).evaluate({"only": S1[:, 0].copy()})
        assert abs(got - case["value"]) <= lc.link_bound(case)
    # non-finite scores: what sklearn says to the reference
    bad = lc.group_scores(A.shape[0], seed=0)
    bad[7, -1] = np.inf                                     # inf / inf under "cos", whatever the partner holds
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="Input contains NaN"):
            pg.LinkAssessment(graph).evaluate([bad[:, j].copy() for j in range(lc.GROUPS)])


def test_modularity_many_columns_and_directions(host_engine, fx):
    pg = host_engine
    inputs = lc.Inputs(pg, fx, "rmat10_dir")
    measure = pg.Modularity(inputs.graph, max_positive_samples=100)
    columns = list(inputs.signals.values())
    many = measure.evaluate_many(columns)
    assert many == [measure.evaluate(c) for c in columns]
    assert pg.Modularity(inputs.graph, max_positive_samples=100).evaluate_many(inputs.slab()) == many
    assert measure.evaluate_many([]) == []
    for j, value in enumerate(many):
        want = lc.modularity(inputs.A, inputs.directed, inputs.S[:, j], 1, 100, 0)
        internal, expected, m = lc.modularity_terms(inputs.A, inputs.directed, inputs.S[:, j], 1, 100, 0)
        assert abs(value - want) <= lc.PARITY * (internal + expected) / 2 / m
    assert issubclass(pg.Modularity, pg.Unsupervised) and pg.Modularity().best_direction() == 1
