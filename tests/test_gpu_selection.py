"""AlgorithmSelection on the MI355X: the recorded cases of tests/golden/golden_selection.json through the batch route (the mixed
batches of include/pgh_mixed.h) and through batch=False, the routes the rankers took, the widths of the mixed calls and the cut into
chunks of 64 columns."""
import numpy as np
import pytest

import selection_common as sc
from parity_common import rel_linf, tolerance_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return sc.fixture()


@pytest.fixture(scope="module")
def pg(gpu_engine):
    from pygrank_amd import _lib
    for name in _lib.MIXED_SIGNATURES:
        assert _lib.entry(name) is not None, name
    return gpu_engine


@pytest.mark.parametrize("batch", [True, False], ids=["batch", "single"])
@pytest.mark.parametrize("index", range(6))
def test_recorded_cases_on_both_routes(pg, fx, index, batch):
    case = fx["cases"][index]
    tuner, rankers = sc.check_case(pg, case, batch)
    splits = len(case["values"][0])
    routes = {name: r["route"] for name, r in zip(rankers, tuner.last_selection["rankers"])}
    calls = tuner.last_selection["mixed_calls"]
    if not batch:
        assert set(routes.values()) == {"single"} and calls == []
        return
    for name, route in routes.items():
        if name in ("NormPPR.85", "Absorb.90", "PPR.85@1e-9"):           # wrapped, absorbing, f64
            assert route == "single", name
        else:
            assert route == ("mixed_ppr" if name.startswith("PPR") else "mixed_poly"), (name, route)
    # four groups of four rankers (PageRank and HeatKernel on each of the two preprocessors), every split of a ranker a column
    assert sorted(c["kind"] for c in calls) == ["mixed_poly"] * 2 + ["mixed_ppr"] * 2
    assert [c["width"] for c in calls] == [4 * splits] * 4
    assert all(len(c["iterations"]) == c["width"] and min(c["iterations"]) >= 2 for c in calls)


def test_more_than_64_columns_are_cut_into_chunks(pg):
    """23 PageRanks on one preprocessor and three splits: 69 columns run as a call of 64 and a call of 5; the values, the choice and
    the ranks are those of batch=False."""
    graph, signal = sc.problem(pg)
    pre = pg.preprocessor("col", assume_immutability=True)
    alphas = [0.5 + 0.02 * k for k in range(23)]

    def run(batch):
        rankers = [pg.PageRank(alpha, preprocessor=pre, **sc.FAMILY) for alpha in alphas]
        tuner = pg.AlgorithmSelection(rankers, fraction_of_training=[0.9, 0.8, 0.6], batch=batch, min_batch_width=2)
        ranks = tuner.rank(graph, signal)
        return tuner.last_selection, np.asarray(ranks.np, dtype=np.float64)
    mixed, ranks_mixed = run(True)
    single, ranks_single = run(False)
    assert [c["width"] for c in mixed["mixed_calls"]] == [64, 5]
    assert {r["route"] for r in mixed["rankers"]} == {"mixed_ppr"} and {r["route"] for r in single["rankers"]} == {"single"}
    assert mixed["selected"] == single["selected"]
    for a, b in zip(mixed["rankers"], single["rankers"]):
        for got, want in zip(a["values"], b["values"]):
            assert abs(got - want) <= sc.ALLOWANCE * abs(want), (got, want)
    assert rel_linf(ranks_mixed, ranks_single) <= tolerance_for({})


def test_small_groups_run_one_by_one_and_a_failing_column_raises(pg):
    graph, signal = sc.problem(pg)
    pre = pg.preprocessor(assume_immutability=True)
    lone = [pg.PageRank(0.85, preprocessor=pre, tol=1e-6), pg.HeatKernel(3, preprocessor=pre, tol=1e-6),
            pg.HeatKernel(3, preprocessor=pre, tol=1e-6, coefficient_type="chebyshev"),
            pg.HeatKernel(5, preprocessor=pre, tol=1e-6, coefficient_type="chebyshev")]
    tuner = pg.AlgorithmSelection(lone, fraction_of_training=[0.8, 0.6])
    tuner.tune(graph, signal)
    assert [r["route"] for r in tuner.last_selection["rankers"]] == ["single"] * 4 and tuner.last_selection["mixed_calls"] == []
    # a group narrower than min_batch_width keeps the column loop; at the width it is batched
    pair = [pg.PageRank(alpha, preprocessor=pre, tol=1e-6) for alpha in (0.85, 0.9)]
    for least, route, widths in ((5, "single", []), (4, "mixed_ppr", [4])):
        tuner = pg.AlgorithmSelection(pair, fraction_of_training=[0.8, 0.6], min_batch_width=least)
        tuner.tune(graph, signal)
        assert [r["route"] for r in tuner.last_selection["rankers"]] == [route] * 2
        assert [c["width"] for c in tuner.last_selection["mixed_calls"]] == widths
    assert pg.AlgorithmSelection.MIN_BATCH_WIDTH >= 2
    # a column that does not converge raises what its own rank() raises
    short = [pg.PageRank(alpha, preprocessor=pre, tol=1e-7, error_type=pg.L1, max_iters=5, dtype="float32") for alpha in (0.85, 0.9)]
    caught = []
    for batch in (True, False):
        with pytest.raises(Exception) as info:
            pg.AlgorithmSelection(short, batch=batch, min_batch_width=2).tune(graph, signal)
        caught.append((type(info.value), str(info.value)))
    assert caught[0] == caught[1]


def test_members_with_a_personalization_transform_run_one_by_one(pg):
    """Five PageRanks and five HeatKernels on one preprocessor; the second and third of each carry a personalization transform (one by
    the constructor, one chained in).  Those four take the one-by-one route, the others are batched, and every value -- and the
    choice -- is what batch=False gives: a transform dropped on the way into the slab would change its ranker's values."""
    graph, signal = sc.problem(pg)
    pre = pg.preprocessor(assume_immutability=True)

    def family():
        ppr = [pg.PageRank(alpha, preprocessor=pre, **sc.FAMILY) for alpha in (0.5, 0.85, 0.9, 0.95, 0.99)]
        heat = [pg.HeatKernel(t, preprocessor=pre, **sc.FAMILY) for t in (1, 2, 3, 5, 7)]
        for group in (ppr, heat):
            group[1].personalization_transform = pg.HeatKernel(1, preprocessor=pre, **sc.FAMILY)
            group[2] << pg.PageRank(0.5, preprocessor=pre, **sc.FAMILY)
        return ppr + heat
    transformed = (1, 2, 6, 7)
    records = {}
    for batch in (True, False):
        rankers = family()
        tuner = pg.AlgorithmSelection(rankers, fraction_of_training=[0.8, 0.6], batch=batch, min_batch_width=2)
        assert tuner.tune(graph, signal) is rankers[tuner.last_selection["selected"]]
        records[batch] = tuner.last_selection
    routes = [r["route"] for r in records[True]["rankers"]]
    assert routes == ["single" if i in transformed else ("mixed_ppr" if i < 5 else "mixed_poly") for i in range(10)]
    assert sorted((c["kind"], c["width"]) for c in records[True]["mixed_calls"]) == [("mixed_poly", 6), ("mixed_ppr", 6)]
    assert records[True]["selected"] == records[False]["selected"]
    for i, (a, b) in enumerate(zip(records[True]["rankers"], records[False]["rankers"])):
        for got, want in zip(a["values"], b["values"]):
            assert abs(got - want) <= sc.ALLOWANCE * abs(want), (i, got, want)
    # the transform matters here: without it the ranker scores differently by far more than the allowance
    bare = pg.AlgorithmSelection([pg.PageRank(0.85, preprocessor=pre, **sc.FAMILY), pg.PageRank(0.9, preprocessor=pre, **sc.FAMILY)],
                                 fraction_of_training=[0.8, 0.6], batch=False)
    bare.tune(graph, signal)
    for i in (0, 1):
        with_transform, without = records[True]["rankers"][1 + i]["values"], bare.last_selection["rankers"][i]["values"]
        assert any(abs(x - y) > 100 * sc.ALLOWANCE * abs(y) for x, y in zip(with_transform, without)), (i, with_transform, without)
