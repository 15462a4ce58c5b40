"""AlgorithmSelection and the filter factories on the host test double (no GPU) against the reference's recorded behaviour
(tests/golden/golden_selection.json).  The double lacks include/pgh_mixed.h, so every ranker takes the one-by-one route here."""
import pytest

import selection_common as sc


@pytest.fixture(scope="module")
def fx():
    return sc.fixture()


def _describe(rankers):
    out = []
    for name, ranker in rankers.items():
        params = {key: float(getattr(ranker, key)) for key in ("alpha", "t") if hasattr(ranker, key)}
        params.update(tol=float(ranker.convergence.tol), max_iters=int(ranker.convergence.max_iters))
        out.append([name, type(ranker).__name__, params])
    return out


@pytest.mark.parametrize("index", range(6))
def test_selection_reproduces_the_reference(host_engine, fx, index):
    pg = host_engine
    assert fx["allowance"] == sc.ALLOWANCE and fx["planted"] == sc.PLANTED and len(fx["cases"]) == 6
    tuner, _ = sc.check_case(pg, fx["cases"][index], True)       # (batch=True: the double has no mixed entry, every ranker runs alone)
    assert {r["route"] for r in tuner.last_selection["rankers"]} == {"single"}
    assert tuner.last_selection["mixed_calls"] == []


class _Recorder:
    """A ranker that notes how it was called and answers with the ranks of the ranker inside."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def rank(self, graph=None, personalization=None, *args, **kwargs):
        self.calls.append(dict(kwargs))
        return self.inner.rank(graph, personalization)


def test_first_of_equal_rankers_wins(host_engine):
    pg = host_engine
    graph, signal = sc.problem(pg)
    pre = pg.preprocessor(assume_immutability=True)
    weak = pg.PageRank(0.5, preprocessor=pre, tol=1e-6)
    twins = [pg.HeatKernel(3, preprocessor=pre, tol=1e-6), pg.HeatKernel(3, preprocessor=pre, tol=1e-6)]
    for batch in (True, False):
        tuner = pg.AlgorithmSelection([weak] + twins, fraction_of_training=[0.8, 0.6], batch=batch)
        assert tuner.tune(graph, signal) is twins[0]
        values = [r["values"] for r in tuner.last_selection["rankers"]]
        assert values[1] == values[2] and min(values[1]) > min(values[0])
        assert tuner.last_selection["selected"] == 1


def test_training_split_and_dropout(host_engine):
    pg = host_engine
    graph, signal = sc.problem(pg)
    pre = pg.preprocessor(assume_immutability=True)
    recorders = [_Recorder(pg.PageRank(0.85, preprocessor=pre, tol=1e-6)), _Recorder(pg.HeatKernel(3, preprocessor=pre, tol=1e-6))]
    tuner = pg.AlgorithmSelection(recorders, fraction_of_training=[0.8, 0.6], combined_prediction=False)
    best, used = tuner._tune(graph, signal, graph_dropout=0.3)
    training, _ = pg.split(pg.to_signal(graph, signal), 0.6, seed=1)          # the last split's training part
    assert sorted(v for v in used if used[v] != 0) == sorted(v for v in training if training[v] != 0)
    assert len(used) == len(signal) and sum(1 for v in used if used[v] != 0) < sum(1 for v in signal if signal[v] != 0)
    whole = pg.AlgorithmSelection(recorders)._tune(graph, signal)[1]
    assert sorted(v for v in whole if whole[v] != 0) == sorted(v for v in signal if signal[v] != 0)
    # no dropout while the candidates are compared, the caller's own for the ranking that follows
    for recorder in recorders:
        assert recorder.calls and all(call == dict(graph_dropout=0) for call in recorder.calls)
        recorder.calls.clear()
    tuner = pg.AlgorithmSelection(recorders, fraction_of_training=0.8)
    tuner.rank(graph, signal, graph_dropout=0.3)
    final = [call for recorder in recorders for call in recorder.calls if call != dict(graph_dropout=0)]
    assert final == [dict(graph_dropout=0.3)]


def test_factories_return_the_reference_families(host_engine, fx):
    pg = host_engine
    assert _describe(pg.create_demo_filters()) == fx["demo_filters"]
    many = pg.create_many_filters()
    assert _describe(many) == fx["many_filters"]
    assert len({id(r.preprocessor) for r in many.values()}) == 2
    assert len({id(r.preprocessor) for r in pg.create_demo_filters().values()}) == 1
    shared = pg.preprocessor(assume_immutability=True)
    assert all(r.preprocessor is shared for r in pg.create_demo_filters(preprocessor=shared, tol=1e-6, max_iters=50).values())
    wrapped = pg.create_variations(pg.create_demo_filters(), {"": pg.Tautology, "+N": pg.Normalize})
    assert list(wrapped) == list(pg.create_demo_filters()) + [name + "+N" for name in pg.create_demo_filters()]
    assert all(isinstance(wrapped[name + "+N"], pg.Normalize) for name in pg.create_demo_filters())
    assert all(isinstance(r, pg.Normalize) for r in pg.create_variations(many, pg.Normalize).values())
    tuner = pg.AlgorithmSelection()
    assert [type(r).__name__ for r in tuner.rankers] == [row[1] for row in fx["demo_filters"]]
    assert any("selected the best among" in part and "heat kernel" in part and "AUC" in part and "0.100" in part
               for part in tuner.references())
    with pytest.raises(Exception):
        pg.AlgorithmSelection(tuning_backend="numpy")


def test_only_rankers_that_run_the_plain_loop_may_join_a_group(host_engine):
    """A personalization transform, a chained ranker, a graph hook, a postprocessor around the filter, f64 by tolerance, the chebyshev
    form or AbsorbingWalks keep a ranker out of every group, whichever place it has in the list."""
    pg = host_engine
    pre = pg.preprocessor(assume_immutability=True)
    key = pg.AlgorithmSelection._group_key
    plain = [pg.PageRank(alpha, preprocessor=pre, tol=1e-6) for alpha in (0.85, 0.9)]
    assert key(plain[0]) is not None and key(plain[0]) == key(plain[1]) and key(plain[0])[0] == "mixed_ppr"
    heat = [pg.HeatKernel(t, preprocessor=pre, tol=1e-6) for t in (1, 3)]
    assert key(heat[0]) is not None and key(heat[0]) == key(heat[1]) and key(heat[0])[0] == "mixed_poly"
    assert key(heat[0]) != key(plain[0])
    chained = pg.PageRank(0.9, preprocessor=pre, tol=1e-6)
    chained << pg.HeatKernel(2, preprocessor=pre, tol=1e-6)
    assert type(chained) is pg.PageRank

    class Hooked(pg.PageRank):
        def _prepare_graph(self, graph, *args, **kwargs):
            return graph
    for ranker in (pg.PageRank(0.9, preprocessor=pre, tol=1e-6, personalization_transform=pg.Normalize()), chained,
                   pg.HeatKernel(3, preprocessor=pre, tol=1e-6, personalization_transform=pg.Normalize()), Hooked(0.9, preprocessor=pre),
                   pg.Normalize(plain[0]), pg.PageRank(0.9, preprocessor=pre, tol=1e-9), pg.AbsorbingWalks(0.9, preprocessor=pre, tol=1e-6),
                   pg.HeatKernel(3, preprocessor=pre, tol=1e-6, coefficient_type="chebyshev"),
                   pg.PageRank(0.9, preprocessor=pre, tol=1e-6, use_quotient=pg.Normalize())):
        assert key(ranker) is None, type(ranker).__name__
    assert key(pg.PageRank(0.9, preprocessor=pre, tol=1e-6, use_quotient=False)) != key(plain[0])
    assert key(pg.PageRank(0.9, preprocessor=pre, tol=1e-5)) != key(plain[0])
    assert key(pg.PageRank(0.9, preprocessor=pg.preprocessor(assume_immutability=True), tol=1e-6)) != key(plain[0])
