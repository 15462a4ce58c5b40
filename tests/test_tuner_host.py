"""The tuner layer on the host test double (no GPU): split, optimize and ParameterTuner against the reference's recorded behaviour
(tests/golden/golden_tuner.json).  The double lacks include/pgh_tune.h, so ParameterTuner's `many` takes its unfused route here."""
import pytest

import tuner_common as tc


@pytest.fixture(scope="module")
def fx():
    return tc.fixture()


def test_split_equals_the_reference(host_engine, fx):
    pg = host_engine
    graph, seeds, _ = tc.planted(pg, fx)
    assert len(fx["split"]) == 12
    for case in fx["split"]:
        tr, te = pg.split(seeds, case["fraction"], case["seed"])
        assert sorted(v for v in tr if tr[v] != 0) == case["signal_training"], case
        assert sorted(v for v in te if te[v] != 0) == case["signal_test"], case
        ltr, lte = pg.split(list(fx["seeds"]), case["fraction"], case["seed"])
        assert (ltr, lte) == (case["list_training"], case["list_test"]), case
    mtr, mte = pg.split({"a": list(fx["seeds"][:10]), "b": list(fx["seeds"][10:17])}, 0.5, 1)
    assert mtr == fx["split_mapping"]["training"] and mte == fx["split_mapping"]["test"]
    same = pg.split(seeds, 1)
    assert same[0] is seeds and same[1] is seeds


def _beale(p):
    return (1.5 - p[0] + p[0] * p[1]) ** 2 + (2.25 - p[0] + p[0] * p[1] ** 2) ** 2 + (2.625 - p[0] + p[0] * p[1] ** 3) ** 2


def _quadratic(p):
    return (p[0] - 3) ** 2 + 2 * (p[1] + 4) ** 2 + 0.5 * (p[2] - 7) ** 2 + 0.25 * p[0] * p[1]


class _Batched:
    """A loss with `many`: records every step's candidate list."""

    def __init__(self, fn):
        self.fn, self.steps, self.single_calls = fn, [], 0

    def __call__(self, w):
        self.single_calls += 1
        return self.fn(w)

    def many(self, candidates):
        self.steps.append([list(w) for w in candidates])
        return [self.fn(w) for w in candidates]


@pytest.mark.parametrize("name, fn", [("optimize_beale", _beale), ("optimize_quadratic", _quadratic)])
def test_optimize_replays_the_reference_trace(fx, name, fn):
    from pygrank_amd import optimize
    rec = fx[name]
    calls = []

    def watched(w):
        calls.append(list(w))
        return fn(w)
    result = optimize(watched, verbose=False, **rec["args"])
    flat = [w for step in rec["steps"] for w in step["candidates"]]
    assert len(calls) == len(flat)
    for mine, want in zip(calls, flat):
        assert max(abs(a - b) for a, b in zip(mine, want)) <= 1e-12
    assert max(abs(a - b) for a, b in zip(result, rec["result"])) <= 1e-12
    batched = _Batched(fn)
    assert optimize(batched, verbose=False, **rec["args"]) == result
    assert batched.single_calls == 0 and len(batched.steps) == len(rec["steps"])
    for mine, step in zip(batched.steps, rec["steps"]):
        assert len(mine) == len(step["candidates"])
        for a, b in zip(mine, step["candidates"]):
            assert max(abs(x - y) for x, y in zip(a, b)) <= 1e-12
        losses = [fn(w) for w in mine]
        assert min(range(len(losses)), key=lambda i: losses[i]) == step["chosen"]


def test_tuner_replay_on_the_host_double(host_engine, fx):
    pg = host_engine
    _, seeds, _ = tc.planted(pg, fx)
    tuner = tc.tuner_for(pg, fx)
    loss = tc.tuner_loss(pg, tuner, seeds)
    assert callable(getattr(loss, "many", None))
    tc.replay(fx, loss)
    assert tuner.last_tune["fused_steps"] == 0 and tuner.last_tune["unfused_steps"] == len(fx["tuner"]["steps"])


def test_tuner_end_to_end_on_the_host_double(host_engine, fx):
    pg = host_engine
    tuner = tc.tuner_for(pg, fx)
    graph, seeds, _ = tc.end_to_end(pg, fx, tuner)
    assert tuner.last_tune["fused_steps"] == 0 and tuner.last_tune["unfused_steps"] > 0
    # a user's generator and another measure: the reference's one-probe-at-a-time loss
    ppr = pg.ParameterTuner(lambda params: pg.PageRank(alpha=params[0]), measure=pg.AUC, deviation_tol=0.01, max_vals=[0.99],
                            min_vals=[0.5], verbose=False)
    assert not hasattr(ppr._loss(ppr._splits(seeds, 0), (), {}), "many")
    assert isinstance(ppr(graph, seeds), pg.GraphSignal) and 0.5 <= ppr.last_params[0] <= 0.99
    cos = pg.ParameterTuner(measure=pg.Cos, verbose=False, **fx["tuner_args"])
    assert not hasattr(cos._loss(cos._splits(seeds, 0), (), {}), "many")
    assert isinstance(cos(graph, seeds), pg.GraphSignal) and len(cos.last_params) == len(fx["tuner_args"]["max_vals"])
    assert cos.last_tune == dict(fused_steps=0, unfused_steps=0)
    with pytest.raises(Exception):
        pg.ParameterTuner(tuning_backend="numpy")


def test_self_clear_dict_and_directions(host_engine):
    pg = host_engine
    d = pg.SelfClearDict()
    d["a"] = 1
    d["b"] = 2
    assert dict(d) == {"b": 2}
    assert pg.AUC([1, 0]).best_direction() == 1 and pg.Cos([1, 0]).best_direction() == 1
    assert pg.Mabs([1, 0]).best_direction() == -1
