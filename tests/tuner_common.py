"""Shared by the tuner's tests (host double and GPU): the fixture of tests/golden/make_golden_tuner.py and the replay checks."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "golden_tuner.json")) as f:
        return json.load(f)


def planted(pg, fx):
    """(graph, seed signal, community signal) of the fixture's planted community."""
    import cases
    A, directed, _ = cases.GRAPHS[fx["community"]["graph"]]()
    graph = pg.AdjacencyWrapper(A, directed=directed)
    seeds = pg.to_signal(graph, {v: 1.0 for v in fx["seeds"]})
    truth = pg.to_signal(graph, {v: 1.0 for v in fx["community_nodes"]})
    return graph, seeds, truth


def tuner_for(pg, fx, **more):
    return pg.ParameterTuner(verbose=False, **fx["tuner_args"], **more)


def tuner_loss(pg, tuner, seeds):
    """The loss ParameterTuner hands to its optimiser for this personalization (first tuning run)."""
    tuner.last_tune = dict(fused_steps=0, unfused_steps=0)
    return tuner._loss(tuner._splits(pg.to_signal(seeds, None), 0), (), {})


def replay(fx, loss):
    """Check 3 of the tuner: the fixture's candidates of every step through `loss.many`; |loss - reference| <= flip budget + 1e-12
    per candidate, and the reference's choice wherever its best and runner-up are further apart than their two budgets.  Returns
    the losses of every step."""
    got_all, skipped = [], 0
    steps = fx["tuner"]["steps"]
    for step in steps:
        got = loss.many(step["candidates"])
        got_all.append(got)
        for mine, want, budget in zip(got, step["losses"], step["flip_budget"]):
            assert abs(mine - want) <= budget + 1e-12, (mine, want, budget)
        order = sorted(range(len(got)), key=lambda i: step["losses"][i])
        best, second = order[0], order[1]
        decisive = step["losses"][second] - step["losses"][best] > step["flip_budget"][best] + step["flip_budget"][second]
        assert decisive == step["argmin_checked"]
        if decisive:
            assert min(range(len(got)), key=lambda i: got[i]) == step["chosen"]
        else:
            skipped += 1
    assert skipped / len(steps) <= 0.25
    assert abs(skipped / len(steps) - fx["tuner"]["skipped_share"]) < 1e-12
    return got_all


def end_to_end(pg, fx, tuner):
    """Check 4: a full run on the planted community."""
    graph, seeds, truth = planted(pg, fx)
    ranks = tuner(graph, seeds)
    assert isinstance(ranks, pg.GraphSignal)
    lo, hi = fx["tuner_args"]["min_vals"], fx["tuner_args"]["max_vals"]
    assert len(tuner.last_params) == len(hi)
    assert all(a <= p <= b for a, p, b in zip(lo, tuner.last_params, hi))
    held_out = pg.AUC(truth, exclude=seeds)(ranks)
    print(f"held-out AUC {held_out:.6f} (reference {fx['tuner']['held_out_auc']:.6f}), last_params {tuner.last_params}, {tuner.last_tune}")
    assert held_out >= fx["tuner"]["held_out_auc"] - fx["tuner"]["largest_flip_budget"]
    assert isinstance(tuner.tune(graph, seeds), pg.NodeRanking)
    assert any("parameters tuned" in part and "AUC" in part for part in tuner.references())
    return graph, seeds, np.asarray(ranks.np, dtype=np.float64)
