"""DEV-CONTAINER-ONLY: fixtures of the fairness postprocessors (tests/test_fairness_host.py, tests/test_gpu_fairness.py) from the
reference, imported read-only with the `wget` shim of SURVEY.md 8c under its numpy backend.  Output:
tests/golden/golden_fairness.json -- seed lists, sensitive lists, parameters and the reference's f64 scalars, no score vectors.

Per graph of cases.GRAPHS (er10k, rmat10_dir, weighted300), with PageRank (PAGERANK below) as the base ranker, the graph's seeds as
the personalization and a random fifth of the nodes (recorded seed) as the sensitive group:
  points     the reference's loss -- the closure of FairPersonalizer.rank itself, caught where it is handed to `optimize` -- at 13
             parameter vectors of FairPersonalizer(ranker, 0.8, pRule_weight=10, parameter_buckets, error_skewing): the box centre, and
             for buckets 1 and 2, error_skewing both ways, a random point, one with the last parameter 0 and one with it 1.  The
             pRule and the error of each point are recomputed from the closure's own objects and ASSERTED to combine into its loss.
  descent    the default FairPersonalizer(ranker, 0.8, pRule_weight=10): the pRule of the original scores, the loss at the starting
             point (the box centre), the final loss, the pRule of the final scores and the iteration count the runs are fixed at.
             ASSERTED: the final loss is at least MIN_IMPROVEMENT below the starting loss (the end-to-end tests ask for half of the
             recorded improvement) and the final pRule is above the original one.  The reference's descent is run on each draw of
             the sensitive group in seed order; a draw that does not meet the condition is dropped and the next seed is tried, up
             to MAX_DRAWS descents.  A graph where none of them meets it has "descent": null and keeps its first draw for the
             points and the AdHocFairness case; "descents_tried" lists every descent that was run, kept or dropped.
  adhoc      AdHocFairness("B") on the original scores: the sums of the sensitive and of the other scores after the transform, the
             pRule before and after.

Run:  PYGRANK_REFERENCE=<checkout of the reference> python tests/golden/make_golden_fairness.py
"""
import json
import os
import sys
import tempfile
import types
import warnings
import importlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
os.environ["pygrankBackend"] = "numpy"
os.environ["HOME"] = tempfile.mkdtemp(prefix="pgh_golden_home_")   # import writes ~/.pygrank/config.json
sys.dont_write_bytecode = True
sys.modules["wget"] = types.ModuleType("wget")                      # pygrank/benchmarks/download.py:3
sys.path.insert(0, os.environ["PYGRANK_REFERENCE"])

import numpy as np  # noqa: E402
import pygrank as pg  # noqa: E402

import cases  # noqa: E402

PAGERANK = dict(alpha=0.85, tol=1e-9, max_iters=1000)
FAIR = dict(target_pRule=0.8, pRule_weight=10)
GRAPHS = ["er10k", "rmat10_dir", "weighted300"]
MIN_IMPROVEMENT = 0.05
MAX_DRAWS = 8
reference_fairness = importlib.import_module("pygrank.algorithms.postprocess.fairness")
_OPTIMIZE = reference_fairness.optimize


def closure_of(loss):
    return dict(zip(loss.__code__.co_freevars, (cell.cell_contents for cell in loss.__closure__)))


def with_caught_loss(personalizer, graph, signal, sensitive, inside):
    """Runs personalizer.rank with `optimize` replaced by `inside(loss, optimize arguments) -> parameters`: the loss is the reference's
    own closure, evaluated while the ranker's convergence manager is the fixed-iteration one."""
    reference_fairness.optimize = lambda loss, **kwargs: inside(loss, kwargs)
    try:
        return personalizer.rank(graph, signal, sensitive=sensitive)
    finally:
        reference_fairness.optimize = _OPTIMIZE


def point_cases(rng):
    points = [dict(buckets=1, skew=False, params=[0.5, 0.5, 0.0, 0.0, 0.5])]
    for buckets in (1, 2):
        for skew in (False, True):
            for last in (None, 0.0, 1.0):
                body = []
                for _ in range(buckets):
                    body += [float(rng.random()), float(rng.random()), float(rng.uniform(-5, 5)), float(rng.uniform(-5, 5))]
                points.append(dict(buckets=buckets, skew=skew, params=body + [float(rng.random()) if last is None else last]))
    return points


def record_points(graph, signal, sensitive, points):
    for buckets in (1, 2):
        for skew in (False, True):
            mine = [p for p in points if p["buckets"] == buckets and p["skew"] == skew]
            personalizer = pg.FairPersonalizer(pg.PageRank(**PAGERANK), parameter_buckets=buckets, error_skewing=skew, max_residual=1, **FAIR)

            def inside(loss, kwargs):
                env = closure_of(loss)
                owner = env["self"]
                for point in mine:
                    point["loss"] = float(loss(point["params"]))
                    prior = owner._FairPersonalizer__culep(env["training"].np, env["sensitive"], env["original_ranks"], point["params"])
                    ranks = owner.ranker.rank(env["graph"], personalization=prior)
                    point["pRule"] = float(env["fairness_measure"](ranks))
                    point["error"] = float(pg.Mabs(env["original_ranks"])(ranks))
                    combined = -point["error"] * pg.Mabs([1, 0]).best_direction() - FAIR["pRule_weight"] * min(FAIR["target_pRule"], point["pRule"])
                    assert abs(combined - point["loss"]) <= 1e-12, (point, combined)
                return [(a + b) / 2 for a, b in zip(kwargs["min_vals"], kwargs["max_vals"])]
            with_caught_loss(personalizer, graph, signal, sensitive, inside)


def record_descent(graph, signal, sensitive):
    ranker = pg.PageRank(**PAGERANK)
    original = ranker.rank(graph, signal)
    out = dict(original_pRule=float(pg.pRule(sensitive)(original)))
    personalizer = pg.FairPersonalizer(ranker, **FAIR)

    def inside(loss, kwargs):
        start = [(a + b) / 2 for a, b in zip(kwargs["min_vals"], kwargs["max_vals"])]
        out["start_params"], out["start_loss"] = start, float(loss(start))
        out["iterations"] = int(personalizer.ranker.convergence.max_iters)
        result = _OPTIMIZE(loss, verbose=False, **kwargs)
        out["final_params"], out["final_loss"] = [float(v) for v in result], float(loss(result))
        return result
    ranks = with_caught_loss(personalizer, graph, signal, sensitive, inside)
    out["final_pRule"] = float(pg.pRule(sensitive)(ranks))
    return out, original


def draw(n, seed):
    return sorted(int(v) for v in np.random.default_rng(seed).choice(n, n // 5, replace=False))


def main():
    warnings.simplefilter("ignore")
    out = dict(pagerank=PAGERANK, fair=FAIR, min_improvement=MIN_IMPROVEMENT, graphs={})
    for index, key in enumerate(GRAPHS):
        A, directed, p = cases.GRAPHS[key]()
        graph = pg.AdjacencyWrapper(A, directed=directed)
        n = A.shape[0]
        seeds = [int(v) for v in np.flatnonzero(p)]
        signal = pg.to_signal(graph, {v: 1.0 for v in seeds})
        first = 300 + 100 * index
        descent, chosen, tried = None, first, []
        for sensitive_seed in range(first, first + MAX_DRAWS):
            sensitive = pg.to_signal(graph, {v: 1.0 for v in draw(n, sensitive_seed)})
            candidate, _ = record_descent(graph, signal, sensitive)
            print(key, "sensitive seed", sensitive_seed, candidate)
            tried.append(dict(sensitive_seed=sensitive_seed, start_loss=candidate["start_loss"], final_loss=candidate["final_loss"],
                              original_pRule=candidate["original_pRule"], final_pRule=candidate["final_pRule"]))
            if candidate["final_loss"] <= candidate["start_loss"] - MIN_IMPROVEMENT and candidate["final_pRule"] > candidate["original_pRule"]:
                descent, chosen = candidate, sensitive_seed
                break
        if descent is None:
            print(key, "descent case dropped: none of", MAX_DRAWS, "descents improves by", MIN_IMPROVEMENT)
        sensitive_seed = chosen
        sensitive_nodes = draw(n, sensitive_seed)
        sensitive = pg.to_signal(graph, {v: 1.0 for v in sensitive_nodes})
        original = pg.PageRank(**PAGERANK).rank(graph, signal)
        points = point_cases(np.random.default_rng(400 + index))
        record_points(graph, signal, sensitive, points)
        for point in points:
            print(key, point)
        fair = pg.AdHocFairness(method="B").transform(original, sensitive=sensitive)
        s = sensitive.np
        adhoc = dict(sensitive_sum=float(np.sum(fair.np * s)), other_sum=float(np.sum(fair.np * (1 - s))),
                     pRule_before=float(pg.pRule(sensitive)(original)), pRule_after=float(pg.pRule(sensitive)(fair)))
        print(key, adhoc)
        out["graphs"][key] = dict(directed=bool(directed), seeds=seeds, sensitive_seed=sensitive_seed, sensitive=sensitive_nodes,
                                  points=points, descent=descent, descents_tried=tried, adhoc=adhoc)
    path = os.path.join(HERE, "golden_fairness.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
