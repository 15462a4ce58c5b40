"""DEV-CONTAINER-ONLY: fixtures of the supervised measures (tests/test_supervised_host.py, tests/test_gpu_supervised.py) from the
reference, imported read-only with the `wget` shim of SURVEY.md 8c under its numpy backend.  Output:
tests/golden/golden_supervised.json -- seed lists, parameters and the reference's f64 results, no score vectors.

The reference's numpy backend answers epsilon() with the f64 epsilon; this engine follows the reference's pytorch backend, whose
epsilon is the f32 one.  So the backend's `epsilon` is REPLACED here at run time by float(np.finfo(np.float32).eps) while the measures
are evaluated: the recorded BinaryCrossEntropy, KLDivergence and MKLDivergence are the reference's formulas in f64 with that shift.
The PageRank run behind two of the score bases keeps the backend's own epsilon, as in make_golden_unsupervised.py.

A score vector is one of the five bases of make_golden_unsupervised.py on a graph of cases.GRAPHS:
  seeds         1 on the graph's seed nodes, 0 elsewhere
  pagerank      PageRank (PAGERANK below) of the seeds, as the filter returns it
  pagerank_max  the same run through Normalize("max")
  zeros, ones   constant vectors
The known scores are the indicator of a SECOND seed list (`known`: half of the graph's seeds and a random twentieth of the nodes), and
every (measure, base) pair is recorded without and with an exclude list (`exclude`: a random fifth of the nodes).  A case records the
f64 value, or that the reference raised ("raises"), or the kind of a non-finite value ("nonfinite": "nan", "inf" or "-inf").

Three measures subtract sums of like size.  The generator ASSERTS the conditioning of every finite case it records for them, and the
tests divide their bound by these floors:
  KLDivergence, MKLDivergence   KL >= KL_FLOOR  (the value is (sum (s+eps) log(s+eps) - sum (s+eps) log(k+eps)) / S - log S + log K)
  PearsonCorrelation            the variance of the scores and of the known scores >= PEARSON_FLOOR times their mean square
  TNR                           its denominator sum (1 - k / max k) >= TNR_FLOOR times the number of evaluated nodes

BinaryCrossEntropy takes log(1 - s + eps), which turns on the last bit of a score next to 1: the reference's Normalize("max") divides,
so the largest entry of pagerank_max is exactly 1 here, and the tests build that base the same way (x / max x, rounded once to f32).

Run:  PYGRANK_REFERENCE=<checkout of the reference> python tests/golden/make_golden_supervised.py
"""
import importlib
import json
import math
import os
import sys
import tempfile
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
os.environ["pygrankBackend"] = "numpy"
os.environ["HOME"] = tempfile.mkdtemp(prefix="pgh_golden_home_")   # import writes ~/.pygrank/config.json
sys.dont_write_bytecode = True
sys.modules["wget"] = types.ModuleType("wget")                      # pygrank/benchmarks/download.py:3
sys.path.insert(0, os.environ["PYGRANK_REFERENCE"])

import numpy as np  # noqa: E402
import pygrank as pg  # noqa: E402
import pygrank.core.backend as reference_backend  # noqa: E402

import cases  # noqa: E402

EPS = float(np.finfo(np.float32).eps)
_ENGINE = importlib.import_module("pygrank.core.backend.numpy")
_ENGINE_EPSILON = _ENGINE.epsilon


def set_epsilon(value):
    """Replaces epsilon() in the numpy engine itself and publishes it again (the loader republishes the engine's functions whenever
    a backend is loaded); None restores the engine's own."""
    _ENGINE.epsilon = _ENGINE_EPSILON if value is None else (lambda: value)
    reference_backend.load_backend("numpy")
    assert reference_backend.epsilon() == pg.epsilon() == (_ENGINE_EPSILON() if value is None else value)


PAGERANK = dict(alpha=0.85, tol=1e-9, max_iters=1000)
GRAPHS = ["er10k", "rmat10_dir", "weighted300"]
BASES = ["seeds", "pagerank", "pagerank_max", "zeros", "ones"]
MEASURES = ["MaxDifference", "Mabs", "L1", "RMabs", "MSQ", "MSQRT", "L2", "Euclidean", "Cos", "Dot", "AUC",
            "Accuracy", "TPR", "TNR", "PPV", "pRule", "L2Disparity", "BinaryCrossEntropy", "CrossEntropy", "KLDivergence",
            "MKLDivergence", "PearsonCorrelation", "MannWhitneyParity"]
KL_FLOOR, PEARSON_FLOOR, TNR_FLOOR = 1e-2, 1e-3, 1e-3


def encode(case, value):
    value = float(value)
    if math.isfinite(value):
        case["value"] = value
    else:
        case["nonfinite"] = "nan" if math.isnan(value) else ("inf" if value > 0 else "-inf")


def conditioned(measure, value, known, scores, keep):
    """The asserted floors of the cancelling measures, over the evaluated nodes."""
    k, s = known[keep], scores[keep]
    if measure in ("KLDivergence", "MKLDivergence"):
        kl = value if measure == "KLDivergence" else -value * len(s)
        return kl >= KL_FLOOR
    if measure == "PearsonCorrelation":
        return all(float(np.var(x)) >= PEARSON_FLOOR * float(np.mean(x * x)) for x in (k, s))
    if measure == "TNR":
        return float(np.sum(1 - k / np.max(k))) >= TNR_FLOOR * len(k)
    return True


def main():
    out = dict(pagerank=PAGERANK, epsilon=EPS, floors=dict(KL=KL_FLOOR, Pearson=PEARSON_FLOOR, TNR=TNR_FLOOR), measures=MEASURES, graphs={})
    warnings.simplefilter("ignore")                                 # log(0), 0 * inf and constant inputs are recorded, not reported
    for index, key in enumerate(GRAPHS):
        A, directed, p = cases.GRAPHS[key]()
        graph = pg.AdjacencyWrapper(A, directed=directed)
        n = A.shape[0]
        seeds = [int(v) for v in np.flatnonzero(p)]
        rng = np.random.default_rng(100 + index)
        known_nodes = sorted(set(seeds[:(len(seeds) + 1) // 2]) | {int(v) for v in rng.choice(n, max(3, n // 20), replace=False)})
        exclude_nodes = sorted(int(v) for v in rng.choice(n, n // 5, replace=False))
        signal = pg.to_signal(graph, {v: 1.0 for v in seeds})
        known = pg.to_signal(graph, {v: 1.0 for v in known_nodes})
        set_epsilon(None)                                           # the score bases are those of the unsupervised fixture: the
        ranks = pg.PageRank(**PAGERANK).rank(graph, signal)         # reference's convergence check reads epsilon() too
        set_epsilon(EPS)
        bases = dict(seeds=signal.np, pagerank=ranks.np, pagerank_max=pg.Normalize("max").transform(ranks).np, zeros=np.zeros(n),
                     ones=np.ones(n))
        recorded = []
        for excluded in (False, True):
            keep = np.ones(n, dtype=bool)
            if excluded:
                keep[exclude_nodes] = False
            assert 0 < known.np[keep].sum() < keep.sum(), key        # both classes stay
            for measure in MEASURES:
                for base in BASES:
                    values = np.asarray(bases[base], dtype=np.float64)
                    case = dict(measure=measure, base=base, excluded=excluded)
                    try:
                        encode(case, getattr(pg, measure)(known, exclude_nodes if excluded else None)
                               .evaluate(pg.to_signal(graph, values.copy())))
                    except Exception as e:
                        case["raises"] = str(e)
                    if "value" in case:
                        normalized = values / np.abs(values).sum() if np.abs(values).sum() != 0 else values
                        assert conditioned(measure, case["value"], known.np, normalized, keep), (key, case)
                    recorded.append(case)
        out["graphs"][key] = dict(directed=bool(directed), seeds=seeds, known=known_nodes, exclude=exclude_nodes, cases=recorded)
        for case in recorded:
            print(key, case["measure"], case["base"], "excluded" if case["excluded"] else "all",
                  case.get("value", case.get("nonfinite", "raises: " + case.get("raises", ""))))
    out["best_direction"] = {measure: int(getattr(pg, measure)([1, 0]).best_direction()) for measure in MEASURES}
    print("best_direction", out["best_direction"])
    path = os.path.join(HERE, "golden_supervised.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
