"""DEV-CONTAINER-ONLY: fixtures of the rank-based measures and of the measure combinations (tests/test_ranking_host.py,
tests/test_gpu_ranking.py) from the reference, imported read-only as in make_golden_supervised.py (numpy backend, the `wget` shim,
epsilon() replaced by the f32 epsilon while the measures are evaluated; the numpy engine's to_primitive, np.array(obj, copy=False),
is replaced by np.asarray, which is what it meant before numpy 2 began to refuse it).  Output: tests/golden/golden_ranking.json -- seed lists,
parameters and the reference's f64 results, no vectors.

Score bases: the five of make_golden_supervised.py (seeds, pagerank, pagerank_max, zeros, ones; the first, fourth and fifth are the
tie-laden ones).  Known scores: `binary`, the indicator of the `known` node list, and `graded`, values in {0, 0.25, 0.5, 1} with ties.
EVERY score base and every known vector is rounded to f32 and back to f64 before the reference sees it: the engine stores f32, so the
tie structure and the order are then the same on both sides (asserted: the rounding is idempotent and what is evaluated is what was
rounded; for the constant, indicator and graded vectors it changes nothing at all).  The two PageRank bases are rebuilt by the tests
with the engine's own PageRank, as the supervised tests do: they agree with the reference's to f32 rounding, not to the bit.

Cases (each records "value", or "nonfinite": "nan" | "inf" | "-inf", or "raises"):
  NDCG                 base x known x k in {None, 1, 10, relevant rows of the known vector, n} x without / with the exclude list
  SpearmanCorrelation  base x known x without / with the exclude list
  combinations         AM, GM, Disparity, Parity over the pairs (AUC, pRule) and (NDCG@10, Cos) of the binary known scores, in the modes
                         weights  constructor, weights [1, 2], the constructor's threshold default (0, 1)
                         zero     constructor, members (A, B, A), weights [1, 0, 0.5]: the middle member is skipped, the sign still alternates
                         add      built with add(): the default (-inf, inf) for A, max_val = 0.8 for B with weight 2
                         hinge    (AM over (AUC, pRule) only) differentiable=True, thresholds [(0, 1), (0, 0.8)], weights [1, 10]
                       x base x without / with the exclude list

Run:  PYGRANK_REFERENCE=<checkout of the reference> python tests/golden/make_golden_ranking.py
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
    # the numpy engine's to_primitive is np.array(obj, copy=False), which numpy 2 refuses whenever a copy is needed (a Python float
    # always needs one): np.asarray is what that call meant under numpy 1.  GM and the differentiable hinge go through it.
    _ENGINE.to_primitive = np.asarray
    _ENGINE.epsilon = _ENGINE_EPSILON if value is None else (lambda: value)
    reference_backend.load_backend("numpy")
    assert reference_backend.epsilon() == pg.epsilon() == (_ENGINE_EPSILON() if value is None else value)


PAGERANK = dict(alpha=0.85, tol=1e-9, max_iters=1000)
GRAPHS = ["er10k", "rmat10_dir", "weighted300"]
BASES = ["seeds", "pagerank", "pagerank_max", "zeros", "ones"]
KNOWNS = ["binary", "graded"]
COMBINATIONS = ["AM", "GM", "Disparity", "Parity"]
PAIRS = ["auc_prule", "ndcg_cos"]
MODES = ["weights", "zero", "add"]


def f32(values):
    rounded = np.asarray(values, dtype=np.float32).astype(np.float64)
    assert np.array_equal(np.asarray(rounded, dtype=np.float32).astype(np.float64), rounded)
    return rounded


def encode(case, value):
    value = float(value)
    if math.isfinite(value):
        case["value"] = value
    else:
        case["nonfinite"] = "nan" if math.isnan(value) else ("inf" if value > 0 else "-inf")


def record(case, evaluate):
    try:
        encode(case, evaluate())
    except Exception as e:
        case["raises"] = type(e).__name__ + ": " + str(e)
    return case


def combination(name, pair, mode, known, exclude):
    """The same construction as tests/rank_common.py:combination."""
    if pair == "auc_prule":
        a, b = pg.AUC(known, exclude), pg.pRule(known, exclude)
    else:
        a, b = pg.NDCG(known, exclude, k=10), pg.Cos(known, exclude)
    cls = getattr(pg, name)
    if mode == "weights":
        return cls([a, b], weights=[1., 2.])
    if mode == "zero":
        return cls([a, b, a], weights=[1., 0., 0.5])
    if mode == "add":
        return cls().add(a).add(b, weight=2., max_val=0.8)
    return cls([a, b], weights=[1., 10.], thresholds=[(0, 1), (0, 0.8)], differentiable=True)


def main():
    out = dict(pagerank=PAGERANK, epsilon=EPS, bases=BASES, knowns=KNOWNS, combinations=COMBINATIONS, pairs=PAIRS, modes=MODES, graphs={})
    warnings.simplefilter("ignore")
    for index, key in enumerate(GRAPHS):
        A, directed, p = cases.GRAPHS[key]()
        graph = pg.AdjacencyWrapper(A, directed=directed)
        n = A.shape[0]
        seeds = [int(v) for v in np.flatnonzero(p)]
        rng = np.random.default_rng(300 + index)
        known_nodes = sorted(set(seeds[:(len(seeds) + 1) // 2]) | {int(v) for v in rng.choice(n, max(3, n // 20), replace=False)})
        exclude_nodes = sorted(int(v) for v in rng.choice(n, n // 5, replace=False))
        grades = rng.choice([0.25, 0.5, 1.0], len(known_nodes))
        graded = {str(g): [int(v) for v, x in zip(known_nodes, grades) if x == g] for g in (0.25, 0.5, 1.0)}
        known_vectors = dict(binary=np.zeros(n), graded=np.zeros(n))
        known_vectors["binary"][known_nodes] = 1.0
        for g, nodes in graded.items():
            known_vectors["graded"][nodes] = float(g)
        signal = pg.to_signal(graph, {v: 1.0 for v in seeds})
        set_epsilon(None)
        ranks = pg.PageRank(**PAGERANK).rank(graph, signal)
        set_epsilon(EPS)
        bases = dict(seeds=signal.np, pagerank=ranks.np, pagerank_max=pg.Normalize("max").transform(ranks).np, zeros=np.zeros(n), ones=np.ones(n))
        bases = {name: f32(values) for name, values in bases.items()}
        for name in ("seeds", "zeros", "ones"):
            assert len(np.unique(bases[name])) <= 2                 # tie-laden: one or two tie groups
        knowns = {}
        for name, values in known_vectors.items():
            assert np.array_equal(f32(values), values)              # f32 holds the indicator and the grades exactly
            knowns[name] = pg.to_signal(graph, f32(values))
        keep = np.ones(n, dtype=bool)
        keep[exclude_nodes] = False
        assert 0 < known_vectors["binary"][keep].sum() < keep.sum(), key
        recorded = []
        for excluded in (False, True):
            exclude = exclude_nodes if excluded else None
            for base in BASES:
                scores = bases[base]

                def signal_of():
                    fresh = pg.to_signal(graph, scores.copy())
                    assert np.array_equal(np.asarray(fresh.np, dtype=np.float64), scores)       # what is evaluated is what was rounded
                    return fresh
                for known_name in KNOWNS:
                    known = knowns[known_name]
                    relevant = int((known_vectors[known_name] != 0).sum())
                    for label, k in (("none", None), ("1", 1), ("10", 10), ("relevant", relevant), ("n", n)):
                        case = dict(measure="NDCG", base=base, known=known_name, k=label, excluded=excluded)
                        recorded.append(record(case, lambda: pg.NDCG(known, exclude, k=k).evaluate(signal_of())))
                    case = dict(measure="SpearmanCorrelation", base=base, known=known_name, excluded=excluded)
                    recorded.append(record(case, lambda: pg.SpearmanCorrelation(known, exclude).evaluate(signal_of())))
                for name in COMBINATIONS:
                    for pair in PAIRS:
                        for mode in MODES + (["hinge"] if (name, pair) == ("AM", "auc_prule") else []):
                            case = dict(measure=name, pair=pair, mode=mode, base=base, excluded=excluded)
                            recorded.append(record(case, lambda: combination(name, pair, mode, knowns["binary"], exclude).evaluate(signal_of())))
        out["graphs"][key] = dict(directed=bool(directed), seeds=seeds, known=known_nodes, graded=graded, exclude=exclude_nodes, cases=recorded)
        for case in recorded:
            print(key, {k: v for k, v in case.items() if k not in ("value", "nonfinite", "raises")},
                  case.get("value", case.get("nonfinite", "raises: " + case.get("raises", ""))))
    # what the reference does where NDCG divides by an IDCG of 0 (no relevant node is evaluated) and where no node is evaluated at
    # all, on weighted300 with constant scores
    A, directed, _ = cases.GRAPHS["weighted300"]()
    graph = pg.AdjacencyWrapper(A, directed=directed)
    n = A.shape[0]
    ones, nothing, everybody = pg.to_signal(graph, np.ones(n)), pg.to_signal(graph, np.zeros(n)), {v: 1.0 for v in range(n)}
    some = pg.to_signal(graph, {0: 1.0, 5: 0.5})
    out["edges"] = dict(
        ndcg_idcg_zero=record({}, lambda: pg.NDCG(nothing).evaluate(ones)),
        ndcg_relevant_all_excluded=record({}, lambda: pg.NDCG(some, [0, 5]).evaluate(ones)),
        ndcg_nothing_kept=record({}, lambda: pg.NDCG(some, everybody).evaluate(ones)),
        ndcg_k_too_large=record({}, lambda: pg.NDCG(some, k=n + 1)),
        spearman_constant_known=record({}, lambda: pg.SpearmanCorrelation(nothing).evaluate(some)))
    print("edges", out["edges"])
    path = os.path.join(HERE, "golden_ranking.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
