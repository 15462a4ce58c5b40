"""DEV-CONTAINER-ONLY: fixtures of the unsupervised measures (tests/test_unsupervised_host.py, tests/test_gpu_unsupervised.py) from the
reference, imported read-only with the `wget` shim of SURVEY.md 8c under its numpy backend.  Output:
tests/golden/golden_unsupervised.json -- seed lists, parameters and the reference's f64 results, no score vectors.

A score vector is `scale` times one of five bases on a graph of cases.GRAPHS:
  seeds         1 on the recorded seed nodes, 0 elsewhere
  pagerank      PageRank (PAGERANK below) of the seeds, as the filter returns it
  pagerank_max  the same run through Normalize("max")
  zeros, ones   constant vectors
Every case names its measure, its base, its scale and the measure's keyword arguments; it records the value, or that the reference
raised.  Infinity is written as the string "inf".

Run:  python tests/golden/make_golden_unsupervised.py
"""
import json
import math
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
os.environ["pygrankBackend"] = "numpy"
os.environ["HOME"] = tempfile.mkdtemp(prefix="pgh_golden_home_")   # import writes ~/.pygrank/config.json
sys.dont_write_bytecode = True
sys.modules["wget"] = types.ModuleType("wget")                      # pygrank/benchmarks/download.py:3
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import pygrank as pg  # noqa: E402

import cases  # noqa: E402

PAGERANK = dict(alpha=0.85, tol=1e-9, max_iters=1000)
GRAPHS = ["er10k", "rmat10_dir", "weighted300"]
# (case name, base, scale, Conductance keyword arguments)
CONDUCTANCE = [
    ("seeds", "seeds", 1, {}),
    ("pagerank_max", "pagerank_max", 1, {}),
    ("pagerank_autofix", "pagerank", 1, dict(autofix=True)),
    ("pagerank_strict", "pagerank", 1, dict(autofix=False)),
    ("tripled_autofix", "pagerank_max", 3, dict(autofix=True)),
    ("tripled_strict", "pagerank_max", 3, dict(autofix=False)),
    ("cut_ratio_only", "pagerank_max", 1, dict(cut_ratio_only=True)),
    ("max_rank_2", "pagerank_max", 1.5, dict(max_rank=2)),
    ("zeros", "zeros", 1, {}),
    ("full", "ones", 1, {}),
]
DENSITY = [("seeds", "seeds", 1), ("pagerank_max", "pagerank_max", 1), ("pagerank", "pagerank", 1), ("tripled", "pagerank_max", 3),
           ("zeros", "zeros", 1), ("full", "ones", 1)]


def encode(value):
    value = float(value)
    return "inf" if math.isinf(value) else value


def main():
    out = dict(pagerank=PAGERANK, graphs={})
    for key in GRAPHS:
        A, directed, p = cases.GRAPHS[key]()
        graph = pg.AdjacencyWrapper(A, directed=directed)
        seeds = [int(v) for v in np.flatnonzero(p)]
        signal = pg.to_signal(graph, {v: 1.0 for v in seeds})
        ranks = pg.PageRank(**PAGERANK).rank(graph, signal)
        n = A.shape[0]
        bases = dict(seeds=signal.np, pagerank=ranks.np, pagerank_max=pg.Normalize("max").transform(ranks).np, zeros=np.zeros(n),
                     ones=np.ones(n))
        recorded = []
        for name, base, scale, kwargs in CONDUCTANCE:
            scores = pg.to_signal(graph, np.asarray(bases[base], dtype=np.float64) * scale)
            case = dict(name=name, measure="Conductance", base=base, scale=scale, kwargs=kwargs)
            try:
                case["value"] = encode(pg.Conductance(**kwargs).evaluate(scores))
            except Exception as e:
                case["raises"] = str(e)
            recorded.append(case)
        for name, base, scale in DENSITY:
            values = np.asarray(bases[base], dtype=np.float64) * scale
            # the GPU test compares the two routes on Density only where its denominator does not cancel
            assert float(np.sum(values ** 2)) <= 0.5 * float(np.sum(values)) ** 2, (key, name)
            case = dict(name=name, measure="Density", base=base, scale=scale, kwargs={})
            case["value"] = encode(pg.Density().evaluate(pg.to_signal(graph, values)))
            recorded.append(case)
        out["graphs"][key] = dict(directed=bool(directed), seeds=seeds, cases=recorded)
        for case in recorded:
            print(key, case["measure"], case["name"], case.get("value", "raises: " + case.get("raises", "")))
    out["best_direction"] = dict(Conductance=int(pg.Conductance().best_direction()), Density=int(pg.Density().best_direction()))
    print("best_direction", out["best_direction"])
    path = os.path.join(HERE, "golden_unsupervised.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
