"""Shared by the tests of the unsupervised measures (host double and GPU): the fixture of tests/golden/make_golden_unsupervised.py
and the replay of its cases."""
import json
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = 1e-6            # the project's parity bound for f32 storage against the f64 oracle (relative)


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "golden_unsupervised.json")) as f:
        return json.load(f)


def decode(value):
    return float("inf") if value == "inf" else float(value)


class Bases:
    """The score vectors of one fixture graph, built once: seeds, pagerank, pagerank_max, zeros, ones (as graph signals)."""

    def __init__(self, pg, fx, key):
        import cases
        A, directed, _ = cases.GRAPHS[key]()
        record = fx["graphs"][key]
        assert bool(directed) == record["directed"]
        self.pg, self.key, self.record = pg, key, record
        self.graph = pg.AdjacencyWrapper(A, directed=directed)
        n = A.shape[0]
        seeds = pg.to_signal(self.graph, {v: 1.0 for v in record["seeds"]})
        ranks = pg.PageRank(**fx["pagerank"]).rank(self.graph, seeds)
        self.signals = dict(seeds=seeds, pagerank=ranks, pagerank_max=pg.Normalize("max").transform(ranks),
                            zeros=pg.to_signal(self.graph, np.zeros(n)), ones=pg.to_signal(self.graph, np.ones(n)))

    def scores(self, case):
        base = self.signals[case["base"]]
        return base if case["scale"] == 1 else base * case["scale"]

    def measure(self, case, graph=None):
        return getattr(self.pg, case["measure"])(graph, **case["kwargs"])


def close(got, want, bound=PARITY):
    if math.isinf(want) or want == 0:
        return got == want
    return abs(got - want) <= bound * abs(want)


def replay(bases, graph_at_construction=False):
    """Every case of the graph: the value within PARITY of the reference's (inf and 0 exactly), or the reference's exception.  Returns
    the values (None where the case raises)."""
    out = []
    for case in bases.record["cases"]:
        measure = bases.measure(case, bases.graph if graph_at_construction else None)
        scores = bases.scores(case)
        if "raises" in case:
            try:
                measure.evaluate(scores)
            except Exception as e:
                assert str(e) == case["raises"], (bases.key, case["name"], str(e))
                out.append(None)
                continue
            raise AssertionError(f"{bases.key}/{case['measure']}/{case['name']}: the reference raises, evaluate returned")
        got = measure.evaluate(scores)
        want = decode(case["value"])
        print(f"{bases.key}/{case['measure']}/{case['name']}: got {got!r} want {want!r}")
        assert close(got, want), (bases.key, case["measure"], case["name"], got, want)
        out.append(got)
    return out
