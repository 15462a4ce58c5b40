"""Shared by the tests of the supervised measures (host double and GPU): the fixture of tests/golden/make_golden_supervised.py, the
bound its values are held to, and the replay of its cases."""
import json
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Inputs are stored as f32, and for the recorded cases every measure is a ratio or a sum of same-signed f64 sums: 16 roundings of f32.
TOL = 16 * 2.0 ** -24
# The three measures that subtract sums of like size get that bound divided by the conditioning floor the generator asserts.
CANCELLING = dict(KLDivergence="KL", MKLDivergence="KL", PearsonCorrelation="Pearson", TNR="TNR")
NEW = ["Accuracy", "TPR", "TNR", "PPV", "pRule", "L2Disparity", "BinaryCrossEntropy", "CrossEntropy", "KLDivergence", "MKLDivergence",
       "PearsonCorrelation", "MannWhitneyParity"]
EXISTING = ["MaxDifference", "Mabs", "L1", "RMabs", "MSQ", "MSQRT", "L2", "Euclidean", "Cos", "Dot", "AUC"]
BASES = ["seeds", "pagerank", "pagerank_max", "zeros", "ones"]


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "golden_supervised.json")) as f:
        return json.load(f)


def bound(fx, measure):
    floor = CANCELLING.get(measure)
    return TOL if floor is None else TOL / fx["floors"][floor]


class Bases:
    """One fixture graph, built once: the five score bases, the known scores and the exclude list (graph signals and a node list)."""

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
        # pagerank_max as the reference's Normalize("max") has it: x / max x, so the largest entry is exactly 1 (BinaryCrossEntropy's
        # log(1 - s + eps) moves by log 1.5 between 1 and 1 - 2^-24, what a product with the stored reciprocal may return there)
        stored = np.asarray(ranks.np, dtype=np.float64)
        self.signals = dict(seeds=seeds, pagerank=ranks, pagerank_max=pg.to_signal(self.graph, stored / stored.max()),
                            zeros=pg.to_signal(self.graph, np.zeros(n)), ones=pg.to_signal(self.graph, np.ones(n)))
        self.known = pg.to_signal(self.graph, {v: 1.0 for v in record["known"]})
        self.exclude = list(record["exclude"])

    def measure(self, name, excluded):
        return getattr(self.pg, name)(self.known, self.exclude if excluded else None)

    def cases(self, name, excluded):
        """The recorded cases of one measure, in the order of BASES."""
        found = {c["base"]: c for c in self.record["cases"] if c["measure"] == name and c["excluded"] == excluded}
        return [found[base] for base in BASES]


def agrees(got, case, tol):
    """`got` against a recorded case: the same kind of non-finite value, 0 exactly, else within `tol` relative.  A case where the
    reference raised is never met by a value."""
    if "raises" in case:
        return False
    if "nonfinite" in case:
        kind = "nan" if math.isnan(got) else ("inf" if got == math.inf else ("-inf" if got == -math.inf else "finite"))
        return kind == case["nonfinite"]
    want = case["value"]
    if want == 0:
        return got == 0
    return abs(got - want) <= tol * abs(want)


def same(a, b):
    """Equal floats, nan equal to nan."""
    return a == b or (a != a and b != b)


def check_many(bases, fx, name, excluded, route, values=None):
    """evaluate_many over the five bases of one measure against the fixture, on the route named; returns the values."""
    measure = bases.measure(name, excluded)
    got = measure.evaluate_many([bases.signals[base] for base in BASES]) if values is None else values
    assert isinstance(got, list) and len(got) == len(BASES)
    if values is None:
        assert measure.last_route == route, (name, measure.last_route)
    tol = bound(fx, name)
    for value, case in zip(got, bases.cases(name, excluded)):
        print(f"{bases.key}/{name}/{case['base']}/{'excluded' if excluded else 'all'}: got {value!r} want "
              f"{case.get('value', case.get('nonfinite'))!r} (bound {tol:.3e})")
        assert agrees(value, case, tol), (bases.key, name, case, value)
    return got
