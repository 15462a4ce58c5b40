"""Shared by the tests of the multi-group measures (host double and GPU) and by tests/golden/make_golden_multigroup.py: the seeded
group scores, a numpy / plain-Python restatement of what the reference's multigroup.py and Modularity compute (written apart from
pygrank_amd/multigroup.py: sets and dictionaries for the balls, np.unique for the tie groups), and the replay of the fixture.

The restatement, checked against the reference by the golden maker (AUC to pairs * 2^-52, Modularity to 1e-15 of its terms,
ClusteringCoefficient to 1e-14 relative or the rounding of the reference's own one-by-one sum):
  similarity   numerator = the LAST group's two scores multiplied (the reference assigns `dot = ui * vi`, it does not accumulate);
               "cos" divides by sqrt(l2u * l2v), l2 = the row's squares added in column order; a zero denominator gives 0
  sample       RandomState(seed): choice(n, max_positive) when n > max_positive (else every node once, no draw), then one
               choice(n, min(max_negative, n)) per candidate; duplicates stay
  pairs        per candidate v: label 1 for every other node of its hops-ball (successors), label 0 for every draw outside the ball
  AUC          two_wins / (2.0 * P * N), two_wins = sum over tie groups of positives * (2 * negatives below + negatives in the group)
"""
import json
import math
import os

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = 1e-6            # the project's parity bound for f32 storage against the f64 oracle (tests/unsupervised_common.py)
GROUPS = 3


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "golden_multigroup.json")) as f:
        return json.load(f)


def group_scores(n, groups=GROUPS, seed=0):
    """[n, groups] f64 scores that f32 holds exactly, in [0, 1): three in ten are exact zeros, row 1 is all zero, rows 3 and 4 are
    identical (ties and safe_div both occur)."""
    rng = np.random.default_rng(1000 + seed)
    S = rng.random((n, groups))
    S[rng.random((n, groups)) < 0.3] = 0.0
    S = S.astype(np.float32).astype(np.float64)
    if n > 1:
        S[1] = 0.0
    if n > 4:
        S[4] = S[3]
    assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
    return S


def pattern(A):
    """Successor lists of the non-zero pattern of A, and the pattern as 0/1 CSR."""
    A = sp.csr_array(A).copy()
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    return sp.csr_array((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)


def sample(n, max_positive, seed):
    state = np.random.RandomState(seed)
    candidates = state.choice(n, max_positive) if n > max_positive else np.arange(n)
    return np.asarray(candidates, dtype=np.int64), state


def pairs(A, hops, max_positive, max_negative, seed):
    """dict(first, second, label, candidates, draws): the pairs of LinkAssessment.evaluate in the reference's candidate order, positives
    (ascending id) before negatives (draw order) within a candidate."""
    P = pattern(A)
    n = P.shape[0]
    successors = [set(P.indices[P.indptr[v]:P.indptr[v + 1]].tolist()) for v in range(n)]
    candidates, state = sample(n, max_positive, seed)
    negatives = state.randint(0, n, size=(len(candidates), min(max_negative, n)))
    first, second, label = [], [], []
    for v, drawn in zip(candidates.tolist(), negatives.tolist()):
        ball, frontier = {v}, {v}
        for _ in range(hops):
            frontier = set().union(*[successors[u] for u in frontier]) - ball
            ball |= frontier
        for u in sorted(ball - {v}):
            first.append(v), second.append(u), label.append(1)
        for u in drawn:
            if u not in ball:
                first.append(v), second.append(u), label.append(0)
    return dict(first=np.array(first, dtype=np.int64), second=np.array(second, dtype=np.int64), label=np.array(label, dtype=np.uint8),
                candidates=candidates, draws=negatives)


def row_squares(S):
    l2 = np.zeros(len(S))
    for j in range(S.shape[1]):                  # column order: the reference's `l2u += ui * ui`
        l2 = l2 + S[:, j] * S[:, j]
    return l2


def predictions(S, first, second, similarity):
    S = np.asarray(S, dtype=np.float64)
    with np.errstate(all="ignore"):
        out = S[second, -1] * S[first, -1]
        if similarity == "cos":
            l2 = row_squares(S)
            den = np.sqrt(l2[second] * l2[first])
            quotient = out / den
            out = np.where(den == 0, 0.0, quotient)
    return out


def factors(S, similarity):
    S = np.asarray(S, dtype=np.float64)
    if similarity == "dot":
        return S[:, -1].copy()
    with np.errstate(all="ignore"):
        den = np.sqrt(row_squares(S))
        return np.where(den == 0, 0.0, S[:, -1] / den)


def two_wins(predicted, label):
    """(two_wins, P, N) in Python integers."""
    predicted = np.asarray(predicted, dtype=np.float64) + 0.0
    label = np.asarray(label) != 0
    values, inverse = np.unique(predicted, return_inverse=True)
    positives = np.bincount(inverse, weights=label, minlength=len(values)).astype(np.int64)
    negatives = np.bincount(inverse, weights=~label, minlength=len(values)).astype(np.int64)
    below = np.cumsum(negatives) - negatives
    return int(np.sum(positives * (2 * below + negatives))), int(positives.sum()), int(negatives.sum())


def auc(predicted, label):
    wins, P, N = two_wins(predicted, label)
    return wins / (2.0 * P * N)


def degrees_and_edges(A, directed):
    """networkx's graph.degree and number_of_edges() from the pattern."""
    P = pattern(A)
    out = np.diff(P.indptr)
    if directed:
        return out + np.bincount(P.indices, minlength=P.shape[0]), int(P.nnz)
    loops = P.diagonal()
    return out + loops, int((P.nnz + loops.sum()) // 2)


def modularity_terms(A, directed, scores, max_rank, max_positive, seed):
    """(w^T P w, (sum w d)^2 / 2m, m): Q = (first - second) / 2m."""
    P = pattern(A)
    n = P.shape[0]
    degree, m = degrees_and_edges(A, directed)
    if m == 0:
        return 0.0, 0.0, 0
    candidates, _ = sample(n, max_positive, seed)
    w = np.bincount(candidates, minlength=n) * np.asarray(scores, dtype=np.float64) / max_rank
    return float(w @ (P @ w)), float(np.dot(w, degree)) ** 2 / 2 / m, m


def modularity(A, directed, scores, max_rank, max_positive, seed):
    internal, expected, m = modularity_terms(A, directed, scores, max_rank, max_positive, seed)
    return 0 if m == 0 else (internal - expected) / 2 / m


def clustering(A, S, similarity, max_positive, seed):
    P = pattern(A)
    n = P.shape[0]
    candidates, _ = sample(n, max_positive, seed)
    c = np.bincount(candidates, minlength=n)
    y = P @ factors(S, similarity)
    closed = np.asarray((P @ P).multiply(P).sum(axis=1)).ravel()
    denominator = float(np.dot(c, closed))
    return 0 if denominator == 0 else float(np.dot(c * y, y)) / denominator


# ---- the fixture's inputs, rebuilt by the maker and by the tests alike ---------------------------------------------------------------
def truth_nodes(n, seed):
    """Per group: (known nodes, exclude nodes) of MultiSupervised."""
    rng = np.random.default_rng(2000 + seed)
    out = []
    for _ in range(GROUPS):
        known = sorted(int(v) for v in rng.choice(n, max(4, n // 10), replace=False))
        exclude = sorted(int(v) for v in rng.choice(n, n // 5, replace=False))
        out.append((known, exclude))
    return out


def close(got, want, bound=PARITY):
    if want == 0 or math.isinf(want):
        return got == want
    return abs(got - want) <= bound * abs(want)


class Inputs:
    """One fixture graph for a test module: the matrix, the engine's graph over it, the group scores as host array, signals and slab."""

    def __init__(self, pg, fx, key):
        import cases
        A, directed, _ = cases.GRAPHS[key]()
        record = fx["graphs"][key]
        assert bool(directed) == record["directed"]
        self.pg, self.key, self.record, self.A, self.directed = pg, key, record, A, bool(directed)
        self.n = A.shape[0]
        self.graph = pg.AdjacencyWrapper(A, directed=directed)
        self.S = group_scores(self.n, seed=record["scores_seed"])
        self.signals = {f"g{j}": pg.to_signal(self.graph, self.S[:, j].copy()) for j in range(GROUPS)}
        self.truths = truth_nodes(self.n, record["scores_seed"])

    def slab(self):
        return self.pg.DeviceMatrix.from_host(self.S)


def link_bound(case):
    """num_pairs * 2^-52: the counts are the reference's; sklearn's trapezoid sum rounds once per threshold at most."""
    return case["num_pairs"] * 2.0 ** -52


def replay_link(inputs, route, fused=True):
    """Every LinkAssessment case of the graph on `route`; returns the values."""
    import warnings
    pg, out = inputs.pg, []
    for case in inputs.record["link"]:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            measure = pg.LinkAssessment(inputs.graph, hops=case["hops"], similarity=case["similarity"], seed=case["seed"],
                                        max_positive_samples=case["max_positive"], max_negative_samples=case["max_negative"], fused=fused)
        got = measure.evaluate(inputs.signals)
        plan = measure.plan()
        print(f"{inputs.key}/link/{case['similarity']}/hops{case['hops']}/seed{case['seed']}: got {got!r} want {case['value']!r} "
              f"pairs {plan.num_pairs} bound {link_bound(case):.3e} route {measure.last_route}")
        assert measure.last_route == route
        assert plan.num_pairs == case["num_pairs"] and plan.num_positive == case["num_positive"]
        assert plan.candidates[:len(case["first_candidates"])].tolist() == case["first_candidates"]
        assert plan.second[plan.label == 0][:len(case["first_negatives"])].tolist() == case["first_negatives"]
        assert abs(got - case["value"]) <= link_bound(case), (inputs.key, case, got)
        out.append(got)
    return out


def replay_modularity(inputs, fused=True):
    pg, out = inputs.pg, []
    for case in inputs.record["modularity"]:
        measure = pg.Modularity(inputs.graph, max_rank=case["max_rank"], max_positive_samples=case["max_positive"], seed=case["seed"],
                                fused=fused)
        got = measure.evaluate(inputs.signals["g0"])
        internal, expected, m = case["internal"], case["expected"], case["edges"]
        print(f"{inputs.key}/modularity/rank{case['max_rank']}/samples{case['max_positive']}: got {got!r} want {case['value']!r} "
              f"terms {internal!r} {expected!r} route {measure.last_route}")
        # the value is a difference: the bound is relative to its two terms
        assert abs(got - case["value"]) <= PARITY * (internal + expected) / 2 / m, (inputs.key, case, got)
        out.append((measure, got))
    return out


def replay_clustering(inputs, route, fused=True):
    import warnings
    pg, out = inputs.pg, []
    for case in inputs.record["clustering"]:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            measure = pg.ClusteringCoefficient(inputs.graph, similarity=case["similarity"], max_positive_samples=case["max_positive"],
                                               seed=case["seed"], fused=fused)
        got = measure.evaluate(inputs.signals)
        print(f"{inputs.key}/clustering/{case['similarity']}: got {got!r} want {case['value']!r} route {measure.last_route}")
        assert measure.last_route == route
        assert close(got, case["value"]), (inputs.key, case, got)
        out.append(got)
    return out


SUPERVISED = ["AUC", "Cos", "NDCG"]
UNSUPERVISED = ["Conductance", "Density"]


def multi_supervised(inputs, name, excluded):
    pg = inputs.pg
    truth = {f"g{j}": pg.to_signal(inputs.graph, {v: 1.0 for v in inputs.truths[j][0]}) for j in range(GROUPS)}
    exclude = {f"g{j}": inputs.truths[j][1] for j in range(GROUPS)} if excluded else None
    return pg.MultiSupervised(getattr(pg, name), truth, exclude)


def replay_multi(inputs):
    pg = inputs.pg
    for case in inputs.record["multi"]:
        if case["kind"] == "supervised":
            measure = multi_supervised(inputs, case["measure"], case["excluded"])
        else:
            measure = pg.MultiUnsupervised(getattr(pg, case["measure"]), inputs.graph)
        got = measure.evaluate(inputs.signals)
        batched = measure.evaluate(inputs.signals, exact=False)
        print(f"{inputs.key}/multi/{case['measure']}/{case.get('excluded')}: got {got!r} batched {batched!r} want {case['value']!r}")
        assert close(got, case["value"]), (inputs.key, case, got)
        assert close(batched, got), (inputs.key, case, got, batched)
        assert close(measure.evaluate(inputs.slab(), exact=False), got)
