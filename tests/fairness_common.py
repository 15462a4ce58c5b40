"""Shared by the tests of the fairness postprocessors (host double and GPU): the fixture of tests/golden/make_golden_fairness.py, the
bounds its values are held to, and the checks both engines run."""
import json
import os

import numpy as np

import supervised_common as sc
from parity_common import REL_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = ["er10k", "rmat10_dir", "weighted300"]
DESCENTS = ["weighted300", "rmat10_dir"]       # the graphs with a recorded descent; the generator drops er10k's (see its docstring)
# The bounds are those the suite already has, no new constant:
#   RANKS     a column of a batch against its single-vector run (tests/test_gpu_batch_edges.py BOUND) and an engine run against the
#             reference's f64 result (tests/parity_common.py REL_TOL): 1e-6 relative L-inf
#   sc.TOL    a supervised measure against its recorded value (tests/supervised_common.py); the slab route against the columns route
#             is held to twice that (tests/test_gpu_supervised.py)
RANKS = REL_TOL


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "golden_fairness.json")) as f:
        return json.load(f)


class Case:
    """One fixture graph: graph, personalization and sensitive signals."""

    def __init__(self, pg, fx, key):
        import cases
        A, directed, _ = cases.GRAPHS[key]()
        self.record = fx["graphs"][key]
        assert bool(directed) == self.record["directed"]
        self.pg, self.key = pg, key
        self.graph = pg.AdjacencyWrapper(A, directed=directed)
        self.seeds = pg.to_signal(self.graph, {v: 1.0 for v in self.record["seeds"]})
        self.sensitive = pg.to_signal(self.graph, {v: 1.0 for v in self.record["sensitive"]})

    def personalizer(self, fx, **more):
        pg = self.pg
        return pg.FairPersonalizer(pg.PageRank(**fx["pagerank"]), verbose=False, **fx["fair"], **more)

    def open(self, personalizer):
        return personalizer._open(self.graph, self.seeds, self.sensitive, (), {})


def loss_bound(loss, params, measure_tol):
    """How far the loss of `params` may move when the ranks move by RANKS relative L-inf and each of the two measures by `measure_tol`
    relative.  With delta = RANKS * max |ranks|: Mabs is a mean of |original - ranks|, so it moves by at most delta; pRule is the
    ratio m1 / m2 of the two groups' mean scores, each of which moves by at most delta, so it moves by at most
    pRule * (delta / m1 + delta / m2) to first order.  The two weights scale the two terms.  Returns (bound, loss in numpy f64 from
    the engine's ranks)."""
    owner = loss.owner
    ranks = np.asarray(owner.ranker.rank(loss.graph, loss.edit(params)).np, dtype=np.float64)
    original = np.asarray(loss.original_ranks.np, dtype=np.float64)
    s = np.asarray(loss.sensitive.np, dtype=np.float64) != 0
    error = float(np.mean(np.abs(original - ranks)))
    m1, m2 = float(np.mean(ranks[s])), float(np.mean(ranks[~s]))
    fairness = min(m1, m2) / max(m1, m2)
    delta = RANKS * float(np.max(np.abs(ranks)))
    bound = owner.retain_rank_weight * (delta + measure_tol * error) \
        + owner.pRule_weight * fairness * (delta / m1 + delta / m2 + measure_tol)
    return bound, owner.retain_rank_weight * error - owner.pRule_weight * min(owner.target_pRule, fairness)


def first_steps(buckets, max_residual, partitions=10):
    """The candidate lists of the first coordinate step of every parameter (autotune.optimize: divide_range=2 halves the range before
    the step), each from the box centre."""
    hi = [1, 1, 5, 5] * buckets + [max_residual]
    lo = [0, 0, -5, -5] * buckets + [0]
    centre = [(a + b) / 2 for a, b in zip(lo, hi)]
    steps = []
    for variable in range(len(hi)):
        reach = (hi[variable] - lo[variable]) / 2 / 2
        step = []
        for part in range(partitions):
            w = list(centre)
            w[variable] = min(hi[variable], max(lo[variable], w[variable] + reach * (part * 2. / (partitions - 1) - 1)))
            step.append(w)
        steps.append(step)
    return steps


def check_points(case, fx):
    """The loss at the fixture's parameter vectors against the reference's recorded f64 value, through loss() and loss.many()."""
    worst = 0.0
    for buckets in (1, 2):
        for skew in (False, True):
            points = [p for p in case.record["points"] if p["buckets"] == buckets and p["skew"] == skew]
            loss = case.open(case.personalizer(fx, parameter_buckets=buckets, error_skewing=skew, max_residual=1))
            try:
                singles = [loss(p["params"]) for p in points]
                many = loss.many([p["params"] for p in points])
                for point, one, batched in zip(points, singles, many):
                    bound, _ = loss_bound(loss, point["params"], sc.TOL)
                    print(f"{case.key} buckets {buckets} skew {skew}: loss {one!r} many {batched!r} want {point['loss']!r} "
                          f"(bound {bound:.3e})")
                    worst = max(worst, abs(one - point["loss"]) / bound, abs(batched - point["loss"]) / bound)
                    assert abs(one - point["loss"]) <= bound, (case.key, point, one)
                    assert abs(batched - point["loss"]) <= bound, (case.key, point, batched)
            finally:
                loss.close()
    return worst


def check_descent(case, fx, personalizer):
    """The end-to-end condition: the final loss, re-evaluated through loss(), is at most the recorded starting loss minus HALF the
    reference's recorded improvement, and the ranks' pRule is above the recorded original pRule."""
    pg, descent = case.pg, case.record["descent"]
    assert descent is not None and descent["start_loss"] - descent["final_loss"] >= fx["min_improvement"]
    ranker = personalizer.ranker
    before = ranker.convergence
    ranks = personalizer.rank(case.graph, case.seeds, case.sensitive)
    assert ranker.convergence is before
    loss = case.open(personalizer)
    try:
        assert ranker.convergence.max_iters == descent["iterations"]
        final = loss(personalizer.last_params)
    finally:
        loss.close()
    fairness = pg.pRule(case.sensitive)(ranks)
    print(f"{case.key}: final loss {final!r} (reference start {descent['start_loss']!r}, final {descent['final_loss']!r}), pRule "
          f"{fairness!r} (original {descent['original_pRule']!r}, reference final {descent['final_pRule']!r}), {personalizer.last_fit}")
    assert final <= descent["start_loss"] - 0.5 * (descent["start_loss"] - descent["final_loss"])
    assert fairness > descent["original_pRule"]
    return ranks


def check_adhoc(case):
    """AdHocFairness("B"): the two groups' sums after the transform against the recorded ones, n * 2^-24 relative (an f32 sum of n
    terms), and the argument order of the constructor."""
    pg, want = case.pg, case.record["adhoc"]
    original = pg.PageRank(alpha=0.85, tol=1e-9, max_iters=1000).rank(case.graph, case.seeds)
    fair = pg.AdHocFairness("B").transform(original, sensitive=case.sensitive)
    values, s = np.asarray(fair.np, dtype=np.float64), np.asarray(case.sensitive.np, dtype=np.float64)
    tol = len(values) * 2.0 ** -24
    got = dict(sensitive_sum=float(np.sum(values * s)), other_sum=float(np.sum(values * (1 - s))))
    print(case.key, got, want)
    for name, value in got.items():
        assert abs(value - want[name]) <= tol * abs(want[name]), (case.key, name, value, want[name])
    assert pg.pRule(case.sensitive)(fair) > want["pRule_before"] or want["pRule_before"] == 1
