"""Shared by the tests of include/pgh_rank.h and of the rank-based measures: a numpy f64 restatement of the reference's NDCG and
SpearmanCorrelation (the stable order from np.lexsort, mid-ranks from tie-group counts, -0.0 canonicalised as Python compares it),
a thin driver of the engine's entries, the fixture and the bounds.

Bounds (derived, not measured):
  DCG, IDCG   a sum of at most T = min(k, relevant rows) non-negative f64 terms known / log2(pos + 2).  The positions are integers and
              must be exact; each term is within a few ulps (one division, one log2), and a sum of T non-negative terms in any order is
              within T ulps of the exact one: |got - want| <= max(T, 4) * 2^-50 * want.
              A one-position error is far larger: moving one relevant row from position p to p + 1 changes its term by
              known * (1 / log2(p + 2) - 1 / log2(p + 3)) ~ known / ((p + 2) ln 2 log2(p + 2)^2); at the largest size used here
              (p = 70 000, known = 0.25) that is 2e-8, while the bound at T = 8192 and DCG < 8192 / log2(3) is below 5e-9 (and for the
              shapes with a few hundred terms below 1e-12).
  rho         d_s, d_k are exact integers; the three sums have n' terms each, every product rounded once: absolute n' * 2^-50 (rho is at
              most 1 in magnitude, and the quotient of the sums inherits their relative error).
"""
import ctypes as C
import json
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, STREAMING, SORTED = 0, 1, 2
DECLINED = 2
MAX_RELEVANT = 8192


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "golden_ranking.json")) as f:
        return json.load(f)


def f32(values):
    """Rounded to f32 and back: what the engine stores."""
    return np.asarray(values, dtype=np.float32).astype(np.float64)


def canonical(values):
    """-0.0 becomes +0.0 (Python's sort compares them equal: a tie, in row order)."""
    return np.asarray(values, dtype=np.float64) + 0.0


def descending_order(values):
    """Row indices in descending order of value, ties in ascending row order."""
    values = canonical(values)
    return np.lexsort((np.arange(len(values)), -values))


def kept_rows(n, exclude):
    return np.ones(n, dtype=bool) if exclude is None else np.asarray(exclude) == 0


def discounted(known_in_order, k):
    top = known_in_order[:k]
    return math.fsum(top / np.log2(np.arange(len(top)) + 2.0)) if len(top) else 0.0


def dcg(scores, known, exclude, k):
    keep = kept_rows(len(known), exclude)
    s, kn = np.asarray(scores, dtype=np.float64)[keep], np.asarray(known, dtype=np.float64)[keep]
    if np.isnan(s).any() and (kn != 0).any():
        return float("nan")
    return discounted(kn[descending_order(s)], k)


def idcg(known, exclude, k):
    kn = np.asarray(known, dtype=np.float64)[kept_rows(len(known), exclude)]
    return discounted(kn[descending_order(kn)], k)


def centred_ranks(values):
    """2 midrank - (n + 1) from tie-group counts: a group of c values that follows `below` smaller ones has midrank below + (c + 1) / 2."""
    _, inverse, counts = np.unique(canonical(values), return_inverse=True, return_counts=True)
    below = np.cumsum(counts) - counts
    return (2 * below + counts + 1)[inverse.reshape(-1)].astype(np.float64) - (len(values) + 1)


def rho(scores, known, exclude):
    keep = kept_rows(len(known), exclude)
    s, kn = np.asarray(scores, dtype=np.float64)[keep], np.asarray(known, dtype=np.float64)[keep]
    if np.isnan(s).any():
        return float("nan")
    ds, dk = centred_ranks(s), centred_ranks(kn)
    below = math.sqrt(math.fsum(ds * ds) * math.fsum(dk * dk))
    return math.fsum(ds * dk) / below if below != 0 else float("nan")


def dcg_bound(want, terms):
    return max(terms, 4) * 2.0 ** -50 * abs(want)


def rho_bound(kept):
    return max(kept, 4) * 2.0 ** -50


def same(a, b):
    return a == b or (a != a and b != b)


def close(got, want, bound):
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got)
    return abs(got - want) <= bound


class Plan:
    def __init__(self, pg, known, exclude=None):
        from pygrank_amd import _lib as L
        self.L = L
        self.known = pg.DeviceVector.from_host(np.asarray(known, dtype=np.float64))
        self.exclude = None if exclude is None else pg.DeviceVector.from_host(np.asarray(exclude, dtype=np.float64))
        self.h = L.c_rank_plan()
        L.check(L.entry("pgh_rank_plan_create")(self.known._h, None if self.exclude is None else self.exclude._h, C.byref(self.h)))
        kept, relevant, negative = C.c_int64(), C.c_int64(), C.c_int32()
        L.check(L.entry("pgh_rank_plan_info")(self.h, C.byref(kept), C.byref(relevant), C.byref(negative)))
        self.kept, self.relevant, self.negative = kept.value, relevant.value, negative.value

    def __del__(self):
        try:
            self.L.entry("pgh_rank_plan_destroy")(self.h)
        except Exception:
            pass

    def ndcg(self, slab, k, route):
        """(status, [dcg per column], idcg) of a DeviceMatrix or, through the vector entry, a DeviceVector."""
        L = self.L
        width = getattr(slab, "b", 1)
        out, ideal = (C.c_double * width)(*([-7.0] * width)), C.c_double(-7.0)
        entry = L.entry("pgh_ndcg" if hasattr(slab, "b") else "pgh_ndcg_vec")
        status = entry(slab._h, self.h, int(k), route, out, C.byref(ideal))
        if status not in (0, DECLINED):
            L.check(status)
        return status, [float(v) for v in out], ideal.value

    def spearman(self, slab):
        L = self.L
        width = getattr(slab, "b", 1)
        out = (C.c_double * width)(*([-7.0] * width))
        status = L.entry("pgh_spearman" if hasattr(slab, "b") else "pgh_spearman_vec")(slab._h, self.h, out)
        L.check(status)
        return [float(v) for v in out]


def check_ndcg(pg, scores, known, exclude, ks, routes=(STREAMING, SORTED), label=""):
    """Both routes of pgh_ndcg on the [n, b] host array `scores` (f32 values) against the restatement, for every k of `ks`; each call is
    made twice and must return the same bits.  Returns the plan."""
    scores = np.asarray(scores, dtype=np.float64)
    n, b = scores.shape
    plan = Plan(pg, known, exclude)
    keep = kept_rows(n, exclude)
    assert plan.kept == int(keep.sum()) and plan.relevant == int((np.asarray(known)[keep] != 0).sum())
    slab = pg.DeviceMatrix.from_host(scores)
    kn = np.asarray(known, dtype=np.float64)[keep]
    in_order = []
    for j in range(b):
        s = scores[keep, j]
        in_order.append(None if np.isnan(s).any() and plan.relevant else kn[descending_order(s)])
    ideal_order = kn[descending_order(kn)]
    for k in ks:
        terms = min(k, plan.relevant)
        want = [float("nan") if o is None else discounted(o, k) for o in in_order]
        want_ideal = discounted(ideal_order, k)
        got = {}
        for route in routes:
            status, values, ideal = plan.ndcg(slab, k, route)
            assert status == 0, (label, n, b, k, route, status)
            again = plan.ndcg(slab, k, route)
            assert all(same(x, y) for x, y in zip(values, again[1])) and ideal == again[2], (label, n, b, k, route)
            assert close(ideal, want_ideal, dcg_bound(want_ideal, min(k, plan.kept))), (label, n, b, k, route, ideal, want_ideal)
            for j in range(b):
                assert close(values[j], want[j], dcg_bound(want[j], terms)), (label, n, b, k, route, j, values[j], want[j])
            got[route] = values
        first, second = got[routes[0]], got[routes[-1]]
        for x, y, w in zip(first, second, want):
            assert close(x, y, dcg_bound(w, terms)), (label, n, b, k, x, y)
    return plan


def check_spearman(pg, scores, known, exclude, label=""):
    scores = np.asarray(scores, dtype=np.float64)
    n, b = scores.shape
    plan = Plan(pg, known, exclude)
    slab = pg.DeviceMatrix.from_host(scores)
    got = plan.spearman(slab)
    assert all(same(x, y) for x, y in zip(got, plan.spearman(slab))), (label, n, b)
    for j in range(b):
        want = rho(scores[:, j], known, exclude)
        assert close(got[j], want, rho_bound(plan.kept)), (label, n, b, j, got[j], want)
    return got


# ---- the fixture of tests/golden/make_golden_ranking.py
GRAPHS = ["er10k", "rmat10_dir", "weighted300"]
KS = ["none", "1", "10", "relevant", "n"]
# NDCG on the columns route: the positions are exact (f32 ordinals hold integers up to 2^24), every term known / (log(ord + 1) / log 2)
# is formed in f32 -- one logarithm (2 ulps), the rounded constant, two divisions, the product with the 0 / 1 mask (exact): below 5 f32
# ulps relative -- and summed in f64.  A sum of non-negative terms is as close, relatively, as its worst term; DCG / IDCG doubles that:
# 10 * 2^-24, kept at the 16 * 2^-24 the other supervised measures are held to (supervised_common.TOL).  On the engine's routes the
# terms are f64 and the only difference left to the reference is the two PageRank bases, rebuilt here in f32.
NDCG_TOL = 16 * 2.0 ** -24
# The members of the recorded combinations (AUC, pRule, NDCG, Cos) lie in [0, 1] and are each within 16 * 2^-24 of the reference; AM is a
# weighted mean of them, Disparity and Parity a signed sum with sum |w| <= 3, the hinge has slope <= 1, and GM -- exp of a weighted mean
# of logarithms -- moves relatively as its members do (a member of 0 is lifted to epsilon on both sides): 4 * 16 * 2^-24 absolute.
COMBINATION_TOL = 64 * 2.0 ** -24


def spearman_tol(kept):
    """f64 throughout: the centred ranks are exact integers, three sums of n' rounded products."""
    return max(kept, 4) * 2.0 ** -50


class Ranking:
    """One fixture graph: supervised_common.Bases' five score bases with this fixture's node lists, and the two known vectors."""

    def __init__(self, pg, fx, key):
        import supervised_common as sc
        self.bases = sc.Bases(pg, dict(fx, graphs={key: fx["graphs"][key]}), key)
        self.pg, self.key, self.record = pg, key, fx["graphs"][key]
        self.graph, self.signals, self.exclude = self.bases.graph, self.bases.signals, self.bases.exclude
        n = len(self.graph)
        graded = np.zeros(n)
        for grade, nodes in self.record["graded"].items():
            graded[nodes] = float(grade)
        self.knowns = dict(binary=self.bases.known, graded=pg.to_signal(self.graph, graded))
        self.n = n
        self.kept = n - len(self.exclude)

    def k_of(self, label, known):
        relevant = len(self.record["known"])
        return dict(none=None, relevant=relevant, n=self.n).get(label) if label in ("none", "relevant", "n") else int(label)

    # The three tie-laden bases (seeds, zeros, ones) are the same f32 vectors on both sides and are held to the bounds above.  The two
    # PageRank bases are rebuilt here by an f32 run and agree with the reference's f64 run only to SCORE_TOL relative per entry (the
    # bound the suite holds every f32 result to), so two rows whose scores are closer than 2 * SCORE_TOL relative -- and not equal: rows
    # of equal score here went through the same arithmetic and are taken to be tied there too -- may stand in the other order in the
    # reference.  at_risk[i] counts such rows for row i: its position and its doubled rank may differ by at most that many.  The slack
    # a case is given is what those displacements can move the measure by, worked out from this run's own vectors:
    #   rho   |d N| <= sum 2 c_i |dk_i|,  |d S| <= E = sum (4 c_i |ds_i| + 4 c_i^2)  for N = sum ds dk, S = sum ds^2, K = sum dk^2, so
    #         |d rho| <= |d N| / sqrt((S - E) K) + |rho| (sqrt(S / (S - E)) - 1)
    #   NDCG  a relevant row at position p moves its term by at most known (1 / log2(p - c + 2) - 1 / log2(p + c + 2)), and a row within
    #         c of position k may enter or leave the sum with its whole term; the sum of those over IDCG (the same on both sides)
    SCORE_TOL = 16 * 2.0 ** -24

    def _kept(self, base, known_name, excluded):
        keep = np.ones(self.n, dtype=bool)
        if excluded:
            keep[self.exclude] = False
        scores = np.asarray(self.signals[base].np, dtype=np.float64)[keep]
        known = np.asarray(self.knowns[known_name].np, dtype=np.float64)[keep]
        return scores, known

    def _at_risk(self, scores):
        ordered = np.sort(scores)
        width = 2 * self.SCORE_TOL * np.abs(scores)
        near = np.searchsorted(ordered, scores + width, side="right") - np.searchsorted(ordered, scores - width, side="left")
        equal = np.searchsorted(ordered, scores, side="right") - np.searchsorted(ordered, scores, side="left")
        return (near - equal).astype(np.float64)

    def spearman_slack(self, base, known_name, excluded):
        if "pagerank" not in base:
            return 0.0
        scores, known = self._kept(base, known_name, excluded)
        c, ds, dk = self._at_risk(scores), centred_ranks(scores), centred_ranks(known)
        N, S, K = float(ds @ dk), float(ds @ ds), float(dk @ dk)
        dN, E = float(np.sum(2 * c * np.abs(dk))), float(np.sum(4 * c * np.abs(ds) + 4 * c * c))
        if S - E <= 0 or K == 0:
            return 2.0
        return dN / math.sqrt((S - E) * K) + abs(N) / math.sqrt(S * K) * (math.sqrt(S / (S - E)) - 1)

    def ndcg_slack(self, base, known_name, excluded, k):
        if "pagerank" not in base:
            return 0.0
        scores, known = self._kept(base, known_name, excluded)
        c = self._at_risk(scores)
        position = np.empty(len(scores))
        position[descending_order(scores)] = np.arange(len(scores))
        moved = (known != 0) & (c > 0)
        p, cm, kn = position[moved], c[moved], known[moved]
        shift = kn * (1 / np.log2(np.maximum(p - cm, 0) + 2) - 1 / np.log2(p + cm + 2))
        edge = np.where(np.abs(p - k) <= cm, kn / np.log2(np.maximum(p - cm, 0) + 2), 0.0)
        ideal = idcg(known, None, k)
        return float(np.sum(np.where(p - cm < k, shift, 0.0)) + np.sum(edge)) / ideal if ideal > 0 else 0.0

    def columns(self):
        import supervised_common as sc
        return [self.signals[base] for base in sc.BASES]

    def cases(self, **match):
        """The recorded cases that match, in the order of the score bases."""
        import supervised_common as sc
        found = {c["base"]: c for c in self.record["cases"] if all(c.get(k) == v for k, v in match.items())}
        return [found[base] for base in sc.BASES]


def combination(pg, name, pair, mode, known, exclude):
    """The same construction as tests/golden/make_golden_ranking.py:combination."""
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


def modes_of(fx, name, pair):
    return fx["modes"] + (["hinge"] if (name, pair) == ("AM", "auc_prule") else [])


def agrees(got, case, tol, absolute=False):
    """`got` against a recorded case: the same kind of non-finite value, else within `tol` (relative unless `absolute`)."""
    if "raises" in case:
        return False
    if "nonfinite" in case:
        kind = "nan" if math.isnan(got) else ("inf" if got == math.inf else ("-inf" if got == -math.inf else "finite"))
        return kind == case["nonfinite"]
    want = case["value"]
    return abs(got - want) <= (tol if absolute else tol * abs(want))


def check_fixture_measures(ranking, fx, route, excluded):
    """NDCG (every known vector and k) and SpearmanCorrelation over the five bases through evaluate_many against the fixture, on the
    route named; returns {(measure, known, k): values}."""
    pg = ranking.pg
    exclude = ranking.exclude if excluded else None
    out = {}
    for known_name, known in ranking.knowns.items():
        for label in KS:
            measure = pg.NDCG(known, exclude, k=ranking.k_of(label, known_name))
            got = measure.evaluate_many(ranking.columns())
            assert measure.last_route == route, (measure.last_route, route)
            for value, case in zip(got, ranking.cases(measure="NDCG", known=known_name, k=label, excluded=excluded)):
                print(f"{ranking.key}/NDCG/{known_name}/k={label}/{case['base']}/{excluded}: got {value!r} want {case}")
                slack = ranking.ndcg_slack(case["base"], known_name, excluded, measure.k)
                assert agrees(value, case, NDCG_TOL * abs(case.get("value", 0)) + slack, absolute=True), (ranking.key, case, value, slack)
            out["NDCG", known_name, label] = got
        measure = pg.SpearmanCorrelation(known, exclude)
        got = measure.evaluate_many(ranking.columns())
        assert measure.last_route == route
        kept = ranking.kept if excluded else ranking.n
        for value, case in zip(got, ranking.cases(measure="SpearmanCorrelation", known=known_name, excluded=excluded)):
            print(f"{ranking.key}/Spearman/{known_name}/{case['base']}/{excluded}: got {value!r} want {case}")
            slack = ranking.spearman_slack(case["base"], known_name, excluded)
            assert agrees(value, case, spearman_tol(kept) + slack, absolute=True), (ranking.key, case, value, slack)
        out["SpearmanCorrelation", known_name, None] = got
    return out


def check_fixture_combinations(ranking, fx, excluded, pairs=None):
    """Every recorded combination (of the member pairs named; default all) over the five bases: evaluate_many against the fixture and,
    to the bit, against evaluate; evaluate_many(exact=False) against the fixture."""
    pg = ranking.pg
    exclude = ranking.exclude if excluded else None
    columns = ranking.columns()
    for name in fx["combinations"]:
        for pair in (fx["pairs"] if pairs is None else pairs):
            for mode in modes_of(fx, name, pair):
                measure = combination(pg, name, pair, mode, ranking.knowns["binary"], exclude)
                many = measure.evaluate_many(columns)
                singles = [combination(pg, name, pair, mode, ranking.knowns["binary"], exclude).evaluate(column) for column in columns]
                for value, case in zip(many, ranking.cases(measure=name, pair=pair, mode=mode, excluded=excluded)):
                    print(f"{ranking.key}/{name}/{pair}/{mode}/{case['base']}/{excluded}: got {value!r} want {case}")
                    # the NDCG member's order slack on the PageRank bases enters with sum |w| <= 3
                    slack = 3 * ranking.ndcg_slack(case["base"], "binary", excluded, 10) if pair == "ndcg_cos" else 0.0
                    assert agrees(value, case, COMBINATION_TOL + slack, absolute=True), (ranking.key, case, value, slack)
                assert all(same(a, b) for a, b in zip(many, singles)), (ranking.key, name, pair, mode, many, singles)
                # exact=False: every active member in one pass; held to the fixture like the exact values, not to their bits
                fast = measure.evaluate_many(columns, exact=False)
                assert measure.last_batched == measure._active(), (name, pair, mode, measure.last_batched)
                for value, case in zip(fast, ranking.cases(measure=name, pair=pair, mode=mode, excluded=excluded)):
                    slack = 3 * ranking.ndcg_slack(case["base"], "binary", excluded, 10) if pair == "ndcg_cos" else 0.0
                    assert agrees(value, case, COMBINATION_TOL + slack, absolute=True), (ranking.key, case, value, slack)
