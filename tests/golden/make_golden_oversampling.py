"""DEV-CONTAINER-ONLY: fixtures of the seed oversampling postprocessors (tests/test_oversampling_host.py, tests/test_gpu_oversampling.py)
from the reference, imported read-only with the `wget` shim of SURVEY.md 8c under its numpy backend.
Output: tests/golden/golden_oversampling.npz.

Per graph of cases.GRAPHS (er10k, rmat12_sym, rmat10_dir, weighted300), with the support of the graph's personalization as ones, around
PageRank(alpha=0.9, error_type=L1, tol=1e-6, max_iters=1000):
  <graph>/so_<method>/ranks, /seeds                       SeedOversampling("safe" | "top" | "neighbors"): the reference's f64 rank
                                                          vector and the size of the grown seed set
  <graph>/so_<method>/nodes                               the seed set, where the graph's own misses a condition below (absent: the
                                                          graph's own seeds): the first of eight others of the same size that holds
  <graph>/bso_<objective>_<source>/ranks, /rounds,        BoostedSeedOversampling(partial, previous) and (naive, original): the rank
                                   /seeds, /weights       vector, the number of rounds, every round's seed count and weight a_N
  <graph>/bso_<objective>_<source>/nodes                  the seed set, where the graph's own misses a condition below (absent: the
                                                          graph's own seeds): the first of eight others of the same size that holds
  rmat10_dir/bso_partial_previous/*_tol1e-9               that case around PageRank(tol=1e-9), the engine's f64 loops (its own /nodes_tol1e-9)
  <MULTI graph>/multi/seeds0..2, /ranks, /rounds          three seed sets whose boosted runs (partial, previous) take different numbers
                                                          of rounds: the propagate case
  <stem>/emulation_rel_linf                               only where the f32 emulation below misses the bar: its own rel-Linf (the
                                                          tests then allow 4x that)

The reference's graph here is its AdjacencyWrapper with the three methods its SeedOversampling asks a graph for (nodes, neighbors,
number_of_edges: the stored entries of a directed graph, every edge once -- (nnz + nnz of the diagonal) / 2 -- of an undirected one).

Every case is ASSERTED (a case that misses a condition is left out and reported, never loosened):
  * a numpy emulation of the engine's route -- f32 storage, f64 sums (`Emulation`) -- selects the same seed set on every round, stops on
    the same round, and stays within rel-Linf 1e-6 of the reference's vector;
  * no rank other than the minimiser lies within relative 5e-5 of a round's floor;
  * | |a_N - previous a_N| - 0.001 | >= 1e-5 on every round;
  * no stopping test of an inner PageRank run sees a residual within six sigma of its tolerance (RESIDUAL_SIGMAS below).

Run:  PYGRANK_REFERENCE=<checkout of the reference> python tests/golden/make_golden_oversampling.py
"""
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
import scipy.sparse as sp  # noqa: E402
import pygrank as pg  # noqa: E402

import cases  # noqa: E402
from oracle import ref_loops as orc  # noqa: E402
from oracle import rmat_np  # noqa: E402

ALPHA, TOL, MAX_ITERS = 0.9, 1e-6, 1000
GRAPHS = ["er10k", "rmat12_sym", "rmat10_dir", "weighted300"]
METHODS = ["safe", "top", "neighbors"]
BOOSTED = [("partial", "previous"), ("naive", "original")]
TIGHT = ("rmat10_dir", "partial", "previous", 1e-9)
MULTI = "rmat10_dir"
BAR, FLOOR_MARGIN, STEP_MARGIN, WEIGHT_TOL = 1e-6, 5e-5, 1e-5, 0.001
# The inner PageRank stops on an L1 residual sum |x' - x| of iterates that sum to 1.  Stored in f32, an entry x_i carries a rounding error
# of at most half an ulp, ulp_i <= 2^-23 x_i: uniform, variance ulp_i^2 / 12.  The engine rounds an iterate twice (the unnormalised
# product, then the scaled iterate) and a residual term holds two iterates: variance ulp_i^2 / 3 per term, so the residual of a run
# carries noise of sigma = 2^-23 sqrt(sum x_i^2 / 3) -- 0.1% to 1% of the tolerance 1e-6 on these graphs.  A run one of whose stopping
# tests sees a residual within RESIDUAL_SIGMAS sigma of the tolerance could stop one iteration apart on the engine, a step that moves
# the ranks by the tolerance times the personalization's norm, far above the bar: it is no case.
RESIDUAL_SIGMAS = 6.0


class Missed(Exception):
    """A case misses one of the conditions: it is left out."""


class Graph(pg.AdjacencyWrapper):
    def nodes(self):
        return range(self.num_nodes)

    def number_of_nodes(self):
        return self.num_nodes

    def neighbors(self, u):
        A = self.adj
        return A.indices[A.indptr[u]:A.indptr[u + 1]]

    def number_of_edges(self):
        if self.directed:
            return self.adj.nnz
        return (self.adj.nnz + int(np.count_nonzero(self.adj.diagonal()))) / 2


def ranker(tol=TOL):
    return pg.PageRank(alpha=ALPHA, error_type=pg.L1, tol=tol, max_iters=MAX_ITERS)


def reference_rank(graph, values, tol=TOL):
    nodes = np.flatnonzero(values)
    return np.asarray(ranker(tol).rank(graph, {int(v): float(values[v]) for v in nodes}).np, dtype=np.float64)


f32 = lambda v: np.asarray(v, dtype=np.float32)                      # noqa: E731
f64 = lambda v: np.asarray(v, dtype=np.float64)                      # noqa: E731


class Emulation:
    """The engine's route in numpy: every vector rounded to f32 where the engine stores it, every sum in f64.  Below fp32 eps the engine
    runs its f64 loops: nothing is rounded then."""

    def __init__(self, A, directed, tol=TOL):
        self.MT = sp.csr_array(orc.normalize(A, "auto", directed)).T.tocsr()
        single = tol >= float(np.finfo(np.float32).eps)
        self.tol = tol
        self.store = (lambda v: f64(f32(v))) if single else f64
        self.ulp = 2.0 ** -23 if single else 2.0 ** -52
        self.closest = np.inf       # over every stopping test of every run: | residual - tol | in sigmas of the f32 noise

    def rank(self, values):
        values = self.store(values)
        norm = float(np.abs(values).sum())
        p = self.store(values / norm)
        x, previous, calls = p.copy(), None, 0
        while True:
            calls += 1
            assert calls < MAX_ITERS
            if previous is not None:
                residual = float(np.abs(x - previous).sum())
                sigma = self.ulp * float(np.sqrt((x * x).sum() / 3.0))
                self.closest = min(self.closest, abs(residual - self.tol) / sigma)
                if residual <= self.tol:
                    break
            previous = x
            y = ALPHA * (self.MT @ x) + (1 - ALPHA) * p
            x = self.store(y / float(y.sum()))
        return self.store(x * norm)

    @staticmethod
    def floor(ranks, seeds):
        return float(ranks[seeds == 1.0].min())

    @staticmethod
    def forms(s, R, RN):
        return float((s * R * R).sum()), float((R * R).sum()), float((s * RN * R).sum())


def weight(objective, S1, S2, S3):
    return S1 / S2 - S3 / S2 if objective == "partial" else 0.5 - 0.5 * S3 / S2


def floor_is_clear(ranks, floor):
    """No rank other than the minimiser (and its exact ties) within relative FLOOR_MARGIN of the floor."""
    gap = np.abs(ranks - floor)
    return bool(np.all((gap == 0) | (gap > FLOOR_MARGIN * abs(floor))))


def rel_linf(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def closing(stem, got, want, out):
    worst = rel_linf(got, want)
    if worst > BAR:
        print("   ", stem, "emulation misses the bar:", worst, "(recorded)")
        out[stem + "/emulation_rel_linf"] = np.float64(worst)
    return worst


def seed_oversampling(key, A, directed, p, method, out):
    graph = Graph(A, directed=directed)
    n = A.shape[0]
    stem = f"{key}/so_{method}"
    want = np.asarray(pg.SeedOversampling(ranker(), method).rank(graph, {int(v): 1.0 for v in np.flatnonzero(p)}).np, dtype=np.float64)
    em = Emulation(A, directed)
    if method == "neighbors":
        grown = p.copy()
        grown[(A.T @ p) > 0] = 1.0
        grown_em = grown
    else:
        first, first_em = reference_rank(graph, p), em.rank(p)
        if method == "safe":
            floor, floor_em = Emulation.floor(first, p), Emulation.floor(first_em, p)
            keep = np.zeros(n, dtype=bool)
        else:
            top = int(n * n / graph.number_of_edges())
            assert 1 <= top <= n
            floor, floor_em = np.sort(first)[n - top], np.sort(first_em)[n - top]
            keep = p == 1.0
        if not floor_is_clear(first, floor):
            raise Missed(f"{stem}: a rank within {FLOOR_MARGIN} of the floor")
        grown, grown_em = ((first >= floor) | keep).astype(np.float64), ((first_em >= floor_em) | keep).astype(np.float64)
    assert np.array_equal(reference_rank(graph, grown), want), stem      # this is what the reference's class did
    if not np.array_equal(grown, grown_em):
        raise Missed(f"{stem}: the emulation selects other seeds")
    got = em.rank(grown_em)
    if em.closest < RESIDUAL_SIGMAS:
        raise Missed(f"{stem}: an inner run's residual within {em.closest:.2f} sigma of its tolerance")
    worst = closing(stem, got, want, out)
    out[stem + "/ranks"], out[stem + "/seeds"] = want, np.int64(grown.sum())
    print(stem, "seeds", int(grown.sum()), "| f32 emulation: rel-Linf", worst)


def boosted(graph, A, directed, p, objective, source, tol=TOL):
    """(reference ranks, rounds, seed counts, weights, emulation rel-Linf); raises Missed when a condition fails."""
    algo = pg.BoostedSeedOversampling(ranker(tol), objective, source)
    want = np.asarray(algo.rank(graph, {int(v): 1.0 for v in np.flatnonzero(p)}).np, dtype=np.float64)
    rounds = int(algo._weight_convergence.iteration) - 1
    em = Emulation(A, directed, tol)
    RN, RN_em = reference_rank(graph, p, tol), em.rank(p)
    mask = mask_em = p
    counts, weights, last, last_em = [], [], 1.0, 1.0
    for k in range(rounds):
        floor, floor_em = Emulation.floor(RN, mask), Emulation.floor(RN_em, mask_em)
        if not floor_is_clear(RN, floor):
            raise Missed(f"round {k}: a rank within {FLOOR_MARGIN} of the floor")
        s, s_em = (RN >= floor).astype(np.float64), (RN_em >= floor_em).astype(np.float64)
        if not np.array_equal(s, s_em):
            raise Missed(f"round {k}: the emulation selects other seeds")
        R, R_em = reference_rank(graph, s, tol), em.rank(s_em)
        a, a_em = weight(objective, *Emulation.forms(s, R, RN)), weight(objective, *Emulation.forms(s_em, R_em, RN_em))
        RN, RN_em = RN + a * R, em.store(RN_em + a_em * R_em)
        if source == "previous":
            mask, mask_em = s, s_em
        for step in (abs(a - last), abs(a_em - last_em)):
            if abs(step - WEIGHT_TOL) < STEP_MARGIN:
                raise Missed(f"round {k}: a weight step of {step}, within {STEP_MARGIN} of the tolerance")
        stop, stop_em = abs(a - last) <= WEIGHT_TOL, abs(a_em - last_em) <= WEIGHT_TOL
        if stop != (k == rounds - 1) or stop_em != stop:
            raise Missed(f"round {k}: the loops stop apart ({stop}, {stop_em}, {rounds} rounds)")
        counts.append(int(s.sum()))
        weights.append((a, a_em))
        last, last_em = a, a_em
    assert rel_linf(RN, want) <= 1e-12, rel_linf(RN, want)              # the restated loop is the reference's class
    if em.closest < RESIDUAL_SIGMAS:
        raise Missed(f"an inner run's residual within {em.closest:.2f} sigma of its tolerance")
    return want, rounds, counts, [w for w, _ in weights], RN_em


def seed_options(A, p):
    """The graph's own seeds, then eight other seed sets of the same size: (note, nodes or None, personalization)."""
    yield "", None, p
    for other in range(1, 9):
        nodes = np.sort(rmat_np.seed_nodes(A, int(p.sum()), seed=100 + other))
        q = np.zeros_like(p)
        q[nodes] = 1.0
        yield f" (seed set {other})", nodes, q


def boosted_case(key, A, directed, p, graph, objective, source, tol, out, left_out):
    """Records one boosted case on the first seed set that meets the conditions; returns whether there is one."""
    stem, tag = f"{key}/bso_{objective}_{source}", "" if tol == TOL else "_tol1e-9"
    for note, nodes, q in seed_options(A, p):
        try:
            want, rounds, counts, weights, got = boosted(graph, A, directed, q, objective, source, tol)
        except Missed as why:
            left_out.append(f"{stem}{tag}{note}: {why}")
            continue
        if tol == TOL:
            worst = closing(stem, got, want, out)
        else:
            worst = rel_linf(got, want)
            out[stem + "/emulation_rel_linf" + tag] = np.float64(worst)
        if nodes is not None:
            out[stem + "/nodes" + tag] = nodes.astype(np.int32)
        out[stem + "/ranks" + tag], out[stem + "/rounds" + tag] = want, np.int64(rounds)
        out[stem + "/seeds" + tag], out[stem + "/weights" + tag] = np.array(counts, dtype=np.int64), np.array(weights)
        print(stem + tag + note, "rounds", rounds, "seeds", counts, "weights", np.round(weights, 5), "| emulation: rel-Linf", worst)
        return True
    return False


def main():
    warnings.simplefilter("ignore")
    out, left_out = {}, []
    for key in GRAPHS:
        A, directed, p = cases.GRAPHS[key]()
        A = sp.csr_array(A)
        p = (np.asarray(p) != 0).astype(np.float64)
        graph = Graph(A, directed=directed)
        for method in METHODS:
            for note, nodes, q in seed_options(A, p):
                try:
                    seed_oversampling(key, A, directed, q, method, out)
                except Missed as why:
                    left_out.append(f"{why}{note}")
                    continue
                if nodes is not None:
                    out[f"{key}/so_{method}/nodes"] = nodes.astype(np.int32)
                break
            else:
                raise AssertionError((key, method))
        for objective, source in BOOSTED:
            assert boosted_case(key, A, directed, p, graph, objective, source, TOL, out, left_out), (key, objective, source)
            if (key, objective, source) == TIGHT[:3]:
                assert boosted_case(key, A, directed, p, graph, objective, source, TIGHT[3], out, left_out), TIGHT
    # the propagate case: three seed sets of MULTI whose runs take different numbers of rounds
    A, directed, _ = cases.GRAPHS[MULTI]()
    A = sp.csr_array(A)
    graph = Graph(A, directed=directed)
    n = A.shape[0]
    rng = np.random.default_rng(64)
    degrees = np.asarray(A.sum(axis=1)).ravel() + np.asarray(A.sum(axis=0)).ravel()
    chosen = {}
    for attempt in range(200):
        if len(chosen) == 3:
            break
        members = np.sort(rng.choice(np.flatnonzero(degrees > 0), int(rng.integers(3, 25)), replace=False))
        p = np.zeros(n)
        p[members] = 1.0
        try:
            want, rounds, counts, weights, got = boosted(graph, A, directed, p, "partial", "previous")
        except (Missed, ZeroDivisionError, Exception) as why:      # noqa: B014
            print("    multi candidate", attempt, "left out:", why)
            continue
        if rounds not in chosen and rel_linf(got, want) <= BAR:
            chosen[rounds] = (members, want)
            print(f"{MULTI}/multi candidate {attempt}: rounds {rounds} seeds {counts}")
    assert len(chosen) == 3, chosen.keys()
    order = sorted(chosen, reverse=True)                            # the longest run first: the batch narrows from its last column
    for j, rounds in enumerate(order):
        out[f"{MULTI}/multi/seeds{j}"] = chosen[rounds][0].astype(np.int32)
    out[f"{MULTI}/multi/ranks"] = np.stack([chosen[r][1] for r in order], axis=1)
    out[f"{MULTI}/multi/rounds"] = np.array(order, dtype=np.int64)
    for line in left_out:
        print("LEFT OUT", line)
    path = os.path.join(HERE, "golden_oversampling.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
