"""DEV-CONTAINER-ONLY: fixtures of Subgraph, Supergraph, MabsMaintain, SeparateNormalization and Sequential (tests/test_subgraph_host.py,
tests/test_gpu_subgraph.py) from the reference, imported read-only with the `wget` shim of SURVEY.md 8c under its numpy backend.
Output: tests/golden/golden_subgraph.npz.

Per graph of tests/subgraph_common.py (networkx graphs from cases.GRAPHS rmat10_dir and weighted300, directed and as max(A, A^T)), with the
graph's personalization, the chains of subgraph_common.build:
  <graph>/top_k<k>/nodes                    PageRank(0.85) >> Top(k), k in (8, 100): the nodes with a non-zero score
  <graph>/sub_k<k>/nodes, /ranks            ... >> Subgraph(): the subgraph's nodes, ascending, and their scores
  <graph>/super_k<k>/ranks, /iterations     ... >> PageRank(0.9, tol=1e-6, error_type=L1) >> Supergraph(): the scores on the whole graph and
                                            the iterations of the inner run
  <graph>/noedge/ranks, /iterations         Subgraph() >> PageRank(...) >> Supergraph() on six nodes no two of which share an edge
  <graph>/mabs/ranks                        MabsMaintain(PageRank(0.85))
  <graph>/sep_binary/ranks, /sep_fraction/ranks   SeparateNormalization(separator, PageRank(0.85))
  <graph>/sequential/ranks                  Sequential(PageRank(0.85), Normalize(), Top(3))

Every case is ASSERTED (a case that misses a condition is left out and reported, never loosened):
  * where a Top(k) selects, the k-th and the (k + 1)-th score lie at least a relative FLOOR_MARGIN = 5e-5 apart (the bar of
    make_golden_oversampling.py): an f32 engine then selects the same nodes;
  * no stopping test of an inner PageRank run sees a residual within RESIDUAL_SIGMAS = 6 sigma of its tolerance, sigma being the f32
    rounding noise of an L1 residual as make_golden_oversampling.py derives it: the engine then stops on the same iteration.

Run:  PYGRANK_REFERENCE=<checkout of the reference> python tests/golden/make_golden_subgraph.py
"""
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
os.environ["pygrankBackend"] = "numpy"
os.environ["HOME"] = tempfile.mkdtemp(prefix="pgh_golden_home_")   # import writes ~/.pygrank/config.json
sys.dont_write_bytecode = True
sys.modules["wget"] = types.ModuleType("wget")                      # pygrank/benchmarks/download.py:3
sys.path.insert(0, os.environ["PYGRANK_REFERENCE"])

import numpy as np  # noqa: E402
import pygrank as pg  # noqa: E402

import subgraph_common as sc  # noqa: E402

FLOOR_MARGIN, RESIDUAL_SIGMAS, TOL = 5e-5, 6.0, 1e-6


class Missed(Exception):
    """A case misses one of the conditions: it is left out."""


class Recorder:
    """An error type that is the reference's L1 and remembers every stopping test: (residual, the iterate it was taken on)."""

    def __init__(self):
        self.tests = []

    def __call__(self, previous):
        measure = pg.L1(previous)

        def evaluate(ranks):
            value = float(measure(ranks))
            self.tests.append((value, np.asarray(ranks, dtype=np.float64).copy()))
            return value
        return evaluate


def check_gap(scores, k, what):
    order = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
    if k < len(order) and not order[k - 1] - order[k] >= FLOOR_MARGIN * abs(order[k - 1]):
        raise Missed(f"{what}: the scores in places {k} and {k + 1} lie {(order[k - 1] - order[k]) / abs(order[k - 1]):.2e} apart")


def check_residuals(recorder, what):
    assert recorder.tests, what
    for residual, x in recorder.tests:
        sigma = 2.0 ** -23 * float(np.sqrt((x * x).sum() / 3.0))
        if abs(residual - TOL) < RESIDUAL_SIGMAS * sigma:
            raise Missed(f"{what}: a stopping test sees {residual:.6e}, {abs(residual - TOL) / sigma:.1f} sigma from the tolerance")


def main():
    out, missed = {}, []
    for key in sc.GRAPHS:
        G, personalization = sc.nx_graph(key)
        A, _, _ = sc.adjacency(key)
        n = A.shape[0]
        base = sc.dense(sc.first_ranker(pg)(G, pg.to_signal(G, personalization)), n)
        for name, k in sc.CHAINS:
            stem = sc.stem(key, name, k)
            try:
                if k is not None:
                    check_gap(base, k, stem)
                if name == "sequential":
                    check_gap(base, 3, stem)
                recorder = Recorder()
                wants_inner = name in ("super", "noedge")
                signal, inner = sc.run(pg, G, personalization, A, name, k, sc.inner_ranker(pg, recorder) if wants_inner else None)
                if wants_inner:
                    check_residuals(recorder, stem)
                    out[stem + "/iterations"] = np.int64(inner.convergence.iteration)
                if name == "top":
                    out[stem + "/nodes"] = np.flatnonzero(sc.dense(signal, n)).astype(np.int64)
                    assert len(out[stem + "/nodes"]) == k, stem
                elif name == "sub":
                    nodes = [int(node) for node in signal]
                    assert len(set(nodes)) == k and signal.graph.number_of_nodes() == k, stem
                    nodes = sorted(nodes)                                   # (a networkx view lists its nodes in set order)
                    out[stem + "/nodes"] = np.asarray(nodes, dtype=np.int64)
                    out[stem + "/ranks"] = np.asarray([float(signal[node]) for node in nodes])
                else:
                    out[stem + "/ranks"] = sc.dense(signal, n)
                if name == "noedge":
                    assert signal.graph is G and G.subgraph(list(sc.independent_scores(A))).number_of_edges() == 0, stem
                print(f"{stem}: ok" + (f", {int(inner.convergence.iteration)} inner iterations" if wants_inner else ""))
            except Missed as why:
                missed.append(str(why))
                print("LEFT OUT", why)
    np.savez_compressed(os.path.join(HERE, "golden_subgraph.npz"), **out)
    print(f"{len(out)} arrays, {len(missed)} cases left out")


if __name__ == "__main__":
    main()
