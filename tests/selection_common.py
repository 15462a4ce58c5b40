"""Shared by the tests of AlgorithmSelection (host double and GPU) and by tests/golden/make_golden_selection.py: the planted graph, the
candidate family and the fixture."""
import json
import os

import numpy as np
import scipy.sparse as sp

from parity_common import rel_linf, tolerance_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED = dict(blocks=3, block_size=200, p_in=0.06, p_out=0.004, seed=7, seeds_every=3)
FAMILY = dict(tol=1e-6, max_iters=10000)
# fraction_of_training settings: one split, two splits, three splits
FRACTIONS = [0.9, [0.8, 0.6], [0.9, 0.8, 0.6]]
MEASURES = ["AUC", "TPR"]
# The GPU supervised tests (tests/supervised_common.py TOL, applied by tests/test_gpu_supervised.py through check_many) allow AUC and
# TPR a relative deviation of 16 * 2^-24 from the reference's value.
ALLOWANCE = 16 * 2.0 ** -24
MARGIN = 100 * ALLOWANCE


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "golden_selection.json")) as f:
        return json.load(f)


def planted_graph():
    """An undirected planted-partition graph: PLANTED.blocks communities of PLANTED.block_size nodes, an edge inside a community with
    probability p_in and across communities with p_out.  -> (adjacency, seeds: every seeds_every-th node of community 0)."""
    rng = np.random.default_rng(PLANTED["seed"])
    n = PLANTED["blocks"] * PLANTED["block_size"]
    block = np.arange(n) // PLANTED["block_size"]
    upper = np.triu(rng.random((n, n)) < np.where(block[:, None] == block[None, :], PLANTED["p_in"], PLANTED["p_out"]), 1)
    A = sp.csr_array((upper | upper.T).astype(np.float64))
    A.sort_indices()
    return A, [int(v) for v in range(0, PLANTED["block_size"], PLANTED["seeds_every"])]


def family(pg, many):
    """name -> ranker: the PageRank / HeatKernel members of create_many_filters(**FAMILY) (`many`), and for the one-by-one route a
    Normalize-wrapped PageRank, an AbsorbingWalks and a PageRank whose tolerance lies below fp32 eps."""
    rankers = {name: ranker for name, ranker in many.items() if name.startswith(("PPR", "HK"))}
    pre = many["PPR.85"].preprocessor
    rankers["NormPPR.85"] = pg.Normalize(pg.PageRank(alpha=0.85, preprocessor=pre, **FAMILY))
    rankers["Absorb.90"] = many["Absorb.90"]
    rankers["PPR.85@1e-9"] = pg.PageRank(alpha=0.85, preprocessor=pre, tol=1e-9, max_iters=FAMILY["max_iters"])
    return rankers


def problem(pg):
    """(graph, seed signal) of the planted graph."""
    A, seeds = planted_graph()
    graph = pg.AdjacencyWrapper(A, directed=False)
    return graph, pg.to_signal(graph, {v: 1.0 for v in seeds})


def check_case(pg, case, batch):
    """One recorded case through AlgorithmSelection(batch=...): the reference's choice, its values within the allowance of the
    supervised measures' tests and its ranks within tolerance_for.  Returns the tuner and the family."""
    graph, signal = problem(pg)
    rankers = family(pg, pg.create_many_filters(**FAMILY))
    assert list(rankers) == case["names"]
    tuner = pg.AlgorithmSelection(rankers.values(), measure=getattr(pg, case["measure"]), fraction_of_training=case["fractions"],
                                  batch=batch, min_batch_width=2)
    ranks = tuner.rank(graph, signal)
    record = tuner.last_selection
    for name, mine, want in zip(rankers, record["rankers"], case["values"]):
        for got, ref in zip(mine["values"], want):
            print(f"{case['fractions']} {case['measure']} {name} [{mine['route']}]: {got!r} reference {ref!r} "
                  f"(allowed {ALLOWANCE * abs(ref):.3e}, off by {abs(got - ref):.3e})")
    for name, mine, want in zip(rankers, record["rankers"], case["values"]):
        assert len(mine["values"]) == len(want)
        for got, ref in zip(mine["values"], want):
            assert abs(got - ref) <= ALLOWANCE * abs(ref), (name, got, ref)
    assert record["selected"] == case["selected"]
    assert tuner.tune(graph, signal) is list(rankers.values())[case["selected"]]
    assert rel_linf(np.asarray(ranks.np, dtype=np.float64), np.asarray(case["ranks"])) <= tolerance_for({})
    return tuner, rankers
