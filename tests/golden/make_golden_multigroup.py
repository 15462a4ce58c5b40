"""DEV-CONTAINER-ONLY: fixtures of the multi-group measures and of Modularity (tests/test_multigroup_host.py,
tests/test_gpu_multigroup.py) from the reference, imported read-only as in make_golden_ranking.py (numpy backend, the `wget` shim,
epsilon() replaced by the f32 epsilon while the measures are evaluated, np.asarray for the numpy engine's to_primitive).
Output: tests/golden/golden_multigroup.json -- parameters and the reference's f64 results, no vectors.

Graphs: cases.GRAPHS as networkx graphs (nodes 0 .. n - 1).  Scores: three groups from tests/link_common.py:group_scores -- values f32
holds exactly, a share of exact zeros, one all-zero row, two identical rows -- handed to the reference as {group: {node: score}}; the
LAST group's dictionary leaves its zeros out, so `.get(u, 0)` meets missing nodes.

Every value of the reference is checked here against the restatement of tests/link_common.py before it is written:
  LinkAssessment          the labels in their order and the negatives' predictions to the bit, the positives' as a sorted list, the AUC
                          to pairs * 2^-52, the bound of the tests (sklearn's sequential trapezoid sum against the single rounding of
                          two_wins / (2.0 P N); the difference is printed, a few 2^-53 at most)
  Modularity              to 1e-15 of its two terms w^T P w and (sum w d)^2 / 2m (the reference adds samples^2 products one by one)
  ClusteringCoefficient   to 1e-14 relative, or terms * 2^-53 where the reference's one-by-one sum has more than 90 terms

Cases:
  LinkAssessment          graph x hops {1, 2} x {cos, dot} x seeds {0, 7}.  Samples: the defaults (2000 / 2000) on weighted300 and
                          2000 / 300 on rmat10_dir (both graphs are smaller than the sample: every node once, no candidate draw),
                          200 / 300 on rmat12_sym and er10k (the sampling branch; the reference then finishes in seconds), and one er10k
                          case with the defaults
  ClusteringCoefficient   graph x {cos, dot}, seed 1 (the default); the defaults on weighted300 and er10k, 100 samples on the two RMAT
                          graphs (the reference scans an iterator per triplet: cubic in a hub's degree)
  Modularity              graph x max_rank {1, 2} x sample {100: below n, n + 1: above n}, the scores of group 0
  MultiSupervised         AUC, Cos, NDCG x without / with the exclude lists;  MultiUnsupervised  Conductance, Density
  edges                   a graph without edges (AUC raises, Modularity 0, ClusteringCoefficient 0); a single group on weighted300

Run:  PYGRANK_REFERENCE=<checkout of the reference> python tests/golden/make_golden_multigroup.py
"""
import importlib
import json
import os
import sys
import tempfile
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ["pygrankBackend"] = "numpy"
os.environ["HOME"] = tempfile.mkdtemp(prefix="pgh_golden_home_")   # import writes ~/.pygrank/config.json
sys.dont_write_bytecode = True
sys.modules["wget"] = types.ModuleType("wget")                      # pygrank/benchmarks/download.py:3
sys.path.insert(0, os.environ["PYGRANK_REFERENCE"])

import networkx as nx  # noqa: E402
import numpy as np  # noqa: E402
import pygrank as pg  # noqa: E402
import pygrank.core.backend as reference_backend  # noqa: E402
from pygrank.measures.multigroup import ClusteringCoefficient, LinkAssessment, MultiSupervised, MultiUnsupervised  # noqa: E402

import cases  # noqa: E402
import link_common as lc  # noqa: E402

EPS = float(np.finfo(np.float32).eps)
_ENGINE = importlib.import_module("pygrank.core.backend.numpy")


def set_epsilon():
    _ENGINE.to_primitive = np.asarray
    _ENGINE.epsilon = lambda: EPS
    reference_backend.load_backend("numpy")
    assert reference_backend.epsilon() == pg.epsilon() == EPS


LINK_SAMPLES = dict(weighted300=(2000, 2000), rmat10_dir=(2000, 300), rmat12_sym=(200, 300), er10k=(200, 300))
CLUSTERING_SAMPLES = dict(weighted300=2000, rmat10_dir=100, rmat12_sym=100, er10k=2000)
GRAPHS = ["weighted300", "rmat10_dir", "rmat12_sym", "er10k"]


def as_networkx(A, directed):
    G = nx.from_scipy_sparse_array(A, create_using=nx.DiGraph if directed else nx.Graph)
    assert list(G) == list(range(A.shape[0]))
    return G


def score_dicts(S):
    groups = {f"g{j}": {v: float(S[v, j]) for v in range(len(S))} for j in range(S.shape[1])}
    last = f"g{S.shape[1] - 1}"
    groups[last] = {v: x for v, x in groups[last].items() if x != 0}
    return groups


def link_case(G, A, S, groups, hops, similarity, seed, max_positive, max_negative):
    seen = {}

    def measure(real):
        seen["real"] = list(real)

        def evaluate(predicted):
            seen["predicted"] = [float(x) for x in predicted]
            return pg.AUC(real)(predicted)
        return evaluate
    value = float(LinkAssessment(G, measure=measure, hops=hops, similarity=similarity, seed=seed, max_positive_samples=max_positive,
                                 max_negative_samples=max_negative).evaluate(groups))
    mine = lc.pairs(A, hops, max_positive, max_negative, seed)
    predicted = lc.predictions(S, mine["first"], mine["second"], similarity)
    real, theirs = np.array(seen["real"]), np.array(seen["predicted"], dtype=np.float64)
    assert np.array_equal(real, mine["label"]), "labels"
    assert np.array_equal(theirs[real == 0], predicted[real == 0]), "negative predictions differ from the restatement"
    assert np.array_equal(np.sort(theirs[real == 1]), np.sort(predicted[real == 1])), "positive predictions differ from the restatement"
    restated = lc.auc(predicted, mine["label"])
    # sklearn adds one trapezoid per threshold, each add rounds: at most len(real) * 2^-52 in all (observed: a few ulp)
    print("   AUC against the restatement:", abs(restated - value) / 2.0 ** -53, "x 2^-53")
    assert abs(restated - value) <= len(real) * 2.0 ** -52, (restated, value)
    negatives = mine["second"][mine["label"] == 0]
    return dict(hops=hops, similarity=similarity, seed=seed, max_positive=max_positive, max_negative=max_negative, value=value,
                num_pairs=int(len(real)), num_positive=int(real.sum()), first_candidates=[int(v) for v in mine["candidates"][:8]],
                first_negatives=[int(v) for v in negatives[:8]])


def main():
    warnings.simplefilter("ignore")
    set_epsilon()
    out = dict(epsilon=EPS, groups=lc.GROUPS, graphs={})
    for index, key in enumerate(GRAPHS):
        A, directed, _ = cases.GRAPHS[key]()
        n = A.shape[0]
        G = as_networkx(A, directed)
        S = lc.group_scores(n, seed=index)
        groups = score_dicts(S)
        record = dict(directed=bool(directed), scores_seed=index, link=[], clustering=[], modularity=[], multi=[])
        samples = [LINK_SAMPLES[key]] + ([(2000, 2000)] if key == "er10k" else [])
        for max_positive, max_negative in samples:
            default_case = (max_positive, max_negative) != LINK_SAMPLES[key]
            for hops in ((1,) if default_case else (1, 2)):
                for similarity in (("cos",) if default_case else ("cos", "dot")):
                    for seed in ((0,) if default_case else (0, 7)):
                        case = link_case(G, A, S, groups, hops, similarity, seed, max_positive, max_negative)
                        record["link"].append(case)
                        print(key, "link", case)
        for similarity in ("cos", "dot"):
            max_positive = CLUSTERING_SAMPLES[key]
            value = float(ClusteringCoefficient(G, similarity=similarity, max_positive_samples=max_positive).evaluate(groups))
            restated = lc.clustering(A, S, similarity, max_positive, 1)
            # the reference adds one non-negative similarity per (v, u1, u2) in turn: `terms` additions, each rounds once
            degree = np.diff(lc.pattern(A).indptr)
            terms = int(np.dot(np.bincount(lc.sample(n, max_positive, 1)[0], minlength=n), degree * degree))
            print("   clustering against the restatement:", abs(restated - value) / abs(value), "relative,", terms, "terms")
            assert abs(restated - value) <= max(1e-14, terms * 2.0 ** -53) * abs(value), (restated, value)
            record["clustering"].append(dict(similarity=similarity, max_positive=max_positive, seed=1, value=value))
            print(key, "clustering", record["clustering"][-1])
        signal = pg.to_signal(G, groups["g0"])
        for max_rank in (1, 2):
            for max_positive in (100, n + 1):
                value = float(pg.Modularity(G, max_rank=max_rank, max_positive_samples=max_positive, seed=0).evaluate(signal))
                internal, expected, m = lc.modularity_terms(A, directed, S[:, 0], max_rank, max_positive, 0)
                assert m == G.number_of_edges()
                assert abs((internal - expected) / 2 / m - value) <= 1e-15 * (internal + expected), (internal, expected, m, value)
                record["modularity"].append(dict(max_rank=max_rank, max_positive=max_positive, seed=0, value=value, internal=internal,
                                                 expected=expected, edges=m))
                print(key, "modularity", record["modularity"][-1])
        truths = lc.truth_nodes(n, index)
        signals = {name: pg.to_signal(G, {v: float(S[v, j]) for v in range(n)}) for j, name in enumerate(groups)}
        for name in lc.SUPERVISED:
            for excluded in (False, True):
                truth = {f"g{j}": pg.to_signal(G, {v: 1.0 for v in truths[j][0]}) for j in range(lc.GROUPS)}
                exclude = {f"g{j}": truths[j][1] for j in range(lc.GROUPS)} if excluded else None
                value = float(MultiSupervised(getattr(pg, name), truth, exclude).evaluate(signals))
                record["multi"].append(dict(kind="supervised", measure=name, excluded=excluded, value=value))
                print(key, "multi", record["multi"][-1])
        for name in lc.UNSUPERVISED:
            value = float(MultiUnsupervised(getattr(pg, name), G).evaluate(signals))
            record["multi"].append(dict(kind="unsupervised", measure=name, value=value))
            print(key, "multi", record["multi"][-1])
        out["graphs"][key] = record
    # the edges
    empty = nx.empty_graph(5)
    S = lc.group_scores(5, seed=9)
    groups = score_dicts(S)
    edges = {}
    try:
        LinkAssessment(empty).evaluate(groups)
        raise AssertionError("the reference scored a graph without edges")
    except Exception as e:
        edges["link_no_edges_raises"] = str(e)
    edges["modularity_no_edges"] = float(pg.Modularity(empty).evaluate(pg.to_signal(empty, groups["g0"])))
    edges["clustering_no_edges"] = float(ClusteringCoefficient(empty).evaluate(groups))
    A, directed, _ = cases.GRAPHS["weighted300"]()
    G = as_networkx(A, directed)
    S1 = lc.group_scores(A.shape[0], groups=1, seed=5)
    single = score_dicts(S1)
    edges["single_group"] = [link_case(G, A, S1, single, 1, similarity, 0, 2000, 2000) for similarity in ("cos", "dot")]
    out["edges"] = edges
    print("edges", edges)
    path = os.path.join(HERE, "golden_multigroup.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
