"""DEV-CONTAINER-ONLY: fixture of AlgorithmSelection (tests/test_selection_host.py, tests/test_gpu_selection.py) from the reference,
imported read-only with the `wget` shim of SURVEY.md 8c under its numpy backend.  Output: tests/golden/golden_selection.json.

The reference's AUC calls ``np.array(..., copy=False)`` (measures/supervised.py:262), which numpy 2 refuses whenever a copy is needed;
the subclass below hands ``np.asarray`` copies to the same sklearn calls instead (as tests/golden/make_golden_tuner.py does).  Nothing
else of the reference is changed.

On the planted graph of tests/selection_common.py, for every fraction_of_training setting of FRACTIONS and each measure of MEASURES,
AlgorithmSelection over selection_common.family(create_many_filters(tol=1e-6)) -- its PageRank and HeatKernel members plus a
Normalize-wrapped PageRank, an AbsorbingWalks and a PageRank at tol = 1e-9: per ranker best_direction * measure on every split, the
index of the selected ranker and the ranks tuner.rank returns.  Also the names and parameters of create_demo_filters and
create_many_filters.

ASSERTED for every case: the selected ranker's value (the least over its splits) leads the runner-up's by at least MARGIN = 100 x the
relative deviation the GPU supervised tests allow AUC and TPR (tests/supervised_common.py TOL = 16 * 2^-24, applied by
tests/test_gpu_supervised.py), times the larger of the two magnitudes: an f32 run cannot legitimately select another ranker.

Run:  PYGRANK_REFERENCE=<checkout of the reference> python tests/golden/make_golden_selection.py
"""
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

import numpy as np  # noqa: E402
import sklearn.metrics  # noqa: E402
import pygrank as pg  # noqa: E402
from pygrank.benchmarks import comparables  # noqa: E402

import selection_common as sc  # noqa: E402


class AUC(pg.AUC):
    def evaluate(self, scores):
        known_scores, scores = self.to_numpy(scores)
        if np.min(known_scores) == np.max(known_scores):
            raise Exception("Cannot evaluate AUC when all labels are the same")
        fpr, tpr, _ = sklearn.metrics.roc_curve(np.asarray(known_scores).copy(), np.asarray(scores).copy())
        return sklearn.metrics.auc(fpr, tpr)


MEASURES = dict(AUC=AUC, TPR=pg.TPR)


def describe(rankers):
    """[[name, class, {alpha or t, tol, max_iters, normalization}]] of a family, in its order."""
    out = []
    for name, ranker in rankers.items():
        params = {key: float(getattr(ranker, key)) for key in ("alpha", "t") if hasattr(ranker, key)}
        params.update(tol=float(ranker.convergence.tol), max_iters=int(ranker.convergence.max_iters))
        out.append([name, type(ranker).__name__, params])
    return out


def values_of(rankers, measure, fractions, signal):
    """selection.py:69-75 per ranker: best_direction * measure on every split."""
    table = []
    for ranker in rankers:
        row = []
        for seed, fraction in enumerate(fractions):
            training, validation = pg.split(signal, fraction, seed=seed)
            m = measure(validation, training)
            row.append(float(m.best_direction() * m.evaluate(ranker.rank(training, graph_dropout=0))))
        table.append(row)
    return table


def main():
    warnings.simplefilter("ignore")
    graph, signal = sc.problem(pg)
    out = dict(planted=sc.PLANTED, family=sc.FAMILY, allowance=sc.ALLOWANCE, margin=sc.MARGIN,
               demo_filters=describe(comparables.create_demo_filters()), many_filters=describe(comparables.create_many_filters()),
               seeds=[int(v) for v in signal if signal[v] != 0], cases=[])
    for fractions in sc.FRACTIONS:
        for name in sc.MEASURES:
            rankers = sc.family(pg, comparables.create_many_filters(**sc.FAMILY))
            tuner = pg.AlgorithmSelection(rankers.values(), measure=MEASURES[name], fraction_of_training=fractions)
            best = tuner.tune(graph, signal)
            selected = [ranker is best for ranker in rankers.values()].index(True)
            listed = fractions if isinstance(fractions, list) else [fractions]
            table = values_of(list(rankers.values()), MEASURES[name], listed, signal)
            least = [min(row) for row in table]
            order = sorted(range(len(least)), key=lambda i: -least[i])
            assert order[0] == selected, (fractions, name, order[:3], selected)
            lead = least[order[0]] - least[order[1]]
            needed = sc.MARGIN * max(abs(least[order[0]]), abs(least[order[1]]))
            print(f"{fractions} {name}: selected {list(rankers)[selected]} {least[order[0]]:.9f}, runner-up {list(rankers)[order[1]]} "
                  f"{least[order[1]]:.9f}, lead {lead:.3e} (needed {needed:.3e})")
            assert lead >= needed, (fractions, name, lead, needed)
            ranks = tuner.rank(graph, signal)
            out["cases"].append(dict(fractions=fractions, measure=name, names=list(rankers), values=table, selected=selected,
                                     ranks=[float(v) for v in np.asarray(ranks.np, dtype=np.float64)]))
    path = os.path.join(HERE, "golden_selection.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
