"""DEV-CONTAINER-ONLY: fixtures of the tuner (tests/test_tuner_host.py, tests/test_gpu_tuner.py) from the reference, imported
read-only with the `wget` shim of SURVEY.md 8c under its numpy backend.  Output: tests/golden/golden_tuner.json.

The reference's AUC calls ``np.array(..., copy=False)`` (measures/supervised.py:262), which numpy 2 refuses whenever a copy is
needed; the subclass below hands ``np.asarray`` copies to the same sklearn calls instead.  Nothing else of the reference is
changed; `optimize` is observed through its module-level candidate builder and a wrapped loss.

Run:  python tests/golden/make_golden_tuner.py
"""
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
os.environ["pygrankBackend"] = "numpy"
os.environ["HOME"] = tempfile.mkdtemp(prefix="pgh_golden_home_")   # import writes ~/.pygrank/config.json
sys.dont_write_bytecode = True
sys.modules["wget"] = types.ModuleType("wget")                      # pygrank/benchmarks/download.py:3
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import sklearn.metrics  # noqa: E402
import pygrank as pg  # noqa: E402
from pygrank.algorithms.autotune import optimization as ref_opt  # noqa: E402

import cases  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)
FRACTION = 0.5
TUNER = dict(fraction_of_training=FRACTION, max_vals=[1] * 11, min_vals=[1] + [0] * 10, divide_range=2, deviation_tol=1e-3, verbose=False)
COMMUNITY = dict(graph="rmat12_sym", centre_seed=5, alpha=0.85, steps=10, size=200, seed_stride=2)


class AUC(pg.AUC):
    def evaluate(self, scores):
        known_scores, scores = self.to_numpy(scores)
        if np.min(known_scores) == np.max(known_scores):
            raise Exception("Cannot evaluate AUC when all labels are the same")
        fpr, tpr, _ = sklearn.metrics.roc_curve(np.asarray(known_scores).copy(), np.asarray(scores).copy())
        return sklearn.metrics.auc(fpr, tpr)


def planted_community(A):
    """The COMMUNITY.size nodes a short personalized walk from one node reaches most, and every COMMUNITY.seed_stride-th as seeds."""
    from oracle import rmat_np
    c = int(rmat_np.seed_nodes(A, 1, seed=COMMUNITY["centre_seed"])[0])
    deg = np.asarray(A.sum(axis=1)).ravel()
    W = A.multiply(1.0 / np.maximum(deg, 1)[:, None]).tocsr()
    e = np.zeros(A.shape[0])
    e[c] = 1.0
    x = e.copy()
    for _ in range(COMMUNITY["steps"]):
        x = COMMUNITY["alpha"] * (W.T @ x) + (1 - COMMUNITY["alpha"]) * e
    community = [int(i) for i in np.argsort(-x, kind="stable")[:COMMUNITY["size"]]]
    return c, community, community[::COMMUNITY["seed_stride"]]


def observed_optimize(loss, **kwargs):
    """The reference's optimize with every step's candidates (its module-level candidate builder is called once per candidate, then
    the loss once per candidate) and losses written down."""
    steps, pending = [], []
    real_add = ref_opt.__dict__["__add"]

    def add(*a, **k):
        out = real_add(*a, **k)
        if not pending or pending[-1]["losses"]:
            pending.append(dict(candidates=[], losses=[]))
        pending[-1]["candidates"].append([float(v) for v in out])
        return out

    def watched(w):
        value = float(loss(w))
        pending[-1]["losses"].append(value)
        return value
    ref_opt.__dict__["__add"] = add
    try:
        result = ref_opt.optimize(watched, **kwargs)
    finally:
        ref_opt.__dict__["__add"] = real_add
    for step in pending:
        best = min(range(len(step["losses"])), key=lambda i: step["losses"][i])
        steps.append(dict(candidates=step["candidates"], losses=step["losses"], chosen=best))
    return [float(v) for v in result], steps


def beale(p):
    return (1.5 - p[0] + p[0] * p[1]) ** 2 + (2.25 - p[0] + p[0] * p[1] ** 2) ** 2 + (2.625 - p[0] + p[0] * p[1] ** 3) ** 2


def quadratic(p):
    return (p[0] - 3) ** 2 + 2 * (p[1] + 4) ** 2 + 0.5 * (p[2] - 7) ** 2 + 0.25 * p[0] * p[1]


def main():
    out = dict(community=COMMUNITY, tuner_args={k: v for k, v in TUNER.items() if k != "verbose"})
    A, directed, _ = cases.GRAPHS[COMMUNITY["graph"]]()
    centre, community, seeds = planted_community(A)
    out["centre"], out["community_nodes"], out["seeds"] = centre, community, seeds
    graph = pg.AdjacencyWrapper(A, directed=directed)
    signal = pg.to_signal(graph, {v: 1.0 for v in seeds})

    # ---- split
    out["split"] = []
    for seed in (0, 1, 2):
        for fraction in (0.9, 0.5, 3, -2):
            tr, te = pg.split(signal, fraction, seed)
            ltr, lte = pg.split(list(seeds), fraction, seed)
            out["split"].append(dict(seed=seed, fraction=fraction,
                                     signal_training=sorted(int(v) for v in tr if tr[v] != 0),
                                     signal_test=sorted(int(v) for v in te if te[v] != 0),
                                     list_training=[int(v) for v in ltr], list_test=[int(v) for v in lte]))
    mtr, mte = pg.split({"a": list(seeds[:10]), "b": list(seeds[10:17])}, 0.5, 1)
    out["split_mapping"] = dict(training={k: [int(v) for v in g] for k, g in mtr.items()},
                                test={k: [int(v) for v in g] for k, g in mte.items()})

    # ---- optimize
    args = dict(max_vals=[4.5, 4.5], min_vals=[-4.5, -4.5], verbose=False)
    result, steps = observed_optimize(beale, **args)
    out["optimize_beale"] = dict(args={k: v for k, v in args.items() if k != "verbose"}, result=result, steps=steps)
    print("beale:", result, len(steps), "steps")
    args = dict(max_vals=[10, 10, 10], min_vals=[-10, -10, -10], coarse=1, depth=2, partition_strategy="step", partitions=1,
                divide_range=1.5, deviation_tol=1e-6, verbose=False)
    result, steps = observed_optimize(quadratic, **args)
    out["optimize_quadratic"] = dict(args={k: v for k, v in args.items() if k != "verbose"}, result=result, steps=steps)
    print("quadratic:", result, len(steps), "steps")

    # ---- ParameterTuner
    training, validation = pg.split(signal, FRACTION, 0)
    known = np.asarray(validation.np, dtype=np.float64)
    kept = np.asarray(training.np, dtype=np.float64) == 0
    positives, negatives = np.flatnonzero(kept & (known != 0)), np.flatnonzero(kept & (known == 0))
    trace = {}

    def optimizer(loss, **kwargs):
        result, steps = observed_optimize(loss, **kwargs)
        trace["steps"] = steps
        return result
    tuner = pg.ParameterTuner(measure=AUC, optimizer=optimizer, **TUNER)
    ranks = tuner.rank(graph, signal)
    terms = len(TUNER["max_vals"])
    for step in trace["steps"]:
        step["flip_budget"] = []
        for w in step["candidates"]:
            scores = np.asarray(tuner.ranker_generator(w).rank(training).np, dtype=np.float64)
            delta = 4 * terms * EPS32 * float(np.max(np.abs(scores)))
            neg = np.sort(scores[negatives])
            close = sum(int(np.searchsorted(neg, s + delta, side="right") - np.searchsorted(neg, s - delta, side="left"))
                        for s in scores[positives])
            step["flip_budget"].append(close / (len(positives) * len(negatives)))
    skipped = 0
    for step in trace["steps"]:
        order = sorted(range(len(step["losses"])), key=lambda i: step["losses"][i])
        gap = step["losses"][order[1]] - step["losses"][order[0]]
        step["argmin_checked"] = bool(gap > step["flip_budget"][order[0]] + step["flip_budget"][order[1]])
        skipped += not step["argmin_checked"]
    truth = pg.to_signal(graph, {v: 1.0 for v in community})
    held_out = float(AUC(truth, exclude=signal)(ranks))
    out["tuner"] = dict(steps=trace["steps"], last_params=[float(v) for v in tuner.last_params], held_out_auc=held_out,
                        num_positive=int(len(positives)), num_negative=int(len(negatives)),
                        skipped_share=skipped / len(trace["steps"]),
                        largest_flip_budget=max(max(step["flip_budget"]) for step in trace["steps"]))
    print(f"tuner: {len(trace['steps'])} steps, skipped share {out['tuner']['skipped_share']:.3f}, held-out AUC {held_out:.6f}, "
          f"largest flip budget {out['tuner']['largest_flip_budget']:.3e}, last_params {out['tuner']['last_params']}")
    path = os.path.join(HERE, "golden_tuner.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
