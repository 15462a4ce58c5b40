"""DEV-CONTAINER-ONLY: fixtures of HopTuner and arnoldi_iteration (tests/test_hop_tuner_host.py, tests/test_gpu_hop_tuner.py over
tests/hop_common.py) from the reference, imported read-only under its numpy backend with the shims of make_golden_krylov.py and
make_golden_tuner.py (the `wget` module, to_primitive = np.asarray, the AUC subclass).  Output: tests/golden/golden_hop.npz.

Graphs: rmat12_sym with make_golden_tuner.py's planted community (100 seeds: 80 / 20, halves 40 / 40) and weighted300 with its own
personalization.  Per variant of VARIANTS (<v> = its name):
  <v>/values   the K x 2 hop values (K = num_parameters + autoregression)          <v>/params   the tuned hop weights
  <v>/ranks    the ranks of tuner.rank                                              <v>/iters    the returned filter's iterations ("krylov")
  <v>/values_dev, /params_dev, /ranks_dev   max |f32 evaluation - reference| of each (ranks: relative to max |ranks|)
  <v>/flip     for AUC-scored hops, K x 2: the share of (positive, negative) pairs whose reference scores lie within
               4 * hop * eps32 * max |score| of each other -- what a different rounding of the scores may turn around
  <v>/flip_strict   the same without the pairs whose two scores are exact zeros (nodes no walk of that length reaches: every
               evaluation adds nothing there, the tie stays a tie) -- what the tests propagate into the bounds of params and ranks
  <v>/pre_offset, /offsets [steps x candidates], /losses, /loss_flip, /best_loss, /best_loss_flip, /offset   with tunable_offset: the
               weights the search starts from, the candidates and losses of every optimize step (observed_optimize), each loss's
               flip budget (4 * K * eps32 * max |score|, the construction of make_golden_tuner.py) and the chosen offset
and per graph <g>: <g>/seeds (node ids) and <g>/seed_values, <g>/arnoldi_Q [n x 20], <g>/arnoldi_h [21 x 20] of
arnoldi_iteration(M, personalization, 20) (the columns of a shorter run are its leading columns), <g>/power_linf [20] the largest entry
of every power of the personalization (what a change of a hop weight moves the ranks by at most), and <g>/arnoldi_Q_dev/<k>,
<g>/arnoldi_h_dev/<k> for k = 6, 10, 20: max |f32 evaluation - reference| over the leading k columns, relative to max |Q| and max |h|.
The "arnoldi" variants and the Arnoldi deviations are recorded for both of the engine's routes: the fused one under the names above and
the primitive loop (`emulate_arnoldi_primitive`: f32 coefficients in f32 elementwise operations, so a less accurate evaluation) under
<v>/values_dev_primitive, /params_dev_primitive, /ranks_dev_primitive and <g>/arnoldi_Q_dev_primitive/<k>, /arnoldi_h_dev_primitive/<k>.

The f32 evaluation is the reference's own code with the engine's storage: conv rounds the operator's values, its operand and its
result to f32 (sums in f64), the ranks are rounded to f32, and arnoldi_iteration is replaced by `emulate_arnoldi` -- the engine's route
(include/pgh_arnoldi.h: raw f32 columns with a scale each, the Gram identity solved in f64, one f32 division per column).  The tests
allow 8 times these deviations: the device only adds other summation orders on top of the same storage rounding.

Run:  python tests/golden/make_golden_hop.py
"""
import importlib
import os
import warnings

import numpy as np

import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))      # tests/hop_common.py

import make_golden_tuner as mgt  # noqa: E402                       # the shims, the AUC subclass, the planted community
import pygrank as pg
import pygrank.core.backend as reference_backend
from pygrank.algorithms.autotune import hop_tuner as ref_hop

import cases
import hop_common
from hop_common import ARNOLDI_DIMS, VARIANTS

HERE = os.path.dirname(os.path.abspath(__file__))
_ENGINE = importlib.import_module("pygrank.core.backend.numpy")
_ENGINE.to_primitive = np.asarray                                   # what np.array(obj, copy=False) meant before numpy 2 refused it
reference_backend.load_backend("numpy")

EPS32 = float(np.finfo(np.float32).eps)
f32 = lambda v: np.asarray(v, dtype=np.float32)                     # noqa: E731
f64 = lambda v: np.asarray(v, dtype=np.float64)                     # noqa: E731

MEASURES = {"Cos": pg.Cos, "AUC": mgt.AUC}


def graphs():
    A, directed, _ = cases.GRAPHS["rmat12_sym"]()
    _, _, seeds = mgt.planted_community(A)
    out = {"rmat12": (pg.AdjacencyWrapper(A, directed=directed), [int(v) for v in seeds], [1.0] * len(seeds))}
    A, directed, p = cases.GRAPHS["weighted300"]()
    nodes = [int(v) for v in np.flatnonzero(p)]
    out["w300"] = (pg.AdjacencyWrapper(A, directed=directed), nodes, [float(f32(p[v])) for v in nodes])   # (values an f32 vector holds)
    return out


def _rounded(M):
    M32 = getattr(M, "array", M).copy().astype(np.float64)
    M32.data = f64(f32(M32.data))
    return M32


class F32Storage:
    """While active: conv stores in f32, arnoldi_iteration is `arnoldi` (one of the engine's two routes)."""
    _cache = {}

    def __init__(self, arnoldi):
        self.replacement = arnoldi

    def __enter__(self):
        # (constructing a filter loads the backend again, which rebinds pygrank.core.backend.conv from the engine module: the
        # replacement goes into the engine module itself)
        self.conv, self.arnoldi = _ENGINE.conv, ref_hop.arnoldi_iteration

        def conv(x, M):
            key = id(M)
            if key not in self._cache:
                self._cache[key] = (M, _rounded(M))
            return f64(f32(f64(f32(x)) @ self._cache[key][1]))
        _ENGINE.conv = conv
        reference_backend.load_backend("numpy")
        ref_hop.arnoldi_iteration = self.replacement
        return self

    def __exit__(self, *exc):
        _ENGINE.conv, ref_hop.arnoldi_iteration = self.conv, self.arnoldi
        reference_backend.load_backend("numpy")
        self._cache.clear()


def emulate_arnoldi(M, b, n):
    """pygrank_amd.krylov._arnoldi_fused in numpy -> (Q f64 of the stored f32 slab, h)."""
    M32 = _rounded(M)
    r = f32(b)
    total = float(np.abs(f64(r)).sum())
    scales = [1.0 / total if total != 0 else 1.0]
    slab = np.zeros((len(r), n), dtype=np.float32)
    slab[:, 0] = r
    h = [[0 for _ in range(n)] for _ in range(n + 1)]
    gram = np.zeros((n, n))
    for k in range(1, n):
        m = 2.0 ** round(np.log2(scales[k - 1]))
        rho = scales[k - 1] / m
        w = f32(m * f64(f32(f64(r) @ M32)))
        basis = f64(slab[:, :k])
        s = np.asarray(scales)
        c = s * rho * (basis.T @ f64(w))
        coefficients = np.zeros(k)
        for j in range(k):
            coefficients[j] = c[j] - gram[j, :j] @ coefficients[:j]
        out = f32(f64(w) - basis @ (coefficients * s / rho))
        raw_norm = float((f64(out) ** 2).sum()) ** 0.5
        for j in range(k):
            h[j][k - 1] = float(coefficients[j])
        h[k][k - 1] = rho * raw_norm
        scales.append(1.0 / raw_norm if raw_norm != 0 else 1.0)
        gram[k, :k] = scales[k] * s * (basis.T @ f64(out))
        slab[:, k] = out
        r = out
    return f64(slab / f32([1.0 / s for s in scales])[None, :]), h


def emulate_arnoldi_primitive(M, b, n):
    """pygrank_amd.krylov._arnoldi_primitive in numpy: the reference's loop with every vector, every scalar operand of an elementwise
    operation and every elementwise outcome rounded to f32 (dots in f64 from the stored vectors)."""
    M32 = _rounded(M)
    b = f32(b)
    total = float(np.abs(f64(b)).sum())
    Q = [f32(b / np.float32(total)) if total != 0 else b]
    h = [[0 for _ in range(n)] for _ in range(n + 1)]
    for k in range(1, n):
        v = f32(f64(Q[k - 1]) @ M32)
        for j in range(k):
            h[j][k - 1] = float(f64(Q[j]) @ f64(v))
            v = f32(v - f32(Q[j] * np.float32(h[j][k - 1])))
        h[k][k - 1] = float(f64(v) @ f64(v)) ** 0.5
        Q.append(f32(v / np.float32(h[k][k - 1])) if h[k][k - 1] != 0 else v * 0)
    return f64(np.stack(Q, axis=1)), h


EMULATIONS = {"fused": emulate_arnoldi, "primitive": emulate_arnoldi_primitive}


def pair_share(scores, positives, negatives, delta):
    neg = np.sort(scores[negatives])
    close = sum(int(np.searchsorted(neg, s + delta, side="right") - np.searchsorted(neg, s - delta, side="left")) for s in scores[positives])
    return close / (len(positives) * len(negatives))


def run(variant, graph, signal, f32_storage):
    """One reference run (f32_storage: None, or the route of EMULATIONS to evaluate in f32 storage) -> dict(values, params, ranks, iters, scored [the vectors the hop measure saw], offset trace)."""
    _, measure_name, basis, num_parameters, autoregression, offset_name = VARIANTS[variant]
    seen = dict(values=[], scored=[], run_params=[])
    cls = MEASURES[measure_name]

    def measure(known, exclude):
        inner = cls(known, exclude)

        class Recording:
            def __call__(self, scores):
                value = float(inner(scores))
                seen["values"].append(value)
                seen["scored"].append(f64(scores).copy())
                return value
        return Recording()
    tuner = pg.HopTuner(measure=measure, basis=basis, num_parameters=num_parameters, autoregression=autoregression,
                        tunable_offset=None if offset_name is None else MEASURES[offset_name])
    real_run = tuner._run

    def watched_run(personalization, params, *args, **kwargs):
        seen["run_params"].append(([float(v) for v in params], personalization))
        return real_run(personalization, params, *args, **kwargs)
    tuner._run = watched_run
    trace = {}
    real_optimize = ref_hop.optimize

    def optimizer(loss, **kwargs):
        result, steps = mgt.observed_optimize(loss, verbose=False, **kwargs)
        trace["steps"], trace["result"] = steps, result
        return result
    ref_hop.optimize = optimizer
    try:
        if f32_storage:
            with F32Storage(EMULATIONS[f32_storage]):
                ranker, personalization = tuner._tune(graph, signal)
                ranks = f64(f32(ranker.rank(graph, personalization).np))
        else:
            ranker, personalization = tuner._tune(graph, signal)
            ranks = f64(ranker.rank(graph, personalization).np)
    finally:
        ref_hop.optimize = real_optimize
    hops = num_parameters + autoregression
    out = dict(values=np.array(seen["values"][:2 * hops]).reshape(hops, 2), scored=seen["scored"][:2 * hops], ranks=ranks, trace=trace,
               run_params=seen["run_params"], tuner=tuner)
    if basis == "krylov":
        out["params"], out["iters"] = f64([float(v) for v in ranker.weights]), int(ranker.convergence.iteration)
    else:
        # (the weights of the last _run are the tuned ones; _run divides them by their absolute sum itself)
        out["params"], out["iters"] = f64(seen["run_params"][-1][0]), 0
    return out


def main():
    warnings.simplefilter("ignore")
    out = dict(factor=np.float64(hop_common.FACTOR))
    loaded = graphs()
    for key, (graph, nodes, values) in loaded.items():
        signal = pg.to_signal(graph, dict(zip(nodes, values)))
        out[key + "/seeds"], out[key + "/seed_values"] = np.array(nodes, dtype=np.int64), f64(values)
        M = pg.GenericGraphFilter([1.0]).preprocessor(graph)
        Q, h = pg.arnoldi_iteration(M, f64(signal.np), max(ARNOLDI_DIMS))
        Q, h = f64(Q), f64(h)
        emulated = {route: emulate(M, f64(signal.np), max(ARNOLDI_DIMS)) for route, emulate in EMULATIONS.items()}
        out[key + "/arnoldi_Q"], out[key + "/arnoldi_h"] = Q, h
        power, tops = f64(signal.np), []
        for _ in range(max(ARNOLDI_DIMS)):
            tops.append(float(np.abs(power).max()))
            power = reference_backend.conv(power, M)
        out[key + "/power_linf"] = f64(tops)
        for k in ARNOLDI_DIMS:
            # a run of k columns is the leading part of a longer one (checked here for the reference itself)
            Qk, hk = pg.arnoldi_iteration(M, f64(signal.np), k)
            assert np.array_equal(f64(Qk), Q[:, :k]) and np.array_equal(f64(hk)[:k, :k - 1], h[:k, :k - 1])
            for route, (Qe, he) in emulated.items():
                he = f64(he)
                q_dev = float(np.abs(Qe[:, :k] - Q[:, :k]).max() / np.abs(Q[:, :k]).max())
                h_dev = float(np.abs(he[:k, :k - 1] - h[:k, :k - 1]).max() / np.abs(h[:k, :k - 1]).max())
                tail = "" if route == "fused" else "_" + route
                out[f"{key}/arnoldi_Q_dev{tail}/{k}"], out[f"{key}/arnoldi_h_dev{tail}/{k}"] = np.float64(q_dev), np.float64(h_dev)
                print(key, "arnoldi", k, route, "Q dev", q_dev, "h dev", h_dev)
    for variant, (key, measure_name, basis, num_parameters, autoregression, offset_name) in VARIANTS.items():
        graph, nodes, values = loaded[key]
        signal = pg.to_signal(graph, dict(zip(nodes, values)))
        ref = run(variant, graph, signal, None)
        emu = run(variant, graph, signal, "fused")
        scale = float(np.abs(ref["ranks"]).max())
        devs = dict(values_dev=float(np.abs(emu["values"] - ref["values"]).max()), params_dev=float(np.abs(emu["params"] - ref["params"]).max()),
                    ranks_dev=float(np.abs(emu["ranks"] - ref["ranks"]).max() / scale) if scale else float(np.abs(emu["ranks"]).max()))
        out[variant + "/values"], out[variant + "/params"], out[variant + "/ranks"] = ref["values"], ref["params"], ref["ranks"]
        out[variant + "/iters"] = np.int64(ref["iters"])
        for what, value in devs.items():
            out[variant + "/" + what] = np.float64(value)
        if basis != "krylov":
            other = run(variant, graph, signal, "primitive")
            for what in ("values", "params", "ranks"):
                dev = float(np.abs(other[what] - ref[what]).max() / (scale if what == "ranks" and scale else 1.0))
                out[f"{variant}/{what}_dev_primitive"] = np.float64(dev)
                print("    primitive route:", what, "off by", dev)
            if measure_name == "AUC":
                emu["values_primitive"] = other["values"]
        print(variant, "iters", ref["iters"], devs, "params", [round(float(v), 4) for v in ref["params"][:4]], "...")
        # ---- the splits, as the reference deals them (the tests rebuild them with the port's split)
        training, validation = pg.split(pg.to_signal(signal, f64(signal.np)), 0.8)
        halves = pg.split(training, 0.5)
        known = f64(validation.np)
        if measure_name == "AUC":
            hops = num_parameters + autoregression
            flip = np.zeros((hops, 2))
            for at, scores in enumerate(ref["scored"]):
                hop, half = divmod(at, 2)
                kept = f64(halves[half].np) == 0
                positives, negatives = np.flatnonzero(kept & (known != 0)), np.flatnonzero(kept & (known == 0))
                flip[hop, half] = pair_share(scores, positives, negatives, 4 * hop * EPS32 * float(np.abs(scores).max()))
            out[variant + "/flip"] = flip
            strict = np.zeros((hops, 2))
            for at, scores in enumerate(ref["scored"]):
                hop, half = divmod(at, 2)
                kept = f64(halves[half].np) == 0
                positives, negatives = np.flatnonzero(kept & (known != 0)), np.flatnonzero(kept & (known == 0))
                zero_pairs = int((scores[positives] == 0).sum()) * int((scores[negatives] == 0).sum())
                strict[hop, half] = flip[hop, half] - zero_pairs / (len(positives) * len(negatives))
            out[variant + "/flip_strict"] = strict
            print("    flip budgets per hop", np.round(flip.max(axis=1), 6).tolist(), "without the pairs of two exact zeros", np.round(strict.max(axis=1), 6).tolist())
            print("    largest flip budget of a hop", float(flip.max()), "emulated values off by", float(np.abs(emu["values"] - ref["values"]).max()))
            for what in ("values", "values_primitive"):
                assert what not in emu or np.all(np.abs(emu[what] - ref["values"]) <= flip + 1e-12), (variant, what)
        if offset_name is not None:
            steps = ref["trace"]["steps"]
            tuner = ref["tuner"]
            hops = num_parameters + autoregression
            kept = f64(training.np) == 0
            positives, negatives = np.flatnonzero(kept & (known != 0)), np.flatnonzero(kept & (known == 0))
            # the weights of the first probe are pre_offset + its offset
            first_weights, _ = ref["run_params"][0]
            pre_offset = f64(first_weights) - steps[0]["candidates"][0][0]
            base = None
            if basis != "krylov":
                base = pg.arnoldi_iteration(tuner.ranker_generator([None] * hops).preprocessor(graph), f64(halves[0].np), hops)[0]
            budgets = []
            for step in steps:
                row = []
                for candidate in step["candidates"]:
                    weights = [float(v + candidate[0]) for v in pre_offset]
                    scores = f64(pg.HopTuner._run(tuner, training, weights, base).np)
                    row.append(pair_share(scores, positives, negatives, 4 * hops * EPS32 * float(np.abs(scores).max())))
                budgets.append(row)
            out[variant + "/pre_offset"] = pre_offset
            out[variant + "/offsets"] = f64([[c[0] for c in step["candidates"]] for step in steps])
            out[variant + "/losses"] = f64([step["losses"] for step in steps])
            out[variant + "/loss_flip"] = f64(budgets)
            losses = out[variant + "/losses"]
            at = np.unravel_index(np.argmin(losses), losses.shape)
            out[variant + "/best_loss"], out[variant + "/best_loss_flip"] = np.float64(losses[at]), np.float64(f64(budgets)[at])
            out[variant + "/offset"] = np.float64(ref["trace"]["result"][0])
            print("    offset", ref["trace"]["result"], "steps", len(steps), "losses", losses.tolist(), "largest flip budget", float(np.max(budgets)))
    path = os.path.join(HERE, "golden_hop.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
