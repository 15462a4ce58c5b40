#!/usr/bin/env python3
"""Times one coordinate step of the default ParameterTuner (5 candidates that differ in one of 41 weights) two ways, on RMAT
graphs built on the device with 100 seeds drawn as bench.py draws them:

  (a) fused:      the tuner's `many` -- pgh_probe_auc, one streaming pass over the power slab for all candidates;
  (b) sequential: the same candidates one by one through GenericGraphFilter(..., optimization_dict=...).rank + Normalize +
                  measures.AUC(validation, exclude=training) -- the reference's evaluation (parameterized.py:135-145), which already
                  reads the stored powers (one pgh_mat_gemv per candidate).

Both routes are timed with pgh_timer_* (events on the engine's stream, host work between the launches included) in ONE process,
alternating, after a warm-up step; medians and min..max spreads over steps x repetitions are reported, with the call of
pgh_probe_auc alone and its GB/s (bytes from shapes: the 128-byte lines of every 256-byte slab row that the leading `terms` floats
touch, plus one class byte per node).  Needs an MI355X: there is no fallback.

    python tools/tune_bench.py --scale 23 --steps 8 [--reps 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Timer:
    def __init__(self, L):
        self.L, self.lib, self.h = L, L.lib(), L.c_timer()
        L.check(self.lib.pgh_timer_create(C.byref(self.h)))

    def time(self, fn):
        self.L.check(self.lib.pgh_timer_start(self.h))
        value = fn()
        self.L.check(self.lib.pgh_timer_stop(self.h))
        ms = C.c_double()
        self.L.check(self.lib.pgh_timer_elapsed_ms(self.h, C.byref(ms)))
        return ms.value, value


def summary(samples):
    return dict(median_ms=round(statistics.median(samples), 4), min_ms=round(min(samples), 4), max_ms=round(max(samples), 4),
                samples=len(samples))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--l1", action="store_true",
                    help="stop the filters on the L1 change instead of the default mean absolute change: on a graph of millions of nodes "
                         "the default rule (tol 1e-6 on |c_k| * |term_k|_1 / n) ends every expansion after its first term, the L1 rule "
                         "lets all 41 weights through")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    from pygrank_amd import autotune
    from pygrank_amd.synthetic import rmat_graph
    pg.load_backend("hip")
    L.ensure_init()                                          # raises without an MI355X
    if L.entry("pgh_probe_auc") is None:
        raise SystemExit("the engine library lacks pgh_probe_auc")
    adj = rmat_graph(args.scale, args.ef, seed=0, normalization="col", a=0.57, b=0.19, c=0.19)
    n = adj.array.shape[0]
    candidates_nodes = np.flatnonzero(np.asarray(pg.degrees(adj.array)) > 0)
    rng = np.random.default_rng(1)
    p = np.zeros(n)
    p[np.sort(rng.choice(candidates_nodes, size=min(args.seeds, len(candidates_nodes)), replace=False))] = 1.0
    signal = pg.to_signal(adj, p)

    tuner = pg.ParameterTuner(verbose=False, **(dict(error_type=pg.L1) if args.l1 else {}))
    splits = tuner._splits(signal, 0)
    loss = tuner._loss(splits, (), {})
    opt = tuner.optimize_args
    weights = [(lo + hi) / 2 for lo, hi in zip(opt["min_vals"], opt["max_vals"])]
    ranges = [(hi - lo) / 2 for lo, hi in zip(opt["min_vals"], opt["max_vals"])]
    timer = Timer(L)

    def step_candidates(variable):
        ranges[variable] /= opt["divide_range"]
        return [autotune._add(weights, variable, ranges[variable] * (part * 2. / (opt["partitions"] - 1) - 1),
                              opt["max_vals"][variable], opt["min_vals"][variable]) for part in range(opt["partitions"])]

    def fused(cands):
        return loss.many(cands)

    def sequential(cands):
        return [loss(w) for w in cands]

    def entry_only(cands):
        from pygrank_amd.filters import GenericGraphFilter
        variants = [GenericGraphFilter(w, **tuner._filter_kwargs) for w in cands]
        training, validation, exclude = splits[0]
        slab, coeffs, _ = variants[0].probe_coefficients(training, None, variants)
        ms, aucs = timer.time(lambda: loss._fused(0, validation, exclude, slab, coeffs))
        return ms, coeffs.shape[0]

    variables = [v for v in range(len(weights)) if ranges[v] > 0]
    cands = step_candidates(variables[0])
    fused(cands), sequential(cands), entry_only(cands)        # warm-up step: builds the slab, the plan and every code object
    a_ms, b_ms, e_ms, worst, terms = [], [], [], 0.0, 0
    for step in range(args.steps):
        cands = step_candidates(variables[(step + 1) % len(variables)])
        got_a = got_b = None
        for _ in range(args.reps):
            ms, got_a = timer.time(lambda: fused(cands))
            a_ms.append(ms)
            ms, got_b = timer.time(lambda: sequential(cands))
            b_ms.append(ms)
            ms, terms = entry_only(cands)
            e_ms.append(ms)
        worst = max(worst, max(abs(x - y) for x, y in zip(got_a, got_b)))
        weights = cands[min(range(len(cands)), key=lambda i: got_a[i])]
    if tuner.last_tune["unfused_steps"]:
        raise SystemExit(f"the fused route was not taken: {tuner.last_tune}")
    a, b, e = summary(a_ms), summary(b_ms), summary(e_ms)
    lines = -(-(4 * 4 * -(-int(terms) // 4)) // 128)          # 128-byte lines of a 256-byte slab row that the leading terms touch
    stream_bytes = n * 128 * lines + n
    out = dict(tool="tune_bench", scale=args.scale, edge_factor=args.ef, n=int(n), seeds=args.seeds, steps=args.steps, reps=args.reps,
               candidates_per_step=opt["partitions"], stopping_rule="L1" if args.l1 else "default (Mabs)", terms=int(terms), fused=a, sequential=b, probe_auc_call=e,
               ratio_fused_over_sequential=round(a["median_ms"] / b["median_ms"], 4),
               spreads_disjoint=bool(a["max_ms"] < b["min_ms"] or b["max_ms"] < a["min_ms"]),
               stream_bytes=int(stream_bytes), probe_auc_gbps=round(stream_bytes / (e["median_ms"] * 1e-3) / 1e9, 1),
               largest_loss_difference_between_routes=worst, positives=loss._plans[0].num_positive,
               negatives=loss._plans[0].num_negative, routes=dict(tuner.last_tune))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
