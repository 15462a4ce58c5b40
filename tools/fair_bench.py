#!/usr/bin/env python3
"""Times coordinate steps of the default FairPersonalizer (PageRank base ranker, one bucket, max_residual 0: 10 candidates that differ
in one of the 5 parameters, the last of which has the empty range [0, 0] and so yields ten equal candidates, as in `optimize`) two ways,
on RMAT graphs built on the device with 100 seeds drawn as bench.py draws them and a random fifth of the nodes as the
sensitive group:

  (a) batched:    the loss's `many` -- pgh_prior_edit writes the candidates' edited priors into one slab, PageRank.propagate runs the
                  multi-seed loop, evaluate_many scores the columns;
  (b) sequential: the same candidates one by one through `loss` -- the reference's route (fairness.py:123-132), what batch=False runs.

Both routes are timed with pgh_timer_* (events on the engine's stream, host work between the launches included) in ONE process,
alternating, after a warm-up step; medians and min..max spreads over steps x repetitions are reported, with the call of pgh_prior_edit
alone and its GB/s (bytes from shapes: 12 n read, 4 n probes written).  Needs an MI355X: there is no fallback.

--tol is the base ranker's tolerance: the run for the original scores stops by it and fixes the iteration count of every candidate's run.

    python tools/fair_bench.py --scale 23 --steps 8 [--reps 3] [--tol 1e-6] [--out profiles/fairness/fair_bench_scale23.log]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tune_bench import Timer, summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    from pygrank_amd import autotune
    from pygrank_amd.synthetic import rmat_graph
    pg.load_backend("hip")
    L.ensure_init()                                          # raises without an MI355X
    if L.entry("pgh_prior_edit") is None:
        raise SystemExit("the engine library lacks pgh_prior_edit")
    adj = rmat_graph(args.scale, args.ef, seed=0, normalization="col", a=0.57, b=0.19, c=0.19)
    n = adj.array.shape[0]
    nodes = np.flatnonzero(np.asarray(pg.degrees(adj.array)) > 0)
    rng = np.random.default_rng(1)
    p = np.zeros(n)
    p[np.sort(rng.choice(nodes, size=min(args.seeds, len(nodes)), replace=False))] = 1.0
    s = np.zeros(n)
    s[rng.choice(n, n // 5, replace=False)] = 1.0
    signal, sensitive = pg.to_signal(adj, p), pg.to_signal(adj, s)

    personalizer = pg.FairPersonalizer(pg.PageRank(alpha=0.85, tol=args.tol), 0.8, pRule_weight=10, verbose=False)
    loss = personalizer._open(adj, signal, sensitive, (), {})
    iterations = int(personalizer.ranker.convergence.max_iters)
    hi, lo, partitions = [1, 1, 5, 5, personalizer.max_residual], [0, 0, -5, -5, 0], 10
    weights = [(a + b) / 2 for a, b in zip(lo, hi)]
    ranges = [(b - a) / 2 for a, b in zip(lo, hi)]
    timer = Timer(L)

    def step_candidates(variable):
        ranges[variable] /= 2
        return [autotune._add(weights, variable, ranges[variable] * (part * 2. / (partitions - 1) - 1), hi[variable], lo[variable])
                for part in range(partitions)]

    try:
        cands = step_candidates(0)
        loss.many(cands), [loss(w) for w in cands], loss._slab(cands)     # warm-up step: every code object, every pooled block
        a_ms, b_ms, e_ms, worst = [], [], [], 0.0
        for step in range(args.steps):
            cands = step_candidates((step + 1) % len(weights))
            got_a = got_b = None
            for _ in range(args.reps):
                ms, got_a = timer.time(lambda: loss.many(cands))
                a_ms.append(ms)
                ms, got_b = timer.time(lambda: [loss(w) for w in cands])
                b_ms.append(ms)
                ms, _ = timer.time(lambda: loss._slab(cands))
                e_ms.append(ms)
            worst = max(worst, max(abs(x - y) for x, y in zip(got_a, got_b)))
            weights = cands[min(range(len(cands)), key=lambda i: got_a[i])]
    finally:
        loss.close()
    a, b, e = summary(a_ms), summary(b_ms), summary(e_ms)
    edit_bytes = 12 * n + 4 * n * partitions
    out = dict(tool="fair_bench", scale=args.scale, edge_factor=args.ef, n=int(n), seeds=args.seeds, tol=args.tol,
               max_residual=personalizer.max_residual, steps=args.steps,
               reps=args.reps, candidates_per_step=partitions, iterations_per_run=iterations, batched=a, sequential=b, prior_edit_call=e,
               ratio_batched_over_sequential=round(a["median_ms"] / b["median_ms"], 4),
               spreads_disjoint=bool(a["max_ms"] < b["min_ms"] or b["max_ms"] < a["min_ms"]),
               edit_bytes=int(edit_bytes), prior_edit_gbps=round(edit_bytes / (e["median_ms"] * 1e-3) / 1e9, 1),
               largest_loss_difference_between_routes=worst, routes=dict(personalizer.last_fit))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
