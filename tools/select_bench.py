#!/usr/bin/env python3
"""Times one AlgorithmSelection._tune two ways on an RMAT graph built on the device, with 100 seeds drawn as bench.py draws them
(SURVEY.md 8d):

  (a) batch:      the default route -- the family's PageRanks and closed-form filters as mixed batches (include/pgh_mixed.h), every
                  other ranker one by one;
  (b) one by one: batch=False -- one rank() per ranker and split, through the single-vector loops only.

--filters many: create_many_filters(tol) -- on a graph that is already preprocessed both of its preprocessors return that graph, so
the 24 filters share one image: two PageRank groups and two HeatKernel groups of 4 rankers each, 8 AbsorbingWalks one by one on both
routes.  --filters demo: create_demo_filters(tol=--tol): 3 PageRanks and 3 HeatKernels.  --splits k: fraction_of_training =
[0.9, 0.8, ...][:k], so a group's batch is 4 k (demo: 3 k) columns wide.  --l1: the filters stop on the L1 change instead of the
default mean absolute change (on millions of nodes the default rule at tol 1e-6 ends every run within a few iterations).

Both routes are timed in ONE process, alternating, after one warm-up run of each: the engine's stream events around the whole _tune
(pgh_timer_*, host work between the launches included) and the host's wall clock around the same call (it ends synchronised: the
values are host floats).  Medians and min..max over --reps repetitions.  Both routes must select the same ranker.  Needs an MI355X.

--min-width w: the batch route's min_batch_width (default 2, so that the mixed batches are what is timed at every width).

    python tools/select_bench.py --scale 23 --filters many [--splits 1] [--reps 3] [--l1] [--out profiles/selection/NAME.log]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tune_bench import Timer, summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--filters", choices=("many", "demo"), default="many")
    ap.add_argument("--splits", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--l1", action="store_true")
    ap.add_argument("--min-width", type=int, default=2,
                    help="min_batch_width of the batch route (2: every group of two or more rankers is batched, whatever its width)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    from pygrank_amd.synthetic import rmat_graph
    pg.load_backend("hip")
    L.ensure_init()                                          # raises without an MI355X
    for name in L.MIXED_SIGNATURES:
        if L.entry(name) is None:
            raise SystemExit("the engine library lacks " + name)
    adj = rmat_graph(args.scale, args.ef, seed=0, normalization="col", a=0.57, b=0.19, c=0.19)
    n = adj.array.shape[0]
    nodes = np.flatnonzero(np.asarray(pg.degrees(adj.array)) > 0)
    p = np.zeros(n)
    p[np.sort(np.random.default_rng(1).choice(nodes, size=min(args.seeds, len(nodes)), replace=False))] = 1.0
    signal = pg.to_signal(adj, p)
    fractions = [0.9, 0.8, 0.7, 0.6, 0.5, 0.4][:args.splits]
    if len(fractions) != args.splits or args.splits < 1:
        raise SystemExit("--splits is 1 to 6")

    def family():
        rankers = pg.create_many_filters(tol=args.tol) if args.filters == "many" else pg.create_demo_filters(tol=args.tol)
        if args.l1:
            for ranker in rankers.values():
                ranker.convergence.error_type = pg.L1
        return rankers

    timer = Timer(L)

    def run(batch):
        rankers = family()
        tuner = pg.AlgorithmSelection(rankers.values(), fraction_of_training=fractions if args.splits > 1 else fractions[0], batch=batch,
                                      min_batch_width=args.min_width)
        start = time.perf_counter()
        ms, _ = timer.time(lambda: tuner._tune(adj, signal))
        wall = (time.perf_counter() - start) * 1e3
        return ms, wall, tuner.last_selection, list(rankers)

    run(True), run(False)                                    # warm-up: every code object, every pooled block, the graph's layouts
    times = {True: dict(event=[], wall=[]), False: dict(event=[], wall=[])}
    last = {}
    for _ in range(args.reps):
        for batch in (True, False):
            ms, wall, record, names = run(batch)
            times[batch]["event"].append(ms)
            times[batch]["wall"].append(wall)
            last[batch] = record
    mixed, single = last[True], last[False]
    if mixed["selected"] != single["selected"]:
        raise SystemExit(f"the routes disagree: batch selects {names[mixed['selected']]}, one by one {names[single['selected']]}")
    worst = max(abs(a - b) for x, y in zip(mixed["rankers"], single["rankers"]) for a, b in zip(x["values"], y["values"]))
    a, b = summary(times[True]["event"]), summary(times[False]["event"])
    out = dict(tool="select_bench", scale=args.scale, edge_factor=args.ef, n=int(n), seeds=args.seeds, filters=args.filters, tol=args.tol,
               error_type="L1" if args.l1 else "default", splits=args.splits, min_batch_width=args.min_width, rankers=len(names), warmup_runs=1, reps=args.reps,
               selected=names[mixed["selected"]], routes={name: r["route"] for name, r in zip(names, mixed["rankers"])},
               mixed_calls=[dict(kind=c["kind"], width=c["width"], iterations=[min(c["iterations"]), max(c["iterations"])],
                                 loop_ms=round(c["loop_ms"], 3)) for c in mixed["mixed_calls"]],
               batch_event_ms=a, one_by_one_event_ms=b, batch_wall_ms=summary(times[True]["wall"]),
               one_by_one_wall_ms=summary(times[False]["wall"]),
               ratio_batch_over_one_by_one=round(a["median_ms"] / b["median_ms"], 4),
               spreads_disjoint=bool(a["max_ms"] < b["min_ms"] or b["max_ms"] < a["min_ms"]),
               largest_value_difference_between_routes=worst)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
