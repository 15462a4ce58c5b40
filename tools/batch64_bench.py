#!/usr/bin/env python3
"""Times ``propagate`` of a filter whose tolerance lies below fp32 eps with the f64 multi-seed loop (``f64_batch=True``,
include/pgh_batch64.h) against today's route (``f64_batch=False``: one single-vector f64 loop per column, a host look per step), on a
symmetrised RMAT graph built on the device with --columns seed sets of --seeds nodes each drawn among the nodes with edges:

  ppr        PageRank(0.85, dtype="float64")
  heat       HeatKernel(3)
  absorbing  AbsorbingWalks()            (the reference's default alpha, 1 - 1e-6)

all under error_type=L1 and --tol (1e-10).  For orientation the f32 multi-seed loop of the same filter at tol 1e-6 is timed beside them
("f32_batch"): it runs fewer iterations and is no substitute.

Every figure is the median of --reps (9) runs timed with pgh_timer_* (events on the engine's stream, host work between the launches
included) in ONE process, the routes alternating, after a warm-up run of each; min..max is the spread.  The batch's per-column iteration
counts and the largest difference between the two f64 routes' values, in f32 ulps, are reported with the times.  Needs an MI355X: there is no fallback.

    python tools/batch64_bench.py --scale 23 --columns 64 --filter ppr [--tol 1e-10] [--out profiles/batch64/...log]
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
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--filter", choices=("ppr", "heat", "absorbing"), default="ppr")
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not 1 <= args.columns <= 64:
        raise SystemExit("--columns: 1 to 64 (one multi-seed run)")

    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    from pygrank_amd.synthetic import rmat_graph
    pg.load_backend("hip")
    L.ensure_init()                                          # raises without an MI355X
    if L.entry("pgh_ppr_run_batch_f64") is None:
        raise SystemExit("the engine library lacks the entries of include/pgh_batch64.h")
    timer = Timer(L)

    adj = rmat_graph(args.scale, args.ef, seed=0, symmetrize=True, a=0.57, b=0.19, c=0.19)
    n = adj.array.shape[0]
    nodes = np.flatnonzero(np.asarray(pg.degrees(adj.array)) > 0)
    rng = np.random.default_rng(1)
    columns = []
    for _ in range(args.columns):
        p = np.zeros(n)
        p[rng.choice(nodes, size=min(args.seeds, len(nodes)), replace=False)] = 1.0
        columns.append(pg.DeviceVector.from_host(p))
    F = pg.DeviceMatrix.from_columns(columns)

    def ranker(f64_batch, tol=args.tol, **kw):
        rule = dict(error_type=pg.L1, tol=tol, max_iters=5000, f64_batch=f64_batch, **kw)
        if args.filter == "ppr":
            return pg.PageRank(0.85, **dict(dict(dtype="float64"), **rule))
        return pg.HeatKernel(3, **rule) if args.filter == "heat" else pg.AbsorbingWalks(**rule)

    def run(r, batched):
        out = r.propagate(adj, F)
        out.column(0)[0]                                     # noqa: B018 -- the result is there
        if batched is not None and (hasattr(r, "last_batches") and "f64" in r.last_batches[0][0]) != batched:
            raise SystemExit("the route under test was not taken")
        iterations = [c["iterations"] for c in r.last_batches[0]] if hasattr(r, "last_batches") else None
        return iterations, out

    routes = dict(f64_batch=lambda: run(ranker(True), True), f64_columns=lambda: run(ranker(False), False),
                  f32_batch=lambda: run(ranker(False, tol=1e-6, dtype="float32"), None))
    samples, seen = {name: [] for name in routes}, {}
    for rep in range(args.reps + 1):                         # (the first round warms every code object and pooled block up)
        for name, fn in routes.items():
            ms, seen[name] = timer.time(fn)
            if rep:
                samples[name].append(ms)
    times = {name: summary(got) for name, got in samples.items()}
    a, b = seen["f64_batch"][1].numpy(), seen["f64_columns"][1].numpy()
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    iterations = seen["f64_batch"][0]
    ratio = times["f64_batch"]["median_ms"] / times["f64_columns"]["median_ms"]
    out = dict(tool="batch64_bench", filter=args.filter, tol=args.tol, scale=args.scale, edge_factor=args.ef, n=int(n), nnz=int(adj.array.nnz),
               columns=args.columns, seeds=args.seeds, reps=args.reps,
               iterations=dict(min=min(iterations), max=max(iterations), sorted=sorted(iterations)),
               f32_batch_iterations=dict(min=min(seen["f32_batch"][0]), max=max(seen["f32_batch"][0])),
               worst_difference_f32_ulp=float(np.max(np.abs(a - b) / ulp)),
               ms_per_propagate=times, f64_batch_over_f64_columns=round(ratio, 4),
               verdict="win" if ratio < 1.0 else "LOSS")
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
