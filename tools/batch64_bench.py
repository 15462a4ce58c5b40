#!/usr/bin/env python3
"""Times ``propagate`` of a filter whose tolerance lies below fp32 eps with the f64 multi-seed loop (``f64_batch=True``,
include/pgh_batch64.h) against today's route (``f64_batch=False``: one single-vector f64 loop per column, a host look per step), on a
symmetrised RMAT graph built on the device with --columns seed sets of --seeds nodes each drawn among the nodes with edges:

  ppr        PageRank(0.85, dtype="float64")
  heat       HeatKernel(3)
  absorbing  AbsorbingWalks()            (the reference's default alpha, 1 - 1e-6)

all under error_type=L1 and --tol (1e-10).  For orientation the f32 multi-seed loop of the same filter at tol 1e-6 is timed beside them
("f32_batch"): it runs fewer iterations and is no substitute.

Every figure is the median of --reps (9) runs timed as tools/benchkit.py fixes it (pgh_timer_* events, ONE process, the routes
alternating after a warm-up round of each); min..max is the spread.  The batch's per-column iteration
counts and the largest difference between the two f64 routes' values, in f32 ulps, are reported with the times.  Needs an MI355X: there is no fallback.

--retire [levels ...] times the retiring f64 batch (``f64_retire=``, include/pgh_retire64.h; no levels: the engine's default list) as a
third f64 route ("f64_retire") beside the two; --stages prints its report (stages, slab columns streamed against the plain batch's)
to stderr; --routes names the routes to time (default: all).  PGH_MM64_PAIR=0 in the environment keeps the four-lane product in the
ld == 2 stages.

--form chebyshev (with --filter heat) times the "chebyshev" form: its f64 batch (include/pgh_cheb64.h) against one single-vector f64
loop per column.  That form has no f32 multi-seed loop, so no "f32_batch" is timed.  For --filter heat, either form,
"f64_batch_ms_per_step" is the batch's median divided by its device steps (the most iterations of a column, less the two that need
no product).

    python tools/batch64_bench.py --scale 23 --columns 64 --filter ppr [--tol 1e-10] [--retire] [--stages] [--out profiles/batch64/...log]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchkit import alternate, emit, engine, nodes_with_edges, over, rmat, seed_columns  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--filter", choices=("ppr", "heat", "absorbing"), default="ppr")
    ap.add_argument("--form", choices=("taylor", "chebyshev"), default="taylor")
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--retire", type=int, nargs="*", default=None, metavar="LEVEL")
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--routes", nargs="+", default=None, choices=("f64_batch", "f64_columns", "f32_batch", "f64_retire"))
    args = ap.parse_args()
    if not 1 <= args.columns <= 64:
        raise SystemExit("--columns: 1 to 64 (one multi-seed run)")
    cheb = args.form == "chebyshev"
    if cheb and args.filter != "heat":
        raise SystemExit("--form chebyshev: a closed-form filter (--filter heat)")

    pg, L, timer = engine("pgh_ppr_run_batch_f64", what="the entries of include/pgh_batch64.h")
    if args.retire is not None and (args.filter == "heat" or L.entry("pgh_ppr_run_batch_f64_retire") is None):
        raise SystemExit("--retire: the recursive filters, and a library with the entries of include/pgh_retire64.h")
    if cheb and L.entry("pgh_cheb_run_batch_f64") is None:
        raise SystemExit("the engine library lacks the entry of include/pgh_cheb64.h")

    adj = rmat(args, symmetrize=True)
    n = adj.array.shape[0]
    columns = seed_columns(pg, n, nodes_with_edges(pg, adj), args.columns, args.seeds, np.random.default_rng(1))
    F = pg.DeviceMatrix.from_columns(columns)                 # (the columns stay allocated: part of the pool's state under the timed runs)

    def ranker(f64_batch, tol=args.tol, **kw):
        rule = dict(error_type=pg.L1, tol=tol, max_iters=5000, f64_batch=f64_batch, **kw)
        if args.filter == "ppr":
            return pg.PageRank(0.85, **dict(dict(dtype="float64"), **rule))
        if args.filter == "heat":
            return pg.HeatKernel(3, **dict(rule, coefficient_type=args.form))
        return pg.AbsorbingWalks(**rule)

    def run(r, batched):
        out = r.propagate(adj, F)
        out.column(0)[0]                                     # noqa: B018 -- the result is there
        if batched is not None and (hasattr(r, "last_batches") and "f64" in r.last_batches[0][0]) != batched:
            raise SystemExit("the route under test was not taken")
        iterations = [c["iterations"] for c in r.last_batches[0]] if hasattr(r, "last_batches") else None
        return iterations, out, (r.last_batches[0][0].get("stages") if iterations else None)

    routes = dict(f64_batch=lambda: run(ranker(True), True), f64_columns=lambda: run(ranker(False), False),
                  f32_batch=lambda: run(ranker(False, tol=1e-6, dtype="float32"), None))
    if cheb:
        del routes["f32_batch"]
    if args.retire is not None:
        routes["f64_retire"] = lambda: run(ranker(True, f64_retire=args.retire or True), True)
    if args.routes:
        routes = {name: fn for name, fn in routes.items() if name in args.routes}
    times, seen = alternate(timer, routes, args.reps)
    out = dict(tool="batch64_bench", filter=args.filter, **(dict(form=args.form) if cheb else {}), tol=args.tol, scale=args.scale, edge_factor=args.ef, n=int(n), nnz=int(adj.array.nnz),
               columns=args.columns, seeds=args.seeds, reps=args.reps)

    def worst_ulp(x, y):
        x, y = seen[x][1].numpy(), seen[y][1].numpy()
        return float(np.max(np.abs(x - y) / np.spacing(np.maximum(np.abs(x), np.abs(y)).astype(np.float32)).astype(np.float64)))
    batch = next((name for name in ("f64_batch", "f64_retire") if name in seen), None)
    if batch is not None:
        iterations = seen[batch][0]
        out["iterations"] = dict(min=min(iterations), max=max(iterations), sorted=sorted(iterations))
    if "f32_batch" in seen:
        out["f32_batch_iterations"] = dict(min=min(seen["f32_batch"][0]), max=max(seen["f32_batch"][0]))
    both = "f64_batch" in seen and "f64_columns" in seen                 # (every key of a run of all routes, in the order it always had)
    if both:
        out["worst_difference_f32_ulp"] = worst_ulp("f64_batch", "f64_columns")
    out["ms_per_propagate"] = times
    if both:
        ratio = times["f64_batch"]["median_ms"] / times["f64_columns"]["median_ms"]
        out.update(f64_batch_over_f64_columns=round(ratio, 4), verdict="win" if ratio < 1.0 else "LOSS")
    if args.filter == "heat" and "f64_batch" in seen and max(seen["f64_batch"][0]) > 2:
        out["f64_batch_ms_per_step"] = round(times["f64_batch"]["median_ms"] / (max(seen["f64_batch"][0]) - 2), 4)
    if "f64_retire" in seen:
        stages = seen["f64_retire"][2]
        out.update(retire_levels=args.retire or "default", pair=os.environ.get("PGH_MM64_PAIR", "1") != "0", stages=stages)
        for other in ("f64_batch", "f64_columns"):
            if other in seen:
                out["f64_retire_over_" + other] = over(times["f64_retire"], times[other])
                out["f64_retire_worst_difference_from_%s_f32_ulp" % other] = worst_ulp("f64_retire", other)
        if "f64_batch" in seen:
            out["same_iterations_as_f64_batch"] = seen["f64_retire"][0] == seen["f64_batch"][0]
            out["plain_column_steps"] = ((args.columns + 1) & ~1) * (max(seen["f64_batch"][0]) - 1)
        if args.stages:
            for ld, live, first in zip(stages["ld"], stages["live"], stages["first_step"]):
                print("stage: ld %2d, %2d live columns, from step %d" % (ld, live, first), file=sys.stderr)
            print("slab columns streamed: %d (the plain f64 batch: %s)" % (stages["column_steps"], out.get("plain_column_steps", "not run")),
                  file=sys.stderr)
    emit(out, args.out)


if __name__ == "__main__":
    main()
