#!/usr/bin/env python3
"""Times a multi-seed run that retires its converged columns (include/pgh_retire.h) against the plain batch and the columns one by one,
on a symmetrised RMAT graph built on the device with --columns seed sets of --seeds nodes each drawn among the nodes with edges, around
PageRank(0.9, error_type=L1, tol=1e-6) -- the setting of tools/oversample_bench.py's inner run:

  propagate  ms per ``propagate`` with retire on ("retire"), with retire off ("plain") and with one ``rank()`` per column ("ranks"),
             with the columns' iteration counts, the retiring run's stages and its column_steps beside the plain run's;
  stages     (--stages) ms per step of every stage: the retiring run is timed once more per prefix of the level list -- no level, the
             first level, the first two ... -- and the time a stage adds over the prefix before it, its narrowing included, is divided
             by the steps it runs.  A stage paid when its ms per step lies below that of the stage before it.

--mixed: one alpha per column, from 0.5 to 0.97 (pgh_ppr_run_batch_mixed and its retiring sibling through the C-ABI; "ranks": one
PageRank(alpha_j).rank per column).  --levels: a comma-separated level list instead of the default 32,16,8,4.

Every figure is the median of --reps (9) runs timed with pgh_timer_* (events on the engine's stream, host work between the launches
included) in ONE process, the routes alternating, after a warm-up run of each; min..max is the spread.  Needs an MI355X: there is no
fallback.

    python tools/retire_bench.py --scale 23 --columns 64 [--mixed] [--levels 48,20,12,4] [--stages] [--out profiles/retire/...log]
"""
import argparse
import ctypes as C
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--levels", default=None)
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not 1 <= args.columns <= 64:
        raise SystemExit("--columns: 1 to 64 (one multi-seed run)")
    levels = [32, 16, 8, 4] if args.levels is None else [int(v) for v in args.levels.split(",") if v]

    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    from pygrank_amd.synthetic import rmat_graph
    pg.load_backend("hip")
    L.ensure_init()                                          # raises without an MI355X
    if L.entry("pgh_ppr_run_batch_mixed_retire" if args.mixed else "pgh_ppr_run_batch_retire") is None:
        raise SystemExit("the engine library lacks the entries of include/pgh_retire.h")
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
    signals = [pg.to_signal(adj, column) for column in columns]
    alphas = [float(a) for a in np.linspace(0.5, 0.97, args.columns)] if args.mixed else [0.9] * args.columns

    def ranker(alpha=0.9, retire=False):
        return pg.PageRank(alpha, error_type=pg.L1, tol=1e-6, max_iters=1000, retire=retire)

    def batch(retire):
        """One multi-seed run -> (per-column iterations, the report's stages or None)."""
        if not args.mixed:
            r = ranker(retire=retire)
            r.propagate(adj, F).column(0)[0]                 # noqa: B018 -- the result is there
            record = r.last_batches[0]
            return [c["iterations"] for c in record], record[0].get("stages")
        first = ranker()
        g = first._batch_graph(adj, (), {})
        norms = F.col_abssum()
        P, R = F.div_cols(norms), pg.DeviceMatrix.empty(F.n, F.b)
        cfg = first._loop_cfg(0.0, True, 1.0)
        cfg.start_from_p = 1
        results, scales = (L.LoopResult * F.b)(), (C.c_double * F.b)(*[float(v) for v in norms])
        head = (g._h, P._h, R._h, C.byref(cfg), (C.c_double * F.b)(*alphas), scales, results)
        report = L.RetireReport()
        if L.retire_on(retire):
            arr, count = L.retire_levels(retire)
            L.check(L.entry("pgh_ppr_run_batch_mixed_retire")(*head, arr, count, C.byref(report)))
        else:
            L.check(L.entry("pgh_ppr_run_batch_mixed")(*head))
        R.column(0)[0]                                       # noqa: B018
        return [r.iterations for r in results], (L.retire_stages(report) if L.retire_on(retire) else None)

    def ranks():
        out = [ranker(alpha).rank(adj, signal) for alpha, signal in zip(alphas, signals)]
        out[-1].np[0]                                        # noqa: B018
        return None, None

    routes = dict(retire=lambda: batch(list(levels)), plain=lambda: batch(False), ranks=ranks)
    samples, seen = {name: [] for name in routes}, {}
    for rep in range(args.reps + 1):                         # (the first round warms every code object and pooled block up)
        for name, run in routes.items():
            ms, seen[name] = timer.time(run)
            if rep:
                samples[name].append(ms)
    propagate = {name: summary(got) for name, got in samples.items()}
    iterations, stages = seen["retire"]
    plain_iterations = seen["plain"][0]
    executed = max(iterations) - 1
    out = dict(tool="retire_bench", scale=args.scale, edge_factor=args.ef, n=int(n), nnz=int(adj.array.nnz), columns=args.columns,
               seeds=args.seeds, mixed=args.mixed, levels=levels, reps=args.reps,
               iterations=dict(min=min(iterations), max=max(iterations), sorted=sorted(iterations)),
               iterations_differ_from_plain=sum(1 for a, b in zip(iterations, plain_iterations) if a != b),
               stages=stages, column_steps=dict(retire=stages["column_steps"], plain=stages["ld"][0] * (max(plain_iterations) - 1)),
               ms_per_propagate=propagate,
               retire_over_plain=round(propagate["retire"]["median_ms"] / propagate["plain"]["median_ms"], 4),
               retire_over_ranks=round(propagate["retire"]["median_ms"] / propagate["ranks"]["median_ms"], 4),
               plain_over_ranks=round(propagate["plain"]["median_ms"] / propagate["ranks"]["median_ms"], 4))

    if args.stages:
        # prefix i of the levels: the run narrows through its first i levels only; what prefix i costs over prefix i - 1 is what the
        # deepest of its stages costs over staying in the stage before
        prefixes = [levels[:i] for i in range(len(levels) + 1)]
        samples, reports = [[] for _ in prefixes], [None] * len(prefixes)
        for rep in range(args.reps + 1):
            for i, prefix in enumerate(prefixes):
                ms, (_, reports[i]) = timer.time(lambda: batch(list(prefix)))
                if rep:
                    samples[i].append(ms)
        medians = [summary(got) for got in samples]
        per_stage, wide_step = [], medians[0]["median_ms"] / max(executed, 1)
        per_stage.append(dict(levels=[], ld=reports[0]["ld"][0], steps=executed, ms_per_step=round(wide_step, 4), run=medians[0]))
        for i in range(1, len(prefixes)):
            here, before = reports[i], reports[i - 1]
            if len(here["ld"]) == len(before["ld"]):          # the level was never reached, or skipped by a deeper fall
                per_stage.append(dict(levels=prefixes[i], ld=None, steps=0, ms_per_step=None, run=medians[i]))
                continue
            first = here["first_step"][-1]
            steps = executed - first + 1
            # the steps from `first` on ran in the stage before under prefix i - 1: at that stage's ms per step
            stayed = next(s["ms_per_step"] for s in reversed(per_stage) if s["ms_per_step"] is not None)
            moved = stayed + (medians[i]["median_ms"] - medians[i - 1]["median_ms"]) / max(steps, 1)
            per_stage.append(dict(levels=prefixes[i], ld=here["ld"][-1], live=here["live"][-1], first_step=first, steps=steps,
                                  ms_per_step=round(moved, 4), ms_per_step_before=round(stayed, 4), paid=bool(moved < stayed),
                                  run=medians[i]))
        out["per_stage"] = per_stage

    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
