#!/usr/bin/env python3
"""Times NDCG(known).evaluate_many(slab) or SpearmanCorrelation(known).evaluate_many(slab) on a slab of 2^scale rows of random scores in
[0, 1) (every fourth column on a grid of 1/64: ties), against known scores in {0, 0.25, 0.5, 1} that are non-zero on --relevant random
rows:

  (a) slab:     include/pgh_rank.h through one plan, 64 columns per call.  NDCG: the streaming count (at most 8192 relevant rows) --
                every kept element of the slab is read once; and, timed apart, the same entry forced onto its sorted route (one radix
                sort per column).  Spearman: one radix sort per column.
  (b) columns:  measures._FORCE_PER_COLUMN: DeviceMatrix.columns() takes the slab apart, one strided pass per column, and every column
                is scored by backend primitives (NDCG: two ordinals() sorts and a masked sum; Spearman: both vectors are downloaded
                and ranked by numpy on the host).  --baseline-columns C scores only the first C columns on this route (the host ranking
                of 2^23 rows takes seconds per column); both routes are also reported per column.

All are timed with pgh_timer_* (events on the engine's stream, host work between the launches included) in ONE process, alternating,
after a warm-up of each; medians and min..max over the repetitions are reported.  pgh_mat_col_stats (include/pgh_measure.h), the plain
read of the same slab, is timed alongside as the yardstick of the streaming pass.  A route counts as faster only when the two min..max
intervals (per column) are disjoint.  Needs an MI355X: there is no fallback.

    python tools/ranking_bench.py --scale 23 --columns 64 [--relevant 100] [--measure ndcg|spearman] [--baseline-columns C] [--reps 9] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOFLINE_GBPS = 8000.0


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


def summary(samples, columns):
    median = statistics.median(samples)
    return dict(median_ms=round(median, 4), min_ms=round(min(samples), 4), max_ms=round(max(samples), 4), samples=len(samples),
                columns=columns, median_ms_per_column=round(median / columns, 5), min_ms_per_column=round(min(samples) / columns, 5),
                max_ms_per_column=round(max(samples) / columns, 5))


def disjoint(a, b):
    return bool(a["max_ms_per_column"] < b["min_ms_per_column"] or b["max_ms_per_column"] < a["min_ms_per_column"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--relevant", type=int, default=100)
    ap.add_argument("--measure", choices=["ndcg", "spearman"], default="ndcg")
    ap.add_argument("--baseline-columns", type=int, default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 repetitions")

    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    from pygrank_amd import measures
    from pygrank_amd.device import DeviceMatrix, DeviceVector
    pg.load_backend("hip")
    L.ensure_init()                                          # raises without an MI355X
    if any(L.entry(name) is None for name in L.RANK_SIGNATURES):
        raise SystemExit("the engine library lacks the entries of include/pgh_rank.h")
    n, b = 1 << args.scale, args.columns
    few = b if args.baseline_columns is None else min(b, args.baseline_columns)
    rng = np.random.default_rng(1)
    slab = DeviceMatrix.empty(n, b)
    for j in range(b):
        column = rng.random(n, dtype=np.float32)
        slab.set_column(j, DeviceVector.from_host(np.round(column * 64) / 64 if j % 4 == 3 else column))
    head = slab if few == b else slab.get_cols(0, few)
    host_known = np.zeros(n, dtype=np.float32)
    host_known[rng.choice(n, min(args.relevant, n), replace=False)] = rng.choice([0.25, 0.5, 1.0], min(args.relevant, n))
    known = DeviceVector.from_host(host_known)
    timer = Timer(L)
    stats_fn = L.entry("pgh_mat_col_stats")
    k = 1000 if args.measure == "ndcg" else None
    measure = pg.NDCG(known, k=k) if args.measure == "ndcg" else pg.SpearmanCorrelation(known)

    def slab_route():
        values = measure.evaluate_many(slab)
        assert measure.last_route == "slab"
        return values

    def columns_route():
        measures._FORCE_PER_COLUMN = True
        try:
            values = measure.evaluate_many(head)
        finally:
            measures._FORCE_PER_COLUMN = False
        assert measure.last_route == "columns"
        return values

    def sorted_route():
        plan = measure._plan_cache[4]
        out = []
        for _, part in slab.chunks():
            dcg, idcg = (C.c_double * part.b)(), C.c_double()
            L.check(L.entry("pgh_ndcg")(part._h, plan._h, k, L.RANK_SORTED, dcg, C.byref(idcg)))
            out.extend(float(v) / idcg.value for v in dcg)
        return out

    def col_stats():
        for _, part in slab.chunks():
            stats = np.empty((part.b, 4))
            L.check(stats_fn(part._h, stats.ctypes.data_as(C.c_void_p)))
        return stats

    runs = dict(slab=(slab_route, b), columns=(columns_route, few), pgh_mat_col_stats=(col_stats, b))
    if args.measure == "ndcg":
        runs["slab_sorted_route"] = (sorted_route, b)
    for run, _ in runs.values():                             # warm-up: the plan, the pool's blocks, every code object
        run()
    samples, values = {key: [] for key in runs}, {}
    for _ in range(args.reps):
        for key, (run, _) in runs.items():
            ms, values[key] = timer.time(run)
            samples[key].append(ms)
    plan = measure._plan_cache[4]
    stream_bytes = n * b * 4 + n
    out = dict(tool="ranking_bench", measure=args.measure, scale=args.scale, n=n, columns=b, baseline_columns=few, relevant=plan.num_relevant,
               k=k, reps=args.reps, stream_bytes=stream_bytes, roofline_gbps=ROOFLINE_GBPS)
    for key, (_, width) in runs.items():
        out[key] = summary(samples[key], width)
    gbps = stream_bytes / (out["slab"]["median_ms"] * 1e-3) / 1e9
    out["slab"].update(gbps=round(gbps, 1), share_of_roofline=round(gbps / ROOFLINE_GBPS, 4))
    out["pgh_mat_col_stats"]["gbps"] = round(n * b * 4 / (out["pgh_mat_col_stats"]["median_ms"] * 1e-3) / 1e9, 1)
    out["slab_over_columns_per_column"] = round(out["slab"]["median_ms_per_column"] / out["columns"]["median_ms_per_column"], 5)
    out["spreads_disjoint"] = disjoint(out["slab"], out["columns"])
    out["slab_over_col_stats"] = round(out["slab"]["median_ms"] / out["pgh_mat_col_stats"]["median_ms"], 3)
    if args.measure == "ndcg":
        out["streaming_over_sorted"] = round(out["slab"]["median_ms"] / out["slab_sorted_route"]["median_ms"], 5)
        out["streaming_sorted_spreads_disjoint"] = disjoint(out["slab"], out["slab_sorted_route"])
        out["largest_difference_streaming_sorted"] = max(abs(x - y) for x, y in zip(values["slab"], values["slab_sorted_route"]))
    pairs = [(x, y) for x, y in zip(values["slab"][:few], values["columns"]) if np.isfinite(x) and np.isfinite(y)]
    out["largest_difference_between_routes"] = max((abs(x - y) for x, y in pairs), default=None)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
