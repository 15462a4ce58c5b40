#!/usr/bin/env python3
"""Times Cos(known).evaluate_many(slab) and KLDivergence(known).evaluate_many(slab) two ways on a slab of 2^scale rows: random scores in
[0, 1), known scores the indicator of a random tenth of the rows.

  (a) slab:     one pgh_pair_forms call (include/pgh_supervised.h) per 64 columns: every row of the slab and of the known scores is
                read once (KLDivergence: one more pass, pgh_mat_col_abssum, for the norms);
  (b) columns:  measures._FORCE_PER_COLUMN: DeviceMatrix.columns() takes the slab apart, one strided pass per column, and every
                column is then scored with the reference's sequence of backend primitives.

Both routes are timed with pgh_timer_* (events on the engine's stream, host work between the launches included) in ONE process,
alternating, after a warm-up of each; medians and min..max over the repetitions are reported, their ratio, and the slab route's GB/s
over n * b * 4 + n * 4 bytes.  pgh_mat_col_stats (include/pgh_measure.h), which reads the same slab the same way with four
accumulators per column, is timed alongside as the yardstick of the MOMENTS pass.  The slab route counts as faster only when the two
min..max intervals are disjoint.  Needs an MI355X: there is no fallback.

    python tools/supervised_bench.py --scale 23 --columns 64 [--reps 5] [--out FILE]
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


def summary(samples):
    return dict(median_ms=round(statistics.median(samples), 4), min_ms=round(min(samples), 4), max_ms=round(max(samples), 4),
                samples=len(samples))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
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
    if L.entry("pgh_pair_forms") is None:
        raise SystemExit("the engine library lacks the entry of include/pgh_supervised.h")
    n, b = 1 << args.scale, args.columns
    rng = np.random.default_rng(1)
    slab = DeviceMatrix.empty(n, b)
    for j in range(b):
        slab.set_column(j, DeviceVector.from_host(rng.random(n, dtype=np.float32)))
    known = DeviceVector.from_host((rng.random(n) < 0.1).astype(np.float32))
    timer = Timer(L)
    stats_fn = L.entry("pgh_mat_col_stats")

    def route(cls, per_column):
        def run():
            measures._FORCE_PER_COLUMN = per_column
            try:
                measure = cls(known)
                values = measure.evaluate_many(slab)
            finally:
                measures._FORCE_PER_COLUMN = False
            assert measure.last_route == ("columns" if per_column else "slab")
            return values
        return run

    def col_stats():
        stats = np.empty((b, 4))
        L.check(stats_fn(slab._h, stats.ctypes.data_as(C.c_void_p)))
        return stats

    runs = {(name, label): route(getattr(pg, name), label == "columns") for name in ("Cos", "KLDivergence") for label in ("slab", "columns")}
    for run in runs.values():                                # warm-up: the pool's blocks, every code object
        run()
    col_stats()
    samples, values, stats_ms = {key: [] for key in runs}, {}, []
    for _ in range(args.reps):
        for key, run in runs.items():
            ms, values[key] = timer.time(run)
            samples[key].append(ms)
        stats_ms.append(timer.time(col_stats)[0])
    stream_bytes = n * b * 4 + n * 4
    out = dict(tool="supervised_bench", scale=args.scale, n=n, columns=b, reps=args.reps, stream_bytes=stream_bytes,
               roofline_gbps=ROOFLINE_GBPS)
    for name in ("Cos", "KLDivergence"):
        a, per = summary(samples[(name, "slab")]), summary(samples[(name, "columns")])
        gbps = stream_bytes / (a["median_ms"] * 1e-3) / 1e9
        worst = max(abs(x - y) / abs(y) for x, y in zip(values[(name, "slab")], values[(name, "columns")]) if np.isfinite(y) and y != 0)
        out[name] = dict(slab=a, columns=per, ratio_slab_over_columns=round(a["median_ms"] / per["median_ms"], 5),
                         spreads_disjoint=bool(a["max_ms"] < per["min_ms"] or per["max_ms"] < a["min_ms"]),
                         slab_gbps=round(gbps, 1), slab_share_of_roofline=round(gbps / ROOFLINE_GBPS, 4),
                         largest_relative_difference_between_routes=worst)
    st = summary(stats_ms)
    out["pgh_mat_col_stats"] = dict(st, gbps=round(n * b * 4 / (st["median_ms"] * 1e-3) / 1e9, 1))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
