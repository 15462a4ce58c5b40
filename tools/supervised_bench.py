#!/usr/bin/env python3
"""Times Cos(known).evaluate_many(slab) and KLDivergence(known).evaluate_many(slab) two ways on a slab of 2^scale rows: random scores in
[0, 1), known scores the indicator of a random tenth of the rows.

  (a) slab:     one pgh_pair_forms call (include/pgh_supervised.h) per 64 columns: every row of the slab and of the known scores is
                read once (KLDivergence: one more pass, pgh_mat_col_abssum, for the norms);
  (b) columns:  measures._FORCE_PER_COLUMN: DeviceMatrix.columns() takes the slab apart, one strided pass per column, and every
                column is then scored with the reference's sequence of backend primitives.

Both routes are timed as tools/benchkit.py fixes it (pgh_timer_* events, ONE process, the routes alternating after a warm-up round of
each); medians and min..max over the repetitions are reported, their ratio, and the slab route's GB/s
over n * b * 4 + n * 4 bytes.  pgh_mat_col_stats (include/pgh_measure.h), which reads the same slab the same way with four
accumulators per column, is timed alongside as the yardstick of the MOMENTS pass.  The slab route counts as faster only when the two
min..max intervals are disjoint.  Needs an MI355X: there is no fallback.

    python tools/supervised_bench.py --scale 23 --columns 64 [--reps 5] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchkit import alternate, disjoint, emit, engine, over  # noqa: E402

ROOFLINE_GBPS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 repetitions")

    pg, L, timer = engine("pgh_pair_forms", what="the entry of include/pgh_supervised.h")
    from pygrank_amd import measures
    from pygrank_amd.device import DeviceMatrix, DeviceVector
    n, b = 1 << args.scale, args.columns
    rng = np.random.default_rng(1)
    slab = DeviceMatrix.empty(n, b)
    for j in range(b):
        slab.set_column(j, DeviceVector.from_host(rng.random(n, dtype=np.float32)))
    known = DeviceVector.from_host((rng.random(n) < 0.1).astype(np.float32))
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
    runs["pgh_mat_col_stats"] = col_stats
    times, values = alternate(timer, runs, args.reps)
    stream_bytes = n * b * 4 + n * 4
    out = dict(tool="supervised_bench", scale=args.scale, n=n, columns=b, reps=args.reps, stream_bytes=stream_bytes,
               roofline_gbps=ROOFLINE_GBPS)
    for name in ("Cos", "KLDivergence"):
        a, per = times[(name, "slab")], times[(name, "columns")]
        gbps = stream_bytes / (a["median_ms"] * 1e-3) / 1e9
        worst = max(abs(x - y) / abs(y) for x, y in zip(values[(name, "slab")], values[(name, "columns")]) if np.isfinite(y) and y != 0)
        out[name] = dict(slab=a, columns=per, ratio_slab_over_columns=over(a, per, 5), spreads_disjoint=disjoint(a, per),
                         slab_gbps=round(gbps, 1), slab_share_of_roofline=round(gbps / ROOFLINE_GBPS, 4),
                         largest_relative_difference_between_routes=worst)
    st = times["pgh_mat_col_stats"]
    out["pgh_mat_col_stats"] = dict(st, gbps=round(n * b * 4 / (st["median_ms"] * 1e-3) / 1e9, 1))
    emit(out, args.out)


if __name__ == "__main__":
    main()
