#!/usr/bin/env python3
"""Times the cut forms of a batch of score columns two ways, on an RMAT graph built on the device (unnormalised, as Conductance and
Density take it by default).  The scores are two hops from `--seeds` random seed nodes per column, every column divided by its
maximum: values in [0, 1], as Normalize("max") leaves a propagate result.

  (a) slab:       pgh_mat_col_stats + pgh_cut_forms (include/pgh_measure.h): a pack pass, one multi-seed pass over the adjacency per
                  slab of 64 columns, one streaming pass over the slab and its product;
  (b) per column: what the reference's Conductance.evaluate costs on the engine's single-vector entry points, column by column:
                  pgh_reduce (max), pgh_ewise_vs (max_rank - s), two pgh_spmv, four pgh_dot.  The columns are taken out of the slab
                  before the clock starts.

Both routes are timed with pgh_timer_* (events on the engine's stream, host work between the launches included) in ONE process,
alternating, after a warm-up of each; medians and min..max over the repetitions are reported, with the largest relative difference
between the two routes' Conductance values.  The slab route counts as faster only when the two min..max intervals are disjoint.
Needs an MI355X: there is no fallback.

    python tools/measure_bench.py --scale 23 --columns 64 [--reps 5] [--out FILE]
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


def conductance(forms):
    """unsupervised.py:102-111 for a directed graph from <N, s>, <N, c>, <C, s>, <C, c>."""
    internal, external = min(forms[0], forms[3]), forms[1]
    return float("inf") if external == 0 or internal == 0 else external / internal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 repetitions")

    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix, DeviceVector
    from pygrank_amd.synthetic import rmat_device_graph
    pg.load_backend("hip")
    L.ensure_init()                                          # raises without an MI355X
    stats_fn, forms_fn = L.entry("pgh_mat_col_stats"), L.entry("pgh_cut_forms")
    if stats_fn is None or forms_fn is None:
        raise SystemExit("the engine library lacks the entries of include/pgh_measure.h")
    lib = L.lib()
    g = rmat_device_graph(args.scale, args.ef, seed=0, normalization="none")
    n, b = g.shape[0], args.columns
    candidates = np.flatnonzero(np.asarray(g.degrees()) > 0)
    rng = np.random.default_rng(1)
    seeds = DeviceMatrix.empty(n, b)
    for j in range(b):
        p = np.zeros(n)
        p[rng.choice(candidates, size=min(args.seeds, len(candidates)), replace=False)] = 1.0
        seeds.set_column(j, DeviceVector.from_host(p))
    hops = g.conv(g.conv(seeds)) if b <= 64 else None
    if hops is None:
        raise SystemExit("at most 64 columns")
    top = np.empty((b, 4))
    L.check(stats_fn(hops._h, top.ctypes.data_as(C.c_void_p)))
    scores = hops.div_cols(np.where(top[:, 2] > 0, top[:, 2], 1.0))
    del seeds, hops
    columns = scores.columns()
    max_rank = 1.0
    timer = Timer(L)

    def slab():
        stats, forms = np.empty((b, 4)), np.empty((b, 4))
        L.check(stats_fn(scores._h, stats.ctypes.data_as(C.c_void_p)))
        if np.any(stats[:, 2] > max_rank):
            raise SystemExit("a column above max_rank")
        L.check(forms_fn(g._h, scores._h, None, max_rank, L.CUT_ALL, forms.ctypes.data_as(C.c_void_p)))
        return [conductance(row) for row in forms]

    def slab_internal():
        stats, forms = np.empty((b, 4)), np.empty((b, 4))
        L.check(stats_fn(scores._h, stats.ctypes.data_as(C.c_void_p)))
        L.check(forms_fn(g._h, scores._h, None, max_rank, L.CUT_INTERNAL, forms.ctypes.data_as(C.c_void_p)))
        return [row[0] / (st[0] ** 2 - st[1]) for row, st in zip(forms, stats)]

    rest, near, far = DeviceVector.empty(n), DeviceVector.empty(n), DeviceVector.empty(n)

    def per_column():
        out, value = [], C.c_double()

        def dot(u, v):
            L.check(lib.pgh_dot(u._h, v._h, C.byref(value)))
            return value.value
        for s in columns:
            L.check(lib.pgh_reduce(L.MAX, s._h, C.byref(value)))
            if value.value > max_rank:
                raise SystemExit("a column above max_rank")
            L.check(lib.pgh_ewise_vs(L.SUB, s._h, max_rank, 1, rest._h))
            L.check(lib.pgh_spmv(g._h, s._h, near._h))
            L.check(lib.pgh_spmv(g._h, rest._h, far._h))
            out.append(conductance([dot(near, s), dot(near, rest), dot(far, s), dot(far, rest)]))
        return out

    slab(), slab_internal(), per_column()                     # warm-up: the multi-seed image, the pool's blocks, every code object
    a_ms, d_ms, b_ms, worst = [], [], [], 0.0
    for _ in range(args.reps):
        ms, got_a = timer.time(slab)
        a_ms.append(ms)
        ms, got_b = timer.time(per_column)
        b_ms.append(ms)
        ms, _ = timer.time(slab_internal)
        d_ms.append(ms)
        worst = max(worst, max(abs(x - y) / abs(y) for x, y in zip(got_a, got_b) if np.isfinite(y) and y != 0))
    a, d, per = summary(a_ms), summary(d_ms), summary(b_ms)
    chunks = -(-b // 32)
    width = 2 * ((min(b, 32) + 3) & ~3)
    # bytes from shapes: the statistics read the slab; per chunk the pack reads its columns and writes X, the forms read X and Y
    slab_bytes = 4 * n * b + chunks * (4 * n * min(b, 32) + 3 * 4 * n * width)
    info = g.info()
    out = dict(tool="measure_bench", scale=args.scale, edge_factor=args.ef, n=int(n), nnz=int(info["nnz"]), columns=b, reps=args.reps,
               seeds_per_column=args.seeds, slab_conductance=a, slab_density=d, per_column_conductance=per,
               graph_passes=dict(slab=chunks, per_column=2 * b),
               ratio_slab_over_per_column=round(a["median_ms"] / per["median_ms"], 4),
               spreads_disjoint=bool(a["max_ms"] < per["min_ms"] or per["max_ms"] < a["min_ms"]),
               slab_stream_bytes_outside_the_graph_pass=int(slab_bytes),
               largest_relative_difference_between_routes=worst, graph_format=g.format())
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
