#!/usr/bin/env python3
"""Times HopTuner and the Arnoldi step on a symmetrised RMAT graph built on the device (normalization="symmetric"), 100 seeds drawn as
bench.py draws them:

  tune      ms per HopTuner.tune with --params hop weights, --basis and --measure: fused and fused=False (the reference's route in
            backend primitives), with the products and slab passes each reports;
  sweep     ms per hop sweep alone (the [n, K] power slabs of both halves): HopTuner's own, two single-vector steps per hop
            ("steps"), against one 2-wide pgh_spmm per hop for both halves ("spmm", `sweep_spmm` below) -- the comparison that
            decided the tuner's sweep; the logs of profiles/hop/ were taken while the tuner still had both, so they also hold a
            "fused_spmm" row under ms_per_tune;
  arnoldi   ms per arnoldi_iteration of 10 and of 20 columns, fused (include/pgh_arnoldi.h) and in primitives, and per step
            (= run / (columns - 1): the way in, the division of the columns and the way out amortised over the steps);
  parameter_tuner   for orientation, ONE ParameterTuner.tune on the same graph and seeds (its default search: hundreds of probes).

Every figure but the last is the median of --reps (9) runs timed with pgh_timer_* (events on the engine's stream, host work between the
launches included) in ONE process, the routes alternating, after a warm-up run of each; min..max is the spread, and
`spreads_disjoint` says whether the spreads of the two routes compared separate.  Needs an MI355X: there is no fallback.

    python tools/hop_bench.py --scale 23 --params 20 [--basis krylov|arnoldi] [--measure cos|auc] [--out profiles/hop/hop_bench_scale23_k20_krylov_cos.log]
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tune_bench import Timer, summary  # noqa: E402


def disjoint(a, b):
    return bool(a["max_ms"] < b["min_ms"] or b["max_ms"] < a["min_ms"])


def alternate(timer, routes, reps):
    """{name: summary} of `reps` timed runs of every route, the routes alternating, after one warm-up round; the last value of each."""
    samples, last = {name: [] for name in routes}, {}
    for rep in range(reps + 1):                              # (the first round warms every code object and pooled block up)
        for name, once in routes.items():
            ms, last[name] = timer.time(once)
            if rep:
                samples[name].append(ms)
    return {name: summary(got) for name, got in samples.items()}, last


def sweep_spmm(pg, g, halves, hops):
    """The sweep HopTuner does NOT use: one multi-seed pass of two columns per hop, its columns copied into the halves' slabs."""
    slabs = [pg.DeviceMatrix.empty(len(p), hops) for p in halves]
    for slab, p in zip(slabs, halves):
        slab.set_column(0, p)
    both = pg.DeviceMatrix.from_columns(halves)
    for i in range(1, hops):
        both = g.conv(both)
        for h, slab in enumerate(slabs):
            slab.set_column(i, both.column(h))
    return slabs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--params", type=int, default=20)
    ap.add_argument("--basis", default="krylov", choices=["krylov", "arnoldi"])
    ap.add_argument("--measure", default="cos", choices=["cos", "auc"])
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--no-parameter-tuner", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    from pygrank_amd import krylov
    from pygrank_amd.synthetic import rmat_graph
    pg.load_backend("hip")
    L.ensure_init()                                          # raises without an MI355X
    if L.entry("pgh_basis_dots") is None or L.entry("pgh_arnoldi_close") is None:
        raise SystemExit("the engine library lacks the entries of include/pgh_arnoldi.h")
    warnings.simplefilter("ignore")
    timer = Timer(L)

    adj = rmat_graph(args.scale, args.ef, seed=0, normalization="symmetric", symmetrize=True, a=0.57, b=0.19, c=0.19)
    n = adj.array.shape[0]
    rng = np.random.default_rng(1)
    nodes = np.flatnonzero(np.asarray(pg.degrees(adj.array)) > 0)
    p = np.zeros(n)
    p[np.sort(rng.choice(nodes, size=min(args.seeds, len(nodes)), replace=False))] = 1.0
    signal = pg.to_signal(adj, p)
    measure = pg.Cos if args.measure == "cos" else pg.AUC

    # ---- a whole tune
    def tune(fused):
        tuner = pg.HopTuner(measure=measure, basis=args.basis, num_parameters=args.params, fused=fused)
        tuner.tune(adj, signal)
        L.check(L.lib().pgh_sync())
        return tuner
    tune_ms, tuners = alternate(timer, dict(primitive=lambda: tune(False), fused=lambda: tune(True)), args.reps)
    for name, tuner in tuners.items():
        stats = tuner.last_tune
        if (name != "primitive") != (stats["route"] == "fused"):
            raise SystemExit(f"{name} took the {stats['route']} route: {stats}")
        tune_ms[name].update(route=stats["route"], sweep=stats["sweep"], products=stats["products"], slab_passes=stats["slab_passes"])

    # ---- the hop sweep alone
    probe = pg.HopTuner(num_parameters=args.params)
    M = probe.ranker_generator([None] * args.params).preprocessor(adj)
    g = krylov._device_graph(M)
    training, _ = pg.split(pg.to_signal(signal, signal.np), 0.8)
    halves = [half.np for half in pg.split(training, 0.5)]

    def sweep(route):
        slabs = sweep_spmm(pg, g, halves, args.params) if route == "spmm" else \
            probe._sweep_powers(g, halves, args.params, probe._fresh_stats())
        L.check(L.lib().pgh_sync())
        return slabs
    sweep_ms, slabs = alternate(timer, dict(spmm=lambda: sweep("spmm"), steps=lambda: sweep("steps")), args.reps)
    worst = max(float(np.abs(a.numpy() - b.numpy()).max()) for a, b in zip(slabs["spmm"], slabs["steps"])) if args.scale <= 20 else None
    del slabs

    # ---- arnoldi_iteration
    arnoldi = {}
    for columns in (10, 20):
        def run(fused, columns=columns):
            out = krylov.arnoldi_run(M, signal.np, columns, fused)
            L.check(L.lib().pgh_sync())
            return out[2]
        got, took = alternate(timer, dict(fused=lambda: run(True), primitive=lambda: run(False)), args.reps)
        if took != dict(fused="fused", primitive="primitive"):
            raise SystemExit(f"arnoldi_iteration took {took}")
        arnoldi[str(columns)] = dict(ms_per_run=got, ms_per_step={name: round(s["median_ms"] / (columns - 1), 4) for name, s in got.items()},
                                     fused_over_primitive=round(got["fused"]["median_ms"] / got["primitive"]["median_ms"], 4),
                                     spreads_disjoint=disjoint(got["fused"], got["primitive"]))

    # ---- for orientation: one ParameterTuner.tune
    parameter_tuner = None
    if not args.no_parameter_tuner:
        def search():
            tuner = pg.ParameterTuner(verbose=False)
            tuner.tune(adj, signal)
            L.check(L.lib().pgh_sync())
            return tuner
        ms, tuner = timer.time(search)
        parameter_tuner = dict(ms=round(ms, 2), runs=1, **tuner.last_tune)

    out = dict(tool="hop_bench", scale=args.scale, edge_factor=args.ef, n=int(n), nnz=int(adj.array.nnz), seeds=args.seeds, params=args.params,
               basis=args.basis, measure=args.measure, reps=args.reps, ms_per_tune=tune_ms,
               fused_over_primitive_tune=round(tune_ms["fused"]["median_ms"] / tune_ms["primitive"]["median_ms"], 4),
               tune_spreads_disjoint=disjoint(tune_ms["fused"], tune_ms["primitive"]),
               ms_per_sweep=sweep_ms, spmm_over_steps_sweep=round(sweep_ms["spmm"]["median_ms"] / sweep_ms["steps"]["median_ms"], 4),
               sweep_spreads_disjoint=disjoint(sweep_ms["spmm"], sweep_ms["steps"]), sweep_routes_max_abs_difference=worst,
               arnoldi=arnoldi, parameter_tuner=parameter_tuner)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
