#!/usr/bin/env python3
"""Times the Krylov-space route of a closed-form filter on a symmetrised RMAT graph built on the device (normalization="symmetric"),
100 seeds drawn as bench.py draws them:

  rank      ms per rank() of the filter with krylov_dims=K fused (include/pgh_krylov.h), of the same with fused=False (backend
            primitives), and of the same filter WITHOUT krylov_dims (the engine's polynomial loop, pgh_poly_run), each with
            error_type=L1 and --tol, with the iteration count and the products it cost;
  basis     ms per Lanczos basis of K dimensions on both routes, and per step (= basis / K: set-up, the division of the columns and
            the way in amortised over the steps);
  residual  ms per pgh_krylov_residuals pass over the [n, K] basis for 64 iterations and for as many as the fused rank() took, beside
            ONE iteration's residual in primitives (a pgh_mat_gemv and two reductions), and the rank vector's pgh_mat_gemv + way out.

Every figure is the median of --reps (9) runs timed with pgh_timer_* (events on the engine's stream, host work between the launches
included) in ONE process, the routes alternating, after a warm-up run of each; min..max is the spread.  Needs an MI355X: there is no
fallback.

    python tools/krylov_bench.py --scale 23 --dims 10 [--filter heat|pprc] [--tol 1e-6] [--out profiles/krylov/krylov_bench_scale23_k10_heat.log]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--dims", type=int, default=10)
    ap.add_argument("--filter", default="heat", choices=["heat", "pprc"])
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    from pygrank_amd import krylov
    from pygrank_amd.synthetic import rmat_graph
    pg.load_backend("hip")
    L.ensure_init()                                          # raises without an MI355X
    if L.entry("pgh_lanczos_close") is None or L.entry("pgh_krylov_residuals") is None:
        raise SystemExit("the engine library lacks the entries of include/pgh_krylov.h")
    warnings.simplefilter("ignore")                          # "Krylov approximation is not stable yet", once per basis
    timer = Timer(L)

    adj = rmat_graph(args.scale, args.ef, seed=0, normalization="symmetric", symmetrize=True, a=0.57, b=0.19, c=0.19)
    n = adj.array.shape[0]
    rng = np.random.default_rng(1)
    nodes = np.flatnonzero(np.asarray(pg.degrees(adj.array)) > 0)
    p = np.zeros(n)
    p[np.sort(rng.choice(nodes, size=min(args.seeds, len(nodes)), replace=False))] = 1.0
    signal = pg.to_signal(adj, p)
    normalised = signal.np / pg.sum(pg.abs(signal.np))
    np.asarray(normalised[0])

    def make(**kwargs):
        common = dict(error_type=pg.L1, tol=args.tol, max_iters=1000, **kwargs)
        return pg.HeatKernel(t=3, **common) if args.filter == "heat" else pg.PageRankClosed(0.85, **common)

    def run(ranker):
        np.asarray(ranker.rank(adj, signal).np[0])           # the result in the caller's ids (a lazy outcome is evaluated here)
        return ranker

    routes = dict(krylov_fused=lambda: run(make(krylov_dims=args.dims, fused=True)),
                  krylov_primitives=lambda: run(make(krylov_dims=args.dims, fused=False)),
                  node_space=lambda: run(make()))
    samples, facts = {name: [] for name in routes}, {}
    for rep in range(args.reps + 1):                         # (the first round warms every code object and pooled block up)
        for name, once in routes.items():
            ms, ranker = timer.time(once)
            facts[name] = dict(iterations=int(ranker.convergence.iteration), spmv=int(ranker.last_loop["spmv"]))
            if name == "krylov_fused":
                facts[name]["residual_passes"] = int(ranker.last_loop["residual_passes"])
            if rep:
                samples[name].append(ms)
    rank = {name: dict(summary(got), **facts[name]) for name, got in samples.items()}

    def basis_of(fused):
        basis = krylov.lanczos(adj.array, normalised, args.dims, fused=fused)
        L.check(L.lib().pgh_sync())
        return basis
    basis_samples = dict(fused=[], primitives=[])
    kept = None
    for rep in range(args.reps + 1):
        for name in basis_samples:
            ms, basis = timer.time(lambda: basis_of(name == "fused"))
            if name == "fused":
                kept = basis
            if rep:
                basis_samples[name].append(ms)
    basis_ms = {name: summary(got) for name, got in basis_samples.items()}
    step_ms = {name: summary([ms / args.dims for ms in got]) for name, got in basis_samples.items()}

    taken = max(rank["krylov_fused"]["iterations"] - 1, 1)
    deltas = np.random.default_rng(2).random((args.dims, 64)) - 0.5
    parts = {
        "residuals_64_iterations": lambda: kept.residuals(deltas, True),
        f"residuals_{min(taken, 64)}_iterations": lambda: kept.residuals(deltas[:, :min(taken, 64)], True),
        "residual_1_iteration_primitives": lambda: kept.residuals(deltas[:, :1], False),
        "ranks_gemv_and_way_out": lambda: np.asarray(kept.project(deltas[:, 0])[0]),
    }
    part_samples = {name: [] for name in parts}
    for rep in range(args.reps + 1):
        for name, once in parts.items():
            ms, got = timer.time(once)
            if name.startswith("residuals_"):
                assert got[2] == 1                            # the fused pass served it
            if rep:
                part_samples[name].append(ms)
    residual = {name: summary(got) for name, got in part_samples.items()}

    out = dict(tool="krylov_bench", scale=args.scale, edge_factor=args.ef, n=int(n), nnz=int(adj.array.nnz), seeds=args.seeds,
               filter=args.filter, dims=args.dims, tol=args.tol, error_type="L1", reps=args.reps, ms_per_rank=rank, ms_per_basis=basis_ms,
               ms_per_lanczos_step=step_ms, ms_per_part=residual,
               fused_over_primitives_rank=round(rank["krylov_fused"]["median_ms"] / rank["krylov_primitives"]["median_ms"], 4),
               fused_over_primitives_step=round(step_ms["fused"]["median_ms"] / step_ms["primitives"]["median_ms"], 4),
               krylov_fused_over_node_space_rank=round(rank["krylov_fused"]["median_ms"] / rank["node_space"]["median_ms"], 4))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
