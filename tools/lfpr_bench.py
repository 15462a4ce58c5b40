#!/usr/bin/env python3
"""Times pg.LFPR on a symmetrised RMAT graph built on the device (raw adjacency, normalization="none"), 100 seeds drawn as bench.py
draws them and a random fifth of the nodes as the sensitive group:

  step      ms per step of LFPR(fused=True), of LFPR(fused=False) and -- beside them -- of PageRank through the backend primitives
            (its device loop switched off, as tests/core_checks.py does), each as (rank() of LONG iterations - rank() of SHORT
            iterations) / (LONG - SHORT) with error_type="iters", so that set-up, the ways in and out of the id space and the end of the
            run cancel;
  rank      ms per rank() of LFPR(error_type=L1, tol=--tol) on both routes, with the iteration count;
  image     ms per rank() on a host (scipy) copy of an RMAT graph of --image-scale with the default preprocessor, which builds the
            device image on every call as the reference does, and with preprocessor(normalization="none", assume_immutability=True),
            which builds it once (the run that builds it is not timed).

Every figure is the median of --reps (9) runs timed with pgh_timer_* (events on the engine's stream, host work between the launches
included) in ONE process, the routes alternating, after a warm-up run of each; min..max is the spread.  Needs an MI355X: there is no
fallback.

    python tools/lfpr_bench.py --scale 23 [--redistributor original] [--out profiles/lfpr/lfpr_bench_scale23.log]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tune_bench import Timer, summary  # noqa: E402

SHORT, LONG = 6, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--redistributor", default=None, choices=[None, "uniform", "original"])
    ap.add_argument("--image-scale", type=int, default=None, help="scale of the host graph of the `image` rows (default: min(scale, 20))")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    from pygrank_amd.synthetic import rmat_graph
    pg.load_backend("hip")
    L.ensure_init()                                          # raises without an MI355X
    if L.entry("pgh_lfpr_close") is None:
        raise SystemExit("the engine library lacks pgh_lfpr_close")
    timer = Timer(L)

    def operands(graph, n, degrees):
        rng = np.random.default_rng(1)
        nodes = np.flatnonzero(degrees > 0)
        p, s = np.zeros(n), np.zeros(n)
        p[np.sort(rng.choice(nodes, size=min(args.seeds, len(nodes)), replace=False))] = 1.0
        s[rng.choice(n, n // 5, replace=False)] = 1.0
        return pg.to_signal(graph, p), pg.to_signal(graph, s)

    adj = rmat_graph(args.scale, args.ef, seed=0, normalization="none", symmetrize=True, a=0.57, b=0.19, c=0.19)
    n = adj.array.shape[0]
    signal, sensitive = operands(adj, n, np.asarray(pg.degrees(adj.array)))

    def lfpr(fused, redistributor=args.redistributor, **kwargs):
        return pg.LFPR(0.85, redistributor, fused=fused, **kwargs)

    def pagerank(**kwargs):
        ranker = pg.PageRank(0.85, **kwargs)
        ranker._fused_loop = lambda *a, **k: False
        ranker._fused_rank = lambda *a, **k: None
        return ranker

    def run(ranker, with_sensitive=True):
        out = ranker.rank(adj, signal, sensitive=sensitive) if with_sensitive else ranker.rank(adj, signal)
        np.asarray(out.np[0])                                # the result in the caller's ids (a lazy outcome is evaluated here)
        return ranker

    routes = dict(lfpr_fused=lambda **k: run(lfpr(True, **k)), lfpr_primitives=lambda **k: run(lfpr(False, **k)),
                  pagerank_primitives=lambda **k: run(pagerank(**k), False))
    # (the step rows always use the uniform redistributor: the redistributor enters _start only, and the inner PageRank of "original"
    # shares the manager, whose "iters" count it would use up)
    samples = {name: {SHORT: [], LONG: []} for name in routes}
    for rep in range(args.reps + 1):                         # (the first round warms every code object and pooled block up)
        for name, make in routes.items():
            for iters in (SHORT, LONG):
                kwargs = dict(error_type="iters", max_iters=iters, **({} if name == "pagerank_primitives" else dict(redistributor=None)))
                ms, ranker = timer.time(lambda: make(**kwargs))
                assert ranker.convergence.iteration == iters
                if rep:
                    samples[name][iters].append(ms)
    step = {name: summary([(b - a) / (LONG - SHORT) for a, b in zip(got[SHORT], got[LONG])]) for name, got in samples.items()}

    rank = {}
    rank_samples = {name: [] for name in ("lfpr_fused", "lfpr_primitives")}
    iterations = {}
    for rep in range(args.reps + 1):
        for name in rank_samples:
            ms, ranker = timer.time(lambda: routes[name](error_type=pg.L1, tol=args.tol, max_iters=1000))
            iterations[name] = int(ranker.convergence.iteration)
            if rep:
                rank_samples[name].append(ms)
    for name, got in rank_samples.items():
        rank[name] = dict(summary(got), iterations=iterations[name])

    image_scale = min(args.scale, 20) if args.image_scale is None else args.image_scale
    small = rmat_graph(image_scale, args.ef, seed=0, normalization="none", symmetrize=True, a=0.57, b=0.19, c=0.19)
    host = small.array.download_transposed().tocsr()         # (symmetric: M^T is M)
    graph = pg.AdjacencyWrapper(host, directed=False)
    del small
    signal2, sensitive2 = operands(graph, host.shape[0], np.asarray(host.sum(axis=1)).ravel())
    remembered = pg.preprocessor(normalization="none", assume_immutability=True)
    image_samples = dict(rebuilt_per_rank=[], remembered=[])
    for rep in range(args.reps + 1):
        for name, extra in (("rebuilt_per_rank", {}), ("remembered", dict(preprocessor=remembered))):
            def once():
                ranker = lfpr(True, error_type=pg.L1, tol=args.tol, max_iters=1000, **extra)
                np.asarray(ranker.rank(graph, signal2, sensitive=sensitive2).np[0])
                return ranker
            ms, ranker = timer.time(once)
            if rep:
                image_samples[name].append(ms)
    image = {name: summary(got) for name, got in image_samples.items()}

    out = dict(tool="lfpr_bench", scale=args.scale, edge_factor=args.ef, n=int(n), nnz=int(adj.array.nnz), seeds=args.seeds,
               redistributor=args.redistributor or "uniform", reps=args.reps, tol=args.tol, step_from_iterations=[SHORT, LONG],
               ms_per_step=step, ms_per_rank=rank,
               fused_over_primitives_step=round(step["lfpr_fused"]["median_ms"] / step["lfpr_primitives"]["median_ms"], 4),
               fused_over_primitives_rank=round(rank["lfpr_fused"]["median_ms"] / rank["lfpr_primitives"]["median_ms"], 4),
               fused_step_over_pagerank_primitive_step=round(step["lfpr_fused"]["median_ms"] / step["pagerank_primitives"]["median_ms"], 4),
               image=dict(scale=image_scale, n=int(host.shape[0]), nnz=int(host.nnz), ms_per_rank=image,
                          remembered_over_rebuilt=round(image["remembered"]["median_ms"] / image["rebuilt_per_rank"]["median_ms"], 4)))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
