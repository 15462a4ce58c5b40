#!/usr/bin/env python3
"""Times pg.BoostedSeedOversampling on a symmetrised RMAT graph built on the device, --columns seed sets of --seeds nodes each drawn
among the nodes with edges:

  propagate  ms per BoostedSeedOversampling(PageRank(0.9, error_type=L1, tol=1e-6)).propagate(graph, seed sets) as one batch (every
             round one multi-seed run of the live columns whatever their number: min_batch_width=2) and with batch=False (the columns one by one), with the columns' rounds;
  inner      ms per PageRank.propagate of the seed sets (one multi-seed run) and per PageRank.rank of the first of them, with the
             iteration counts: what a round spends most of its time in on either route;
  round      ms per round's slab passes -- resample, the three sums, the update with the next floor -- and of the first floor, on
             [n, columns] slabs through include/pgh_oversample.h (fused) and from backend primitives (fused=False).

Every figure is the median of --reps (9) runs timed as tools/benchkit.py fixes it (pgh_timer_* events, ONE process, the routes
alternating after a warm-up round of each); min..max is the spread.  Needs an MI355X: there is no
fallback.

    python tools/oversample_bench.py --scale 23 --columns 64 [--objective naive] [--source original] [--retire] [--out profiles/oversampling/...log]
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--objective", default="partial", choices=["partial", "naive"])
    ap.add_argument("--source", default="previous", choices=["previous", "original"])
    ap.add_argument("--retire", action="store_true", help="the inner ranker retires its converged columns (PageRank(retire=True))")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    pg, _, timer = engine("pgh_boost_update")
    from pygrank_amd.oversampling import _SlabPasses

    adj = rmat(args, symmetrize=True)
    n = adj.array.shape[0]
    F = pg.DeviceMatrix.from_columns(seed_columns(pg, n, nodes_with_edges(pg, adj), args.columns, args.seeds, np.random.default_rng(1)))

    def boosted(**kwargs):
        ranker = pg.PageRank(0.9, error_type=pg.L1, tol=1e-6, max_iters=1000, retire=args.retire)
        return pg.BoostedSeedOversampling(ranker, args.objective, args.source, **kwargs)

    def run(**kwargs):
        algo = boosted(**kwargs)
        out = algo.propagate(adj, F)
        out.column(0)[0]                                     # noqa: B018 -- the result is there
        return algo

    rounds, widths = {}, {}

    def what_it_ran(name, algo):
        rounds[name], widths[name] = list(algo.last_rounds), algo.last_widths
        assert name != "batch" or algo.last_passes["primitive"] == 0
    propagate, _ = alternate(timer, dict(batch=lambda: run(min_batch_width=2), one_by_one=lambda: run(batch=False)), args.reps,
                             what_it_ran, keep=False)
    batch_widths = widths["batch"][0]
    assert rounds["batch"] == rounds["one_by_one"], (rounds["batch"], rounds["one_by_one"])

    # what a round spends most of its time in: the inner ranker on the seed sets, as one multi-seed run and as a single rank()
    ranker = pg.PageRank(0.9, error_type=pg.L1, tol=1e-6, max_iters=1000, retire=args.retire)
    first = pg.to_signal(adj, F.column(0))
    counts = {}

    def iterations(name, _):                                 # (the ranker is shared: each route's count is read before the other runs)
        if name == "propagate":
            counts[name] = [r["iterations"] for r in ranker.last_batches[0]] if getattr(ranker, "last_batches", None) else []
        else:
            counts[name] = int(ranker.convergence.iteration)
    inner, _ = alternate(timer, dict(propagate=lambda: ranker.propagate(adj, F).column(0)[0], rank=lambda: ranker.rank(adj, first).np[0]),
                         args.reps, iterations)
    inner["propagate"].update(iterations_min=min(counts["propagate"], default=0), iterations_max=max(counts["propagate"], default=0))
    inner["rank"].update(iterations=counts["rank"])

    # one round's passes on full-width slabs: the ranks of the seed sets as `total`, a second copy as `fresh`
    ranker = pg.PageRank(0.9, error_type=pg.L1, tol=1e-6, max_iters=1000)
    total = ranker.propagate(adj, F)
    fresh = ranker.propagate(adj, F)
    weights = [0.01] * F.b
    names = ("fused", "primitives")
    passes, floors = {name: _SlabPasses(name == "fused") for name in names}, []

    def one_round(name):
        grown, _ = passes[name].resample(total, floors[0])
        passes[name].forms(grown, fresh, total)
        return passes[name].update(total, fresh, weights, grown)

    def between(key, value):                                 # a route's floor feeds its round; every round counts its four passes anew
        name, what = key
        if what == "floor":
            floors[:] = [value[0]]
        else:
            assert passes[name].calls == (dict(fused=4, primitive=0) if name == "fused" else dict(fused=0, primitive=4))
            passes[name] = _SlabPasses(name == "fused")
    routes = {}
    for name in names:
        routes[(name, "floor")] = lambda name=name: passes[name].floor(total, F)
        routes[(name, "round")] = lambda name=name: one_round(name)
    got, _ = alternate(timer, routes, args.reps, between, keep=False)
    per_round = {name: dict(floor=got[(name, "floor")], round=got[(name, "round")]) for name in names}

    out = dict(tool="oversample_bench", scale=args.scale, edge_factor=args.ef, n=int(n), nnz=int(adj.array.nnz), columns=args.columns,
               seeds=args.seeds, objective=args.objective, source=args.source, reps=args.reps, retire=args.retire,
               rounds=dict(min=min(rounds["batch"]), max=max(rounds["batch"]), total=sum(rounds["batch"])), batch_widths=batch_widths,
               ms_per_propagate=propagate,
               batch_over_one_by_one=over(propagate["batch"], propagate["one_by_one"]),
               ms_per_inner_run=inner, ms_per_round_passes=per_round,
               fused_over_primitives_round=over(per_round["fused"]["round"], per_round["primitives"]["round"]),
               fused_over_primitives_floor=over(per_round["fused"]["floor"], per_round["primitives"]["floor"]))
    emit(out, args.out)


if __name__ == "__main__":
    main()
