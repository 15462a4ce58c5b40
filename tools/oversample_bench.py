#!/usr/bin/env python3
"""Times pg.BoostedSeedOversampling on a symmetrised RMAT graph built on the device, --columns seed sets of --seeds nodes each drawn
among the nodes with edges:

  propagate  ms per BoostedSeedOversampling(PageRank(0.9, error_type=L1, tol=1e-6)).propagate(graph, seed sets) as one batch (every
             round one multi-seed run of the live columns whatever their number: min_batch_width=2) and with batch=False (the columns one by one), with the columns' rounds;
  inner      ms per PageRank.propagate of the seed sets (one multi-seed run) and per PageRank.rank of the first of them, with the
             iteration counts: what a round spends most of its time in on either route;
  round      ms per round's slab passes -- resample, the three sums, the update with the next floor -- and of the first floor, on
             [n, columns] slabs through include/pgh_oversample.h (fused) and from backend primitives (fused=False).

Every figure is the median of --reps (9) runs timed with pgh_timer_* (events on the engine's stream, host work between the launches
included) in ONE process, the routes alternating, after a warm-up run of each; min..max is the spread.  Needs an MI355X: there is no
fallback.

    python tools/oversample_bench.py --scale 23 --columns 64 [--objective naive] [--source original] [--retire] [--out profiles/oversampling/...log]
"""
import argparse
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
    ap.add_argument("--objective", default="partial", choices=["partial", "naive"])
    ap.add_argument("--source", default="previous", choices=["previous", "original"])
    ap.add_argument("--retire", action="store_true", help="the inner ranker retires its converged columns (PageRank(retire=True))")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    from pygrank_amd.oversampling import _SlabPasses
    from pygrank_amd.synthetic import rmat_graph
    pg.load_backend("hip")
    L.ensure_init()                                          # raises without an MI355X
    if L.entry("pgh_boost_update") is None:
        raise SystemExit("the engine library lacks pgh_boost_update")
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
    del columns

    def boosted(**kwargs):
        ranker = pg.PageRank(0.9, error_type=pg.L1, tol=1e-6, max_iters=1000, retire=args.retire)
        return pg.BoostedSeedOversampling(ranker, args.objective, args.source, **kwargs)

    def run(**kwargs):
        algo = boosted(**kwargs)
        out = algo.propagate(adj, F)
        out.column(0)[0]                                     # noqa: B018 -- the result is there
        return algo

    samples = dict(batch=[], one_by_one=[])
    rounds = {}
    for rep in range(args.reps + 1):                         # (the first round warms every code object and pooled block up)
        for name, kwargs in (("batch", dict(min_batch_width=2)), ("one_by_one", dict(batch=False))):
            ms, algo = timer.time(lambda: run(**kwargs))
            rounds[name] = list(algo.last_rounds)
            widths = algo.last_widths
            if name == "batch":
                batch_widths = widths[0]
                assert algo.last_passes["primitive"] == 0
            if rep:
                samples[name].append(ms)
    assert rounds["batch"] == rounds["one_by_one"], (rounds["batch"], rounds["one_by_one"])
    propagate = {name: summary(got) for name, got in samples.items()}

    # what a round spends most of its time in: the inner ranker on the seed sets, as one multi-seed run and as a single rank()
    ranker = pg.PageRank(0.9, error_type=pg.L1, tol=1e-6, max_iters=1000, retire=args.retire)
    first = pg.to_signal(adj, F.column(0))
    inner_samples = dict(propagate=[], rank=[])
    for rep in range(args.reps + 1):
        ms_many, _ = timer.time(lambda: ranker.propagate(adj, F).column(0)[0])
        many_iterations = [r["iterations"] for r in ranker.last_batches[0]] if getattr(ranker, "last_batches", None) else []
        ms_one, _ = timer.time(lambda: ranker.rank(adj, first).np[0])
        one_iterations = int(ranker.convergence.iteration)
        if rep:
            inner_samples["propagate"].append(ms_many)
            inner_samples["rank"].append(ms_one)
    inner = dict(propagate=dict(summary(inner_samples["propagate"]), iterations_min=min(many_iterations, default=0),
                                iterations_max=max(many_iterations, default=0)),
                 rank=dict(summary(inner_samples["rank"]), iterations=one_iterations))

    # one round's passes on full-width slabs: the ranks of the seed sets as `total`, a second copy as `fresh`
    ranker = pg.PageRank(0.9, error_type=pg.L1, tol=1e-6, max_iters=1000)
    total = ranker.propagate(adj, F)
    fresh = ranker.propagate(adj, F)
    weights = [0.01] * F.b
    pass_samples = dict(fused=dict(floor=[], round=[]), primitives=dict(floor=[], round=[]))
    for rep in range(args.reps + 1):
        for name, fused in (("fused", True), ("primitives", False)):
            passes = _SlabPasses(fused)
            ms_floor, (floors, counts) = timer.time(lambda: passes.floor(total, F))

            def one_round():
                grown, _ = passes.resample(total, floors)
                passes.forms(grown, fresh, total)
                return passes.update(total, fresh, weights, grown)
            ms_round, _ = timer.time(one_round)
            assert passes.calls == (dict(fused=4, primitive=0) if fused else dict(fused=0, primitive=4))
            if rep:
                pass_samples[name]["floor"].append(ms_floor)
                pass_samples[name]["round"].append(ms_round)
    per_round = {name: {what: summary(got) for what, got in both.items()} for name, both in pass_samples.items()}

    out = dict(tool="oversample_bench", scale=args.scale, edge_factor=args.ef, n=int(n), nnz=int(adj.array.nnz), columns=args.columns,
               seeds=args.seeds, objective=args.objective, source=args.source, reps=args.reps, retire=args.retire,
               rounds=dict(min=min(rounds["batch"]), max=max(rounds["batch"]), total=sum(rounds["batch"])), batch_widths=batch_widths,
               ms_per_propagate=propagate,
               batch_over_one_by_one=round(propagate["batch"]["median_ms"] / propagate["one_by_one"]["median_ms"], 4),
               ms_per_inner_run=inner, ms_per_round_passes=per_round,
               fused_over_primitives_round=round(per_round["fused"]["round"]["median_ms"] / per_round["primitives"]["round"]["median_ms"], 4),
               fused_over_primitives_floor=round(per_round["fused"]["floor"]["median_ms"] / per_round["primitives"]["floor"]["median_ms"], 4))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
