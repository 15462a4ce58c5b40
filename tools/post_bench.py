#!/usr/bin/env python3
"""Times a postprocessor's ``propagate`` on a symmetrised RMAT graph built on the device, --columns seed sets of --seeds nodes each
drawn among the nodes with edges, around PageRank(0.9, error_type=L1, tol=1e-6):

  transform  ms per transformation of the inner ranker's [n, columns] outcome alone: "slab" through the entries of
             include/pgh_post.h (what ``propagate`` does with it), "columns" through the postprocessor's ``transform`` column by column
             on backend primitives (``fused=False``; the columns are taken out of the slab before the clock starts), and for top and
             ordinals "entries": columns times pgh_vec_kth_largest / pgh_vec_ordinals, the single-vector entries alone;
  propagate  ms per whole ``propagate``: "slab" (one inner batch, slab passes), "columns" (``fused=False``: one inner batch, the
             columns through backend primitives) and "ranks" (``batch=False``: one ``rank()`` per column, the route before the slab
             forms existed).

--chain: top (Top(k)), normalize (Normalize("sum")), sweep (Sweep; its baseline run is made before the clock starts on every route)
or ordinals.  Several chains and widths (comma separated) share one graph.  Every figure is the median of --reps (9) runs timed
with pgh_timer_* (events on the engine's stream, host work between the launches included) in ONE process, the routes alternating,
after a warm-up run of each; min..max is the spread.  A route counts as faster only when the two min..max intervals are disjoint.
Needs an MI355X: there is no fallback.

    python tools/post_bench.py --scale 23 --columns 64 --chain top [--k 10] [--retire] [--out-dir profiles/post]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tune_bench import Timer, summary  # noqa: E402


def disjoint(a, b):
    return a["max_ms"] < b["min_ms"] or b["max_ms"] < a["min_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--columns", default="64")
    ap.add_argument("--chain", default="top")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--retire", action="store_true", help="the inner ranker retires its converged columns (PageRank(retire=True))")
    ap.add_argument("--out-dir", default=None)
    args = ap.parse_args()
    chains = args.chain.split(",")
    widths = [int(w) for w in args.columns.split(",")]
    for chain in chains:
        if chain not in ("top", "normalize", "sweep", "ordinals"):
            raise SystemExit("--chain: top, normalize, sweep or ordinals, not " + chain)

    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    from pygrank_amd.postprocess import _Calls
    from pygrank_amd.synthetic import rmat_graph
    pg.load_backend("hip")
    L.ensure_init()                                          # raises without an MI355X
    if L.entry("pgh_post_kth_largest") is None:
        raise SystemExit("the engine library lacks the entries of include/pgh_post.h")
    timer = Timer(L)

    adj = rmat_graph(args.scale, args.ef, seed=0, symmetrize=True, a=0.57, b=0.19, c=0.19)
    n = adj.array.shape[0]
    nodes = np.flatnonzero(np.asarray(pg.degrees(adj.array)) > 0)

    def ranker():
        return pg.PageRank(0.9, error_type=pg.L1, tol=1e-6, max_iters=1000, retire=args.retire)

    def make(chain, **switches):
        post = dict(top=lambda: pg.Top(ranker(), args.k), normalize=lambda: pg.Normalize(ranker(), "sum"),
                    sweep=lambda: pg.Sweep(ranker()), ordinals=lambda: pg.Ordinals(ranker()))[chain]()
        for name, value in switches.items():
            setattr(post, name, value)
        if chain == "sweep":
            post._uniforms_on(adj)._h                          # noqa: B018 -- the baseline run, once per graph, before any clock
        return post

    for width in widths:
        rng = np.random.default_rng(1)
        columns = []
        for _ in range(width):
            p = np.zeros(n)
            p[rng.choice(nodes, size=min(args.seeds, len(nodes)), replace=False)] = 1.0
            columns.append(pg.DeviceVector.from_host(p))
        F = pg.DeviceMatrix.from_columns(columns)
        del columns
        inner = ranker().propagate(adj, F)
        inner_columns = inner.columns()
        for chain in chains:
            posts = dict(slab=make(chain), columns=make(chain, fused=False), ranks=make(chain, batch=False))

            # ---- the transformation alone
            def slab_route():
                out = posts["slab"]._slab(adj, inner, _Calls())
                assert out is not None
                out.column(0)[0]                               # noqa: B018 -- the result is there
                return out

            def columns_route():
                outs = [posts["columns"].transform(pg.to_signal(adj, column)).np for column in inner_columns]
                outs[-1][0]                                    # noqa: B018
                return outs

            def entries_route():
                if chain == "top":
                    return [column.kth_largest(args.k) for column in inner_columns]
                outs = [column.ordinals() for column in inner_columns]
                outs[-1][0]                                    # noqa: B018
                return outs

            routes = dict(slab=slab_route, columns=columns_route)
            if chain in ("top", "ordinals"):
                routes["entries"] = entries_route
            samples = {name: [] for name in routes}
            for rep in range(args.reps + 1):                   # (the first round warms every code object and pooled block up)
                for name, run in routes.items():
                    ms, _ = timer.time(run)
                    if rep:
                        samples[name].append(ms)
            transform = {name: summary(got) for name, got in samples.items()}

            # ---- the whole propagate
            samples = {name: [] for name in posts}
            for rep in range(args.reps + 1):
                for name, post in posts.items():
                    ms, _ = timer.time(lambda: post.propagate(adj, F).column(0)[0])
                    assert post.last_propagate["route"] == name, (name, post.last_propagate)
                    if rep:
                        samples[name].append(ms)
            propagate = {name: summary(got) for name, got in samples.items()}

            out = dict(tool="post_bench", scale=args.scale, edge_factor=args.ef, n=int(n), nnz=int(adj.array.nnz), columns=width,
                       chain=chain, k=args.k if chain == "top" else None, seeds=args.seeds, reps=args.reps, retire=args.retire,
                       slab_calls=dict(posts["slab"].last_propagate["calls"]),
                       ms_per_transform=transform, ms_per_propagate=propagate,
                       transform_slab_over_columns=round(transform["slab"]["median_ms"] / transform["columns"]["median_ms"], 4),
                       transform_spreads_disjoint=disjoint(transform["slab"], transform["columns"]),
                       propagate_slab_over_ranks=round(propagate["slab"]["median_ms"] / propagate["ranks"]["median_ms"], 4),
                       propagate_slab_ranks_spreads_disjoint=disjoint(propagate["slab"], propagate["ranks"]),
                       propagate_slab_over_columns=round(propagate["slab"]["median_ms"] / propagate["columns"]["median_ms"], 4),
                       propagate_slab_columns_spreads_disjoint=disjoint(propagate["slab"], propagate["columns"]))
            if "entries" in transform:
                out["transform_slab_over_entries"] = round(transform["slab"]["median_ms"] / transform["entries"]["median_ms"], 4)
                out["transform_slab_entries_spreads_disjoint"] = disjoint(transform["slab"], transform["entries"])
            line = json.dumps(out)
            print(line, flush=True)
            if args.out_dir:
                os.makedirs(args.out_dir, exist_ok=True)
                with open(os.path.join(args.out_dir, f"post_bench_scale{args.scale}_b{width}_{chain}{'_retire' if args.retire else ''}.log"), "w") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
