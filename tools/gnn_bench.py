#!/usr/bin/env python
"""Forward + backward of gnn.differentiable_propagate, timed on four routes:

  fused      training mode (graph_dropout = R): one resident loop per pass (include/pgh_gnn.h pgh_linear_run_batch); the features are
             a contiguous f32 tensor on the GPU when torch sees one (views, nothing staged), a CPU tensor otherwise
  stepwise   the same with fused=False: one masked product per step, slab arithmetic on the host
  eval       graph_dropout = 0: ranker.propagate on host-staged slabs, the backward on the transposed operator
  parent     that eval mode on another checkout (--parent-root DIR, its library built): a child process, run once before and once
             after the other routes

    python tools/gnn_bench.py --scale 14 --columns 64 --steps 10 --rate 0.5 [--filter pagerank|generic] [--parent-root DIR] [--log FILE]

--steps K is the filter's max_iters (K - 1 products for PageRank, K - 2 for the ten-hop generic filter's taylor sum).  Every route is
timed `--repeats` times (default 9), the routes ALTERNATING inside every repeat after one untimed warm-up of each; the line reports the
median and the spread (min .. max) per route in milliseconds, wall clock around forward + backward with the device idle at both ends.
Prints one JSON line; --log appends it to a file (profiles/gnn/)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, default=14)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rate", type=float, default=0.5)
    ap.add_argument("--filter", choices=("pagerank", "generic"), default="pagerank")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose pygrank_amd is timed (the child of --parent-root sets it)")
    ap.add_argument("--only", default=None, help="comma-separated routes (default: all this checkout serves)")
    ap.add_argument("--log", default=None)
    return ap.parse_args()


def summary(samples):
    return dict(median_ms=statistics.median(samples), min_ms=min(samples), max_ms=max(samples), n=len(samples))


def main():
    args = parse()
    import torch                                                   # before the engine library loads: one HIP runtime for both
    sys.path.insert(0, args.package_root)
    sys.path.insert(1, ROOT)                                       # oracle.rmat_np (the generator) from this checkout
    import numpy as np
    import pygrank_amd as pg
    from pygrank_amd import gnn
    from oracle import rmat_np
    pg.load_backend("hip")
    cuda = torch.cuda.is_available()
    A = rmat_np.rmat_csr(args.scale, 8, seed=5)
    n = A.shape[0]
    graph = pg.AdjacencyWrapper(A, directed=True)
    pre = pg.preprocessor(normalization="col", assume_immutability=True)
    if args.filter == "pagerank":
        ranker = pg.PageRank(0.9, preprocessor=pre, use_quotient=False, error_type="iters", max_iters=args.steps)
    else:
        ranker = pg.GenericGraphFilter([0.9 ** k for k in range(10)], preprocessor=pre, error_type="iters", max_iters=args.steps)
    rng = np.random.default_rng(1)
    device = "cuda" if cuda else "cpu"
    base = torch.tensor(rng.random((n, args.columns)), dtype=torch.float32, device=device)
    W = torch.tensor(rng.random((n, args.columns)), dtype=torch.float32, device=device)
    training = "graph_dropout" in gnn.differentiable_propagate.__code__.co_varnames
    routes = dict(eval=dict())
    if training:
        routes = dict(fused=dict(graph_dropout=args.rate), stepwise=dict(graph_dropout=args.rate, fused=False), eval=dict(graph_dropout=0))
    if args.only:
        routes = {name: routes[name] for name in args.only.split(",")}

    def once(kwargs):
        X = base.clone().requires_grad_(True)
        if cuda:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        Y = gnn.differentiable_propagate(ranker, graph, X, **kwargs)
        (Y * W).sum().backward()
        if cuda:
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def parent():
        cmd = [sys.executable, os.path.abspath(__file__), "--package-root", args.parent_root, "--only", "eval", "--scale", str(args.scale),
               "--columns", str(args.columns), "--steps", str(args.steps), "--filter", args.filter, "--repeats", str(args.repeats)]
        out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1]
        return json.loads(out)["routes"]["eval"]

    result = dict(tool="gnn_bench", scale=args.scale, n=n, nnz=int(A.nnz), columns=args.columns, steps=args.steps, rate=args.rate,
                  filter=args.filter, tensors=device, package_root=os.path.relpath(args.package_root, ROOT), routes={})
    if args.parent_root:
        result["routes"]["parent_before"] = parent()
    samples = {name: [] for name in routes}
    taken = {}
    for name, kwargs in routes.items():                           # warm-up: images, the transposed graph, code objects
        once(kwargs)
        taken[name] = dict(route=getattr(gnn, "last_call", {}).get("route"), staged_bytes=getattr(gnn, "last_call", {}).get("staged_bytes"))
    for _ in range(args.repeats):
        for name, kwargs in routes.items():
            samples[name].append(once(kwargs))
    for name in routes:
        result["routes"][name] = dict(summary(samples[name]), **taken[name])
    if args.parent_root:
        result["routes"]["parent_after"] = parent()
    line = json.dumps(result)
    print(line)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as log:
            log.write(line + "\n")


if __name__ == "__main__":
    main()
