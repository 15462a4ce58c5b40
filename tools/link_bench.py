#!/usr/bin/env python3
"""Times one LinkAssessment.evaluate (the default measure, AUC) on an undirected R-MAT graph of 2^scale nodes (edge factor 8) against a
slab of --columns columns of random scores in [0, 1) (three in ten are zeros: ties):

  (a) device:  the entries of include/pgh_link.h through the instance's plan -- row pass, pair pass, radix sort, integer count; the slab
               stays on the device;
  (b) host:    fused=False -- the slab is downloaded (n x columns doubles) and the same restatement runs in numpy.

Both are timed with time.perf_counter around evaluate (the device route synchronises before it returns) in ONE process, alternating,
after a warm-up of each that also builds the plan; medians and min..max over the repetitions are reported, and a route counts as faster
only when the two min..max intervals are disjoint.  The plan -- the sample, the BFS balls and the pair list, numpy on the host CSR -- is
built once per instance and shared by every evaluation; its construction is timed apart, on fresh instances (--plan-reps).  The
device route's stages are not timed one by one here.  Needs an MI355X: there is no fallback.

    python tools/link_bench.py --scale 20 --columns 64 [--hops 1] [--similarity cos|dot] [--reps 9] [--plan-reps 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summary(samples):
    return dict(median_ms=round(statistics.median(samples), 4), min_ms=round(min(samples), 4), max_ms=round(max(samples), 4),
                samples=len(samples))


def timed(fn):
    start = time.perf_counter()
    value = fn()
    return (time.perf_counter() - start) * 1e3, value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--hops", type=int, default=1)
    ap.add_argument("--similarity", choices=["cos", "dot"], default="cos")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--plan-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 repetitions")

    import scipy.sparse as sp
    import pygrank_amd as pg
    from oracle import rmat_np
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix
    pg.load_backend("hip")
    L.ensure_init()                                          # raises without an MI355X
    if any(L.entry(name) is None for name in L.LINK_SIGNATURES):
        raise SystemExit("the engine library lacks the entries of include/pgh_link.h")
    warnings.simplefilter("ignore")
    A = rmat_np.rmat_csr(args.scale, 8, seed=3)
    A = sp.csr_array(A + A.T)
    graph = pg.AdjacencyWrapper(A, directed=False)
    n, b = A.shape[0], args.columns
    rng = np.random.default_rng(1)
    slab = DeviceMatrix.empty(n, b)
    for j in range(b):
        column = rng.random(n, dtype=np.float32)
        column[rng.random(n) < 0.3] = 0.0
        slab.set_column(j, pg.DeviceVector.from_host(column))
    kwargs = dict(hops=args.hops, similarity=args.similarity)
    plan_ms = []
    for _ in range(max(1, args.plan_reps)):
        ms, plan = timed(pg.LinkAssessment(graph, **kwargs).plan)
        plan_ms.append(ms)
    device, host = pg.LinkAssessment(graph, **kwargs), pg.LinkAssessment(graph, fused=False, **kwargs)
    runs = dict(device=lambda: device.evaluate(slab), host=lambda: host.evaluate(slab))
    values = {key: run() for key, run in runs.items()}       # warm-up: the plans, the device scratch, every code object
    assert (device.last_route, host.last_route) == ("device", "host")
    samples = {key: [] for key in runs}
    for _ in range(args.reps):
        for key, run in runs.items():
            ms, values[key] = timed(run)
            samples[key].append(ms)
    out = dict(tool="link_bench", scale=args.scale, n=n, nnz=int(A.nnz), columns=b, hops=args.hops, similarity=args.similarity,
               reps=args.reps, pairs=plan.num_pairs, positives=plan.num_positive, candidates=len(plan.candidates),
               plan_build=summary(plan_ms), device=summary(samples["device"]), host=summary(samples["host"]),
               slab_download_bytes=n * b * 8)
    out["device_over_host"] = round(out["device"]["median_ms"] / out["host"]["median_ms"], 5)
    out["spreads_disjoint"] = bool(out["device"]["max_ms"] < out["host"]["min_ms"] or out["host"]["max_ms"] < out["device"]["min_ms"])
    out["values_equal"] = bool(values["device"] == values["host"])
    out["auc"] = values["device"]
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
