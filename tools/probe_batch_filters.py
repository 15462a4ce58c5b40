"""Multi-seed loops of the closed-form filters and the absorbing walks (include/pgh_batch.h) against the column loop they replace:
HeatKernel (t = 5: default rule, and 31 terms) and AbsorbingWalks (alpha = 0.85, L1 1e-6) on RMAT with b personalizations of 100 seeds each,
once through ``propagate`` (one device loop per 64 columns) and once column by column (NodeRanking.propagate: one fused single-vector
run per column).  Reports ms per batch step, the column loop's ms per column step, and the speedup of the whole call.
Usage: python tools/probe_batch_filters.py --scale 23 --batch 64"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pygrank_amd as pg  # noqa: E402
from pygrank_amd import _lib as L  # noqa: E402
from pygrank_amd.signals import NodeRanking  # noqa: E402
from pygrank_amd.synthetic import rmat_graph  # noqa: E402


def timed(fn, reps=2):
    out, best = None, None
    for _ in range(reps):
        del out                                   # (a result kept across the call costs the next one a 2 GB allocation)
        L.check(L.lib().pgh_sync())
        t0 = time.perf_counter()
        out = fn()
        L.check(L.lib().pgh_sync())
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=23)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    pg.load_backend("hip")
    adj = rmat_graph(args.scale, 16, seed=0)
    g = adj.array
    n = g.shape[0]
    cand = np.flatnonzero(np.asarray(pg.degrees(g)) > 0)
    feats = np.zeros((n, args.batch))
    for j in range(args.batch):
        feats[np.sort(np.random.default_rng(1 + j).choice(cand, 100, replace=False)), j] = 1.0
    F = pg.to_primitive(feats)
    report = dict(scale=args.scale, batch=args.batch, nnz=int(g.nnz))
    # (the default rule, Mabs 1e-6, divides by n: at scale 23 |result_1| / n is below it and every column stops at iteration 2 without a
    # product -- the fixed 31-term run, BASELINE.json configs[3], is what measures a step)
    for name, make in (("heat_kernel_t5", lambda: pg.HeatKernel(5)),
                       ("heat_kernel_t5_31_terms", lambda: pg.HeatKernel(5, error_type="iters", max_iters=31)),
                       ("absorbing_walks_085_l1", lambda: pg.AbsorbingWalks(0.85, error_type=pg.L1, tol=1e-6, max_iters=1000))):
        ranker = make()
        out, dt_b = timed(lambda: ranker.propagate(adj, F))
        info = [c for batch in ranker.last_batches for c in batch]
        steps = max(c["spmv"] for c in info)
        loop_ms = sum(batch[0]["loop_ms"] for batch in ranker.last_batches)
        single = make()
        ref, dt_c = timed(lambda: NodeRanking.propagate(single, adj, F), reps=1)
        worst = max(float(np.max(np.abs(np.asarray(out)[:, j] - np.asarray(ref)[:, j])) / np.max(np.abs(np.asarray(ref)[:, j])))
                    for j in range(args.batch))
        col_steps = sum(c["spmv"] for c in info)
        report[name] = dict(batch_wall_ms=round(dt_b * 1e3, 1), batch_loop_ms=round(loop_ms, 1), batch_steps=steps,
                            ms_per_batch_step=round(loop_ms / max(steps, 1), 3), column_loop_wall_ms=round(dt_c * 1e3, 1),
                            column_steps=col_steps, ms_per_column_step=round(dt_c * 1e3 / max(col_steps, 1), 3),
                            speedup=round(dt_c / dt_b, 2), worst_rel_linf_vs_column_loop=worst,
                            iterations=sorted(set(c["iterations"] for c in info)))
        print(name, json.dumps(report[name]), flush=True)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
