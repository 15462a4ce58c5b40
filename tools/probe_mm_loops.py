"""Whole-call wall times of the multi-seed loops on one checkout (--root): PageRank L1 1e-6, HeatKernel 31 terms and AbsorbingWalks L1
through propagate (the settings of tools/probe_batch_filters.py, without its column loop), the two mixed entries called directly, and
pgh_linear_run_batch (tools/gnn_bench.py's setting: 64 columns, 10 steps, rate 0.5).  One JSON line: per figure the wall time of every
repeat behind a first, untimed-for-the-median call.  Two checkouts are compared by alternating processes (profiles/mm_loops/README.md).
Usage: python tools/probe_mm_loops.py --root . --tag head --scale 23"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", required=True)
ap.add_argument("--tag", required=True)
ap.add_argument("--scale", type=int, default=23)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import pygrank_amd as pg  # noqa: E402
from pygrank_amd import _lib as L  # noqa: E402
from pygrank_amd.device import DeviceMatrix  # noqa: E402
from pygrank_amd.synthetic import rmat_graph  # noqa: E402
assert os.path.abspath(pg.__file__).startswith(os.path.abspath(args.root)), pg.__file__
pg.load_backend("hip")
adj = rmat_graph(args.scale, 16, seed=0)
g = adj.array
n, b = g.shape[0], args.batch
cand = np.flatnonzero(np.asarray(pg.degrees(g)) > 0)
feats = np.zeros((n, b), dtype=np.float32)
for j in range(b):
    feats[np.sort(np.random.default_rng(1 + j).choice(cand, 100, replace=False)), j] = 1.0
F = pg.to_primitive(feats)
sync = lambda: L.check(L.lib().pgh_sync())


def timed(fn):
    times, out = [], None
    for _ in range(args.reps + 1):                     # the first call pays the layout build and the pool's first allocations
        del out
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return times[1:]


report = dict(tag=args.tag, scale=args.scale, batch=b)
for name, make in (("ppr_l1", lambda: pg.PageRank(0.85, error_type=pg.L1, tol=1e-6, max_iters=1000)),
                   ("heat_31_terms", lambda: pg.HeatKernel(5, error_type="iters", max_iters=31)),
                   ("absorbing_l1", lambda: pg.AbsorbingWalks(0.85, error_type=pg.L1, tol=1e-6, max_iters=1000))):
    ranker = make()
    t = timed(lambda: ranker.propagate(adj, F))
    info = [c for batch in ranker.last_batches for c in batch]
    report[name] = dict(wall_ms=[round(x, 3) for x in t], median=round(float(np.median(t)), 3), steps=max(c["spmv"] for c in info),
                        loop_ms=round(sum(batch[0]["loop_ms"] for batch in ranker.last_batches), 3))
norms = feats.sum(axis=0).astype(np.float64)
P = DeviceMatrix.from_host(feats / norms)
R = DeviceMatrix.empty(n, b)
results = (L.LoopResult * b)()
sc = (C.c_double * b)(*norms)
cfg = L.LoopCfg(alpha=-7.0, use_quotient=1, err_kind=1, tol=1e-6, max_iters=1000, end_modulo=1, out_scale=1.0, in_norm=0.0, start_from_p=1)
alphas = (C.c_double * b)(*np.linspace(0.5, 0.95, b))
t = timed(lambda: L.check(L.entry("pgh_ppr_run_batch_mixed")(g._h, P._h, R._h, C.byref(cfg), alphas, sc, results)))
report["mixed_ppr"] = dict(wall_ms=[round(x, 3) for x in t], median=round(float(np.median(t)), 3), steps=max(r.spmv_count for r in results))
terms = 30
coeffs = np.zeros((terms, b))
for j in range(b):
    tt, c = 1 + j % 7, 1.0
    for k in range(terms):
        coeffs[k, j] = c
        c = c * tt / (k + 2)
cfg2 = L.LoopCfg(alpha=-7.0, use_quotient=0, err_kind=3, tol=1e-6, max_iters=terms + 1, end_modulo=1, out_scale=1.0, in_norm=0.0, start_from_p=1)
t = timed(lambda: L.check(L.entry("pgh_poly_run_batch_mixed")(g._h, P._h, coeffs.ctypes.data_as(C.c_void_p), terms, R._h, C.byref(cfg2), sc, results)))
report["mixed_poly"] = dict(wall_ms=[round(x, 3) for x in t], median=round(float(np.median(t)), 3), steps=max(r.spmv_count for r in results))
K = 10
a, bb, cc = (C.c_double * K)(*[0.9] * K), (C.c_double * K)(*[0.1] * K), (C.c_double * (K + 1))(*([0.0] * K + [1.0]))
ms = C.c_double(0.0)
run = lambda: L.entry("pgh_linear_run_batch")(g._h, P._h, 1.0, K, a, bb, cc, R._h, 0.5, 77, 1, C.byref(ms))
status = run()
if status == 0:
    t = timed(lambda: L.check(run()))
    report["linear_dropout"] = dict(wall_ms=[round(x, 3) for x in t], median=round(float(np.median(t)), 3), steps=K, loop_ms=round(ms.value, 3))
else:
    report["linear_dropout"] = dict(status=status, error=(L.lib().pgh_last_error() or b"").decode())
print(json.dumps(report), flush=True)
