"""DEV-CONTAINER-ONLY: fixtures of the locally fair PageRank (tests/test_lfpr_host.py, tests/test_gpu_lfpr.py) from the reference,
imported read-only with the `wget` shim of SURVEY.md 8c under its numpy backend.  Output: tests/golden/golden_lfpr.npz.

Per graph of cases.GRAPHS (er10k, rmat12_sym, rmat10_dir, weighted300), with the graph's seeds as the personalization and
default_rng(300).choice(n, n // 5, replace=False) as the sensitive group, LFPR(alpha=0.85, tol=1e-6, max_iters=1000) with
redistributor None ("uniform"), "original" and pg.HeatKernel(t=3) ("heat"):
  <graph>/sensitive              the sensitive nodes (sorted)
  <graph>/<redistributor>/ranks  the reference's f64 rank vector
  <graph>/<redistributor>/iters  the convergence manager's final iteration count
  <graph>/original/inner         the count the inner col-normalised PageRank leaves in the shared manager
and one run at tol=1e-9 (TIGHT below): .../ranks_tol1e-9, and .../f32_rel_linf_tol1e-9 = the rel-Linf against it of the f32 evaluation.

Every case is ASSERTED to meet the bars of the tests with a numpy evaluation of the engine's fused route that keeps f32 storage and
f64 sums (`evaluate`): rel-Linf <= 1e-6 against the reference's vector and the same iteration count.

Run:  PYGRANK_REFERENCE=<checkout of the reference> python tests/golden/make_golden_lfpr.py
"""
import os
import sys
import tempfile
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
os.environ["pygrankBackend"] = "numpy"
os.environ["HOME"] = tempfile.mkdtemp(prefix="pgh_golden_home_")   # import writes ~/.pygrank/config.json
sys.dont_write_bytecode = True
sys.modules["wget"] = types.ModuleType("wget")                      # pygrank/benchmarks/download.py:3
sys.path.insert(0, os.environ["PYGRANK_REFERENCE"])

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import pygrank as pg  # noqa: E402

import cases  # noqa: E402

ALPHA = 0.85
LFPR = dict(alpha=ALPHA, tol=1e-6, max_iters=1000)
GRAPHS = ["er10k", "rmat12_sym", "rmat10_dir", "weighted300"]
TIGHT = ("er10k", "uniform", 1e-9)
BAR = 1e-6


def redistributor(name):
    return {"uniform": None, "original": "original", "heat": pg.HeatKernel(t=3)}[name]


def evaluate(A, p, s, original, tol, max_iters=1000):
    """The fused route in numpy: one raw graph, y0 = alpha x_scale W^T (d x) + (1 - alpha) p, then the close pass; every vector is
    rounded to f32 where the engine stores it, every sum is f64.  Returns (ranks in f64, the outer loop's has_converged calls)."""
    W = sp.csr_matrix(A).astype(np.float64)
    n = W.shape[0]
    f32 = lambda v: np.asarray(v, dtype=np.float32)                      # noqa: E731
    f64 = lambda v: np.asarray(v, dtype=np.float64)                      # noqa: E731
    norm = float(np.abs(p).sum())
    s, p = f32(s), f32(f64(f32(p)) / norm)
    phi = float(f64(s).sum()) / n
    R, B = f64(f32(W.T @ f64(s))), f64(f32(W.T @ (1 - f64(s))))
    case1 = R < phi * (R + B)
    case2 = (~case1) & (R != 0)
    case3 = (~case1) & (~case2)
    inv = lambda v: np.where(v != 0, 1.0 / np.where(v != 0, v, 1), 0.0)  # noqa: E731
    d = f32(np.where(case1, inv(B) * (1 - phi), np.where(case2, inv(R) * phi, 1.0)))
    dR = f32(np.where(case1, phi - (1 - phi) * inv(B) * R, np.where(case3, phi, 0.0)))
    dB = f32(np.where(case2, (1 - phi) - phi * inv(R) * B, np.where(case3, 1 - phi, 0.0)))
    o = np.ones(n) if original is None else f64(f32(original))
    xR, xB = f32(o * f64(s)), f32(o * (1 - f64(s)))
    sum_r, sum_b = float(f64(xR).sum()), float(f64(xB).sum())
    div = lambda a, b: a / b if b != 0 else 0.0                          # noqa: E731
    x, x_scale = p.copy(), 1.0
    u = f32(f64(x) * f64(d))
    delta_r, delta_b = float(f64(x) @ f64(dR)), float(f64(x) @ f64(dB))
    calls = 1
    while True:
        y0 = f32(ALPHA * x_scale * (W.T @ f64(u)) + (1 - ALPHA) * f64(p))
        cR, cB = ALPHA * div(delta_r, sum_r), ALPHA * div(delta_b, sum_b)
        y = f32(f64(y0) + cR * f64(xR) + cB * f64(xB))
        u = f32(f64(y) * f64(d))
        scale = div(1.0, float(f64(y).sum()))
        err = float(np.abs(f64(y) * scale - f64(x) * x_scale).sum()) / n
        delta_r, delta_b = scale * float(f64(y) @ f64(dR)), scale * float(f64(y) @ f64(dB))
        x, x_scale = y, scale
        calls += 1
        if calls >= max_iters or err <= max(tol, float(np.finfo(np.float32).eps)):
            break
    out = f64(f32(f64(x) * x_scale))
    out = f64(f32(out - f64(p) * (1 - ALPHA)))
    return f64(f32(out * norm)), calls


def rel_linf(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def main():
    warnings.simplefilter("ignore")
    out = {}
    for key in GRAPHS:
        A, directed, p = cases.GRAPHS[key]()
        n = A.shape[0]
        graph = pg.AdjacencyWrapper(A, directed=directed)
        signal = pg.to_signal(graph, {int(v): float(p[v]) for v in np.flatnonzero(p)})
        members = np.sort(np.random.default_rng(300).choice(n, n // 5, replace=False))
        s = np.zeros(n)
        s[members] = 1
        sensitive = pg.to_signal(graph, {int(v): 1.0 for v in members})
        out[f"{key}/sensitive"] = members.astype(np.int32)
        for name in ("uniform", "original", "heat"):
            runs = [LFPR["tol"]] + ([TIGHT[2]] if (key, name) == TIGHT[:2] else [])
            for tol in runs:
                algo = pg.LFPR(redistributor=redistributor(name), **dict(LFPR, tol=tol))
                ranks = np.asarray(algo.rank(graph, signal, sensitive=sensitive).np, dtype=np.float64)
                total = int(algo.convergence.iteration)
                inner, original = 0, None
                if name == "original":
                    base = pg.PageRank(alpha=ALPHA, tol=tol, max_iters=1000, normalization="col")
                    original = np.asarray(base.rank(graph, signal).np, dtype=np.float64) / float(np.abs(p).sum())
                    inner = int(base.convergence.iteration)
                elif name == "heat":
                    original = np.asarray(redistributor(name)(pg.to_signal(graph, signal.np / np.abs(signal.np).sum())).np, dtype=np.float64)
                got, calls = evaluate(A, p, s, original, tol)
                worst = rel_linf(got, ranks)
                print(key, name, tol, "iterations", total, "inner", inner, "| f32 evaluation: rel-Linf", worst, "calls", calls)
                if tol == LFPR["tol"]:
                    assert worst <= BAR and calls == total - inner, (key, name, worst, calls, total, inner)
                    out[f"{key}/{name}/ranks"] = ranks
                    out[f"{key}/{name}/iters"] = np.int64(total)
                    if name == "original":
                        out[f"{key}/{name}/inner"] = np.int64(inner)
                else:
                    out[f"{key}/{name}/ranks_tol1e-9"] = ranks
                    out[f"{key}/{name}/f32_rel_linf_tol1e-9"] = np.float64(worst)
    path = os.path.join(HERE, "golden_lfpr.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
