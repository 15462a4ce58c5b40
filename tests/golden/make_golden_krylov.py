"""DEV-CONTAINER-ONLY: fixtures of the Krylov-space filters (tests/test_krylov_host.py, tests/test_gpu_krylov.py) from the reference,
imported read-only as in make_golden_ranking.py (numpy backend, the `wget` shim; the numpy engine's to_primitive, np.array(obj,
copy=False), replaced by np.asarray).  Output: tests/golden/golden_krylov.npz.

Per case of tests/krylov_common.py:CASES (graph, normalization, filter, krylov_dims, tol; max_iters 1000), with the graph's seeds as the
personalization:
  <case>/ranks   the reference's f64 rank vector          <case>/iters   the convergence manager's final iteration count
  <case>/bound   krylov_error_bound of the case           <case>/H       the reference's k x k matrix
  <case>/V       the reference's basis, only for the cases of krylov_common.STORED_V
  <case>/emu_rel the rel-Linf of the f32 evaluation below against <case>/ranks
  <case>/emu_H, /emu_V, /emu_orth  (up to 10 dimensions) max |H - H_ref|, max |V - V_ref| and max |V^T V - I| of that evaluation: the
                 tests allow the engine `factor` (= 8) times these, since the device only adds another summation order on top of the
                 same storage rounding
and the raising case path12/bound/<dims>, path12/message/<dims> for networkx.path_graph(12), personalization {0: 1}, symmetric.

Every case is ASSERTED to meet the bars of the tests with a numpy evaluation of the engine's fused route (`emulate`): the Lanczos
vectors stored in f32, every sum in f64, the deferred scales 1 / |r_j|, the f32 divisors of pgh_mat_div_cols, the residuals from
V @ d_t, the ranks rounded to f32 -- ranks within rel-Linf 1e-6 of the reference, equal iteration counts, the bound on the same side of
0.01.  A case that fails these with the reference alone is to be replaced, not the bar loosened.

Run:  PYGRANK_REFERENCE=<checkout of the reference> python tests/golden/make_golden_krylov.py
"""
import importlib
import os
import sys
import tempfile
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ["pygrankBackend"] = "numpy"
os.environ["HOME"] = tempfile.mkdtemp(prefix="pgh_golden_home_")   # import writes ~/.pygrank/config.json
sys.dont_write_bytecode = True
sys.modules["wget"] = types.ModuleType("wget")                      # pygrank/benchmarks/download.py:3
sys.path.insert(0, os.environ["PYGRANK_REFERENCE"])

import numpy as np  # noqa: E402
import pygrank as pg  # noqa: E402
import pygrank.core.backend as reference_backend  # noqa: E402

import krylov_common as kc  # noqa: E402

_ENGINE = importlib.import_module("pygrank.core.backend.numpy")
_ENGINE.to_primitive = np.asarray                                   # what np.array(obj, copy=False) meant before numpy 2 refused it
reference_backend.load_backend("numpy")

f32 = lambda v: np.asarray(v, dtype=np.float32)                     # noqa: E731
f64 = lambda v: np.asarray(v, dtype=np.float64)                     # noqa: E731


def reference_filter(name):
    _, normalization, cls, params, dims, tol = kc.CASES[name]
    return getattr(pg, cls)(krylov_dims=dims, normalization=normalization, tol=tol, max_iters=kc.MAX_ITERS, **params)


def emulate(name, M, p):
    """The engine's fused route in numpy -> (ranks f64, has_converged calls, bound, V f64 of the stored f32 slab, H)."""
    _, _, _, _, k, tol = kc.CASES[name]
    n = len(p)
    MT = getattr(M, "array", M).T.tocsr().astype(np.float64)         # conv(x, M) = x @ M = M^T x
    MT.data = f64(f32(MT.data))                                      # the engine stores the operator's values / scales in f32
    r = f32(p)
    p_norm = float((f64(r) ** 2).sum()) ** 0.5
    s, previous, previous_s = 1.0 / p_norm, None, 0.0
    slab = np.zeros((n, k), dtype=np.float32)
    slab[:, 0] = r
    first, alphas, norms, divisors, w0 = r, [], [], [p_norm], None
    for j in range(k):
        m = 2.0 ** round(np.log2(s))                                 # the product's multiplier: a power of two, exact in f32 ...
        rho = s / m                                                  # ... and the rest of the scale stays a host scalar
        terms = MT.copy()
        terms.data = f64(f32(MT.data) * r[MT.indices])               # f32 products (oracle/host_abi.cpp row_dot), an f64 row sum,
        w = f32(m * f64(f32(np.asarray(terms.sum(axis=1)).ravel())))  # stored as f32: w' = m M^T r; conv(v_j) = rho w'
        if j == 0:
            w0 = f64(w) * rho
        a = s * rho * float((f64(r) * f64(w)).sum())
        out = f64(w) - (a * s / rho) * f64(r)
        if previous is not None:
            out = out - (norms[j - 1] * previous_s / rho) * f64(previous)
        out = f32(out)
        raw_norm = float((f64(out) ** 2).sum()) ** 0.5
        alphas.append(a)
        norms.append(rho * raw_norm)
        if j == k - 1:
            break
        slab[:, j + 1] = out
        divisors.append(raw_norm)
        previous, previous_s, r, s = r, s, out, 1.0 / raw_norm
    V = f64(slab / f32(divisors)[None, :])                           # k_mat_div_cols: an f32 quotient
    H = np.diag(alphas) + np.diag(norms[1:], -1) + np.diag(norms[1:], 1)
    unit = np.zeros(k)
    unit[0] = 1.0
    bound = max(float(np.abs(f64(f32(V @ unit)) - f64(first) / p_norm).sum()) / n, float(np.abs(f64(f32(V @ H[:, 0])) - f64(w0)).sum()) / n)
    # the filter's loop on k x k matrices with the reference's own _coefficient and _recursion, the residuals from V @ d_t
    algo = reference_filter(name)
    algo.coefficient = None
    algo.prev_term = 0
    result, power = H * 0, np.eye(k)
    before = unit * p_norm
    tolerance = max(tol, float(np.finfo(np.float64).eps))            # the change V d_t is taken from d_t itself: no fp32-eps clamp
    calls = 1
    while True:
        if calls >= kc.MAX_ITERS:
            raise Exception("the emulation ran out of iterations")
        algo.convergence.iteration = calls
        algo.coefficient = algo._coefficient(algo.coefficient)
        result, power = algo._recursion(result, power, algo.coefficient)
        power = power @ H
        now = f64(result)[:, 0].copy()
        error = float(np.abs(V @ (now - before)).sum()) / n
        before = now
        calls += 1
        if error <= tolerance:
            break
    return f64(f32(V @ before)), calls, bound, V, H


def main():
    warnings.simplefilter("ignore")
    out = dict(factor=np.float64(kc.FACTOR))
    for name, (key, normalization, _, _, k, tol) in kc.CASES.items():
        A, directed, p = kc.graph_of(key)
        graph = pg.AdjacencyWrapper(A, directed=directed)
        signal = pg.to_signal(graph, kc.seeds_of(key))
        l1 = float(np.abs(signal.np).sum())
        algo = reference_filter(name)
        ranks = f64(algo.rank(graph, signal).np)
        M = pg.preprocessor(normalization=normalization)(graph)
        normalised = f64(signal.np) / l1
        V_ref, H_ref = pg.krylov_base(M, normalised, k)
        V_ref, H_ref = f64(V_ref), f64(H_ref)
        bound_ref = float(pg.krylov_error_bound(V_ref, H_ref, M, normalised))
        got, calls, bound, V, H = emulate(name, M, normalised)
        got = f64(f32(got * l1))                                    # preserve_norm rides on the way out of the id space
        worst = float(np.abs(got - ranks).max() / np.abs(ranks).max())
        print(name, "iters", algo.convergence.iteration, "emulated", calls, "rel-Linf", worst, "bound", bound_ref, "emulated", bound)
        assert worst <= kc.BAR, (name, worst)
        assert calls == algo.convergence.iteration, (name, calls, algo.convergence.iteration)
        assert (bound > 0.01) == (bound_ref > 0.01) and bound_ref <= 0.01, (name, bound, bound_ref)
        out[name + "/ranks"], out[name + "/iters"], out[name + "/bound"] = ranks, np.int64(algo.convergence.iteration), np.float64(bound_ref)
        out[name + "/H"], out[name + "/emu_rel"] = H_ref, np.float64(worst)
        if k <= kc.BASIS_DIMS:
            devs = dict(emu_H=np.abs(H - H_ref).max(), emu_V=np.abs(V - V_ref).max(), emu_orth=np.abs(V.T @ V - np.eye(k)).max())
            print("   ", {what: float(value) for what, value in devs.items()}, "reference orth", float(np.abs(V_ref.T @ V_ref - np.eye(k)).max()))
            for what, value in devs.items():
                out[name + "/" + what] = np.float64(value)
        if name in kc.STORED_V:
            out[name + "/V"] = V_ref
    graph = kc.path_graph(12)
    for dims in kc.RAISING_DIMS:
        algo = pg.HeatKernel(t=3, krylov_dims=dims, normalization="symmetric", tol=1e-6, max_iters=kc.MAX_ITERS)
        try:
            algo.rank(graph, {0: 1})
            raise AssertionError("the reference did not raise on path_graph(12) at " + str(dims) + " dimensions")
        except Exception as e:
            if isinstance(e, AssertionError):
                raise
            message = str(e)
        bound = float(message.split("relative error ")[1].split(" ")[0])
        print("path12", dims, message)
        assert bound > 0.01
        out[f"path12/bound/{dims}"], out[f"path12/message/{dims}"] = np.float64(bound), np.array(message)
    path = os.path.join(HERE, "golden_krylov.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
