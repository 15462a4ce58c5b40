"""Shared by tests/golden/make_golden_krylov.py, tests/test_krylov_host.py, tests/test_gpu_krylov.py and tests/test_gpu_krylov_kernels.py:
the cases of tests/golden/golden_krylov.npz, how one of them is run through the public API, and include/pgh_krylov.h in numpy."""
import os
import warnings

import numpy as np

import cases
from parity_common import rel_linf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-6                 # ranks, rel-Linf against the reference's f64 run (the bar of the LFPR goldens)
FACTOR = 8                 # bases: at most this many times the deviation the generator's f32 evaluation recorded
BASIS_DIMS = 10            # bases (V, H, V^T V - I) are compared up to this many dimensions only
MAX_ITERS = 1000

# name -> (graph, normalization, filter, its parameters, krylov_dims, tol)
CASES = {
    "er10k/heat3/5": ("er10k", "symmetric", "HeatKernel", dict(t=3), 5, 1e-6),
    "er10k/heat3/10": ("er10k", "symmetric", "HeatKernel", dict(t=3), 10, 1e-6),
    "er10k/heat5cheb/10": ("er10k", "symmetric", "HeatKernel", dict(t=5, coefficient_type="chebyshev"), 10, 1e-6),
    "er10k/pprc/20": ("er10k", "symmetric", "PageRankClosed", dict(alpha=0.85), 20, 1e-6),
    "rmat12_sym/heat3/5": ("rmat12_sym", "symmetric", "HeatKernel", dict(t=3), 5, 1e-6),
    "rmat12_sym/pprc/10": ("rmat12_sym", "symmetric", "PageRankClosed", dict(alpha=0.85), 10, 1e-6),
    "rmat12_sym/heat3tol9/10": ("rmat12_sym", "symmetric", "HeatKernel", dict(t=3), 10, 1e-9),
    "rmat10_dir/heat3/5": ("rmat10_dir", "col", "HeatKernel", dict(t=3), 5, 1e-6),
    "rmat10_dir/heat3/10": ("rmat10_dir", "col", "HeatKernel", dict(t=3), 10, 1e-6),
    "weighted300/heat3/10": ("weighted300", "symmetric", "HeatKernel", dict(t=3), 10, 1e-6),
}
# cases whose V the fixture stores (at 10 dimensions; the 5-dimension basis of the same graph is its prefix)
STORED_V = {"rmat10_dir/heat3/10": ["rmat10_dir/heat3/5"], "weighted300/heat3/10": []}
RAISING_DIMS = (3, 5)      # networkx.path_graph(12), personalization {0: 1}, symmetric: the bound lies above 0.01

_fixture = None
_graphs = {}


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = np.load(os.path.join(ROOT, "tests", "golden", "golden_krylov.npz"))
    return _fixture


def graph_of(key):
    if key not in _graphs:
        _graphs[key] = cases.GRAPHS[key]()
    return _graphs[key]


def path_graph(nodes):
    import networkx as nx
    return nx.path_graph(nodes)


def seeds_of(key):
    p = graph_of(key)[2]
    return {int(v): float(p[v]) for v in np.flatnonzero(p)}


def make_filter(pg, name, **extra):
    _, normalization, cls, params, dims, tol = CASES[name]
    return getattr(pg, cls)(krylov_dims=dims, normalization=normalization, tol=tol, max_iters=MAX_ITERS, **params, **extra)


def run(pg, name, **extra):
    """(the filter, its ranks in f64) of case `name`."""
    key = CASES[name][0]
    A, directed, _ = graph_of(key)
    graph = pg.AdjacencyWrapper(A, directed=directed)
    algo = make_filter(pg, name, **extra)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ranks = algo.rank(graph, pg.to_signal(graph, seeds_of(key)))
    return algo, np.asarray(ranks.np, dtype=np.float64)


def check(pg, name, **extra):
    fx = fixture()
    algo, got = run(pg, name, **extra)
    worst = rel_linf(got, fx[name + "/ranks"])
    print(name, extra, "rel-Linf", worst, "iterations", algo.convergence.iteration, "reference", int(fx[name + "/iters"]), algo.last_loop)
    assert worst <= BAR, (name, worst)
    assert algo.convergence.iteration == int(fx[name + "/iters"])
    return algo, got


def basis_of(pg, name, fused=True):
    """(V, H) as numpy f64 from pg.krylov_base on the case's graph and L1-normalised personalization."""
    key, normalization, _, _, dims, _ = CASES[name]
    A, directed, _ = graph_of(key)
    graph = pg.AdjacencyWrapper(A, directed=directed)
    signal = pg.to_signal(graph, seeds_of(key))
    M = pg.preprocessor(normalization=normalization)(graph)
    p = signal.np / pg.sum(pg.abs(signal.np))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        V, H = pg.krylov_base(M, p, dims, fused=fused)
    return np.asarray(V, dtype=np.float64), np.asarray(H, dtype=np.float64)


def check_basis(pg, name, fused=True):
    """The bounds of the bases: H, V (where the fixture stores it, or its prefix) and V^T V - I at most FACTOR times what the generator's
    f32 evaluation of the engine's route recorded for the case.  Only up to BASIS_DIMS dimensions."""
    fx = fixture()
    dims = CASES[name][4]
    assert dims <= BASIS_DIMS
    V, H = basis_of(pg, name, fused)
    assert V.shape == (graph_of(CASES[name][0])[0].shape[0], dims) and H.shape == (dims, dims)
    h_dev = float(np.abs(H - fx[name + "/H"]).max())
    orth = float(np.abs(V.T @ V - np.eye(dims)).max())
    print(name, "fused" if fused else "primitive", "H", h_dev, "allowed", FACTOR * float(fx[name + "/emu_H"]),
          "orth", orth, "allowed", FACTOR * float(fx[name + "/emu_orth"]))
    assert h_dev <= FACTOR * float(fx[name + "/emu_H"])
    assert orth <= FACTOR * float(fx[name + "/emu_orth"])
    stored = name if name in STORED_V else next((k for k, prefixes in STORED_V.items() if name in prefixes), None)
    if stored is not None:
        v_dev = float(np.abs(V - fx[stored + "/V"][:, :dims]).max())
        print(name, "V", v_dev, "allowed", FACTOR * float(fx[name + "/emu_V"]))
        assert v_dev <= FACTOR * float(fx[name + "/emu_V"])
    return V, H


# ---- include/pgh_krylov.h in numpy f64, from f32 operands: what the GPU kernels are compared with
def close_reference(w, v, a, u, b):
    """(out in f64 before the store's rounding, the cancellation scale |w| + |a v| + |b u|) of pgh_lanczos_close; u None = no third term."""
    w, v = np.asarray(w, dtype=np.float64), np.asarray(v, dtype=np.float64)
    out, scale = w - a * v, np.abs(w) + np.abs(a * v)
    if u is not None:
        u = np.asarray(u, dtype=np.float64)
        out, scale = out - b * u, scale + np.abs(b * u)
    return out, scale


def numpy_entries(lib):
    """{name: callable} with the signatures of include/pgh_krylov.h, evaluated in numpy through the transfers of `lib`: stand-ins that
    let the fused route's host side run on the host test double."""
    import ctypes as C

    def down(h):
        out = np.empty(lib.pgh_vec_len(h), dtype=np.float32)
        assert lib.pgh_vec_d2h_f32(h, out.ctypes.data_as(C.c_void_p), len(out)) == 0
        return out

    def up(h, values):
        values = np.ascontiguousarray(values, dtype=np.float32)
        assert lib.pgh_vec_h2d_f32(h, values.ctypes.data_as(C.c_void_p), len(values)) == 0

    def slab_down(h):
        n, b = C.c_int64(), C.c_int32()
        assert lib.pgh_mat_shape(h, C.byref(n), C.byref(b)) == 0
        out = np.empty((n.value, b.value), dtype=np.float64)
        assert lib.pgh_mat_d2h_f64(h, out.ctypes.data_as(C.c_void_p)) == 0
        return out

    def close(w, v, a, u, b, out, basis, col, sums):
        if not (np.isfinite(a) and np.isfinite(b)):
            return 2
        want, _ = close_reference(down(w), down(v), a, None if u is None else down(u), b)
        stored = np.float32(want)
        up(out, stored)
        if basis is not None:
            assert lib.pgh_mat_set_col(basis, col, out) == 0
        sums[0] = float((stored.astype(np.float64) ** 2).sum())
        sums[1] = float((stored.astype(np.float64) * down(v).astype(np.float64)).sum())
        return 0

    def residuals(basis, deltas, count, probes, abssum, absmax):
        d = np.array([deltas[k] for k in range(count * probes)], dtype=np.float64).reshape(count, probes)
        if not np.all(np.isfinite(d)):
            return 2
        got = residual_reference(slab_down(basis), d)
        for t in range(probes):
            abssum[t], absmax[t] = got[0][t], got[1][t]
        return 0
    return dict(pgh_lanczos_close=close, pgh_krylov_residuals=residuals)


def residual_reference(basis, deltas):
    """(sum_i |r|, max_i |r|, sum_i sum_c |basis delta|, max_i sum_c |basis delta|) per probe of pgh_krylov_residuals, f64."""
    B = np.asarray(basis, dtype=np.float64)[:, :deltas.shape[0]]
    r = np.abs(B @ deltas)
    mags = np.abs(B) @ np.abs(deltas)
    zero = np.zeros(deltas.shape[1])
    if not len(B):
        return zero, zero, zero, zero
    return r.sum(axis=0), r.max(axis=0), mags.sum(axis=0), mags.max(axis=0)
