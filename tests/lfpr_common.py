"""Shared by tests/test_lfpr_host.py and tests/test_gpu_lfpr.py: the cases of tests/golden/golden_lfpr.npz (make_golden_lfpr.py) and how
one of them is run through pg.LFPR."""
import os

import numpy as np

import cases
from parity_common import rel_linf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = ["er10k", "rmat12_sym", "rmat10_dir", "weighted300"]
REDISTRIBUTORS = ["uniform", "original", "heat"]
LFPR = dict(alpha=0.85, tol=1e-6, max_iters=1000)
BAR = 1e-6                                   # the project's bar; the generator's f32 evaluation stays below 4.2e-7
TIGHT = ("er10k", "uniform")                 # the case the fixture also holds at tol=1e-9

_fixture = None
_graphs = {}


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = np.load(os.path.join(ROOT, "tests", "golden", "golden_lfpr.npz"))
    return _fixture


def graph_of(key):
    if key not in _graphs:
        _graphs[key] = cases.GRAPHS[key]()
    return _graphs[key]


def redistributor(pg, name):
    return {"uniform": None, "original": "original", "heat": pg.HeatKernel(t=3)}[name]


class Case:
    def __init__(self, pg, key, members=None):
        A, directed, p = graph_of(key)
        self.pg, self.key, self.n = pg, key, A.shape[0]
        self.graph = pg.AdjacencyWrapper(A, directed=directed)
        self.seeds = {int(v): float(p[v]) for v in np.flatnonzero(p)}
        members = fixture()[f"{key}/sensitive"] if members is None else members
        self.sensitive = {int(v): 1.0 for v in members}

    def run(self, name, **kwargs):
        """(the filter, its ranks in f64) of LFPR(redistributor `name`) with the fixture's parameters, overridden by kwargs."""
        pg = self.pg
        algo = pg.LFPR(redistributor=redistributor(pg, name), **{**LFPR, **kwargs})
        ranks = algo.rank(self.graph, pg.to_signal(self.graph, self.seeds), sensitive=pg.to_signal(self.graph, self.sensitive))
        return algo, np.asarray(ranks.np, dtype=np.float64)

    def check(self, name, **kwargs):
        fx = fixture()
        algo, got = self.run(name, **kwargs)
        want = fx[f"{self.key}/{name}/ranks"]
        worst = rel_linf(got, want)
        print(self.key, name, kwargs, "rel-Linf", worst, "iterations", algo.convergence.iteration, "reference", int(fx[f"{self.key}/{name}/iters"]))
        assert worst <= BAR, (self.key, name, worst)
        assert algo.convergence.iteration == int(fx[f"{self.key}/{name}/iters"])
        return algo, got


# ---- include/pgh_lfpr.h in numpy f64, from f32 operands: what the GPU kernels are compared with, and (numpy_entries) stand-ins for the
# two entries that let the fused loop of pg.LFPR run on the host test double
def setup_reference(s, R, B, o, phi):
    """(d, dR, dB, xR, xB in f64 before the store's rounding) of pgh_lfpr_setup; `o` None = no `original`."""
    s, R, B = (np.asarray(v, dtype=np.float64) for v in (s, R, B))
    o = np.ones_like(s) if o is None else np.asarray(o, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_r, inv_b = np.where(R != 0, 1.0 / R, 0.0), np.where(B != 0, 1.0 / B, 0.0)
    case1 = R < phi * (R + B)
    case2 = (~case1) & (R != 0)
    case3 = (~case1) & (~case2)
    d = np.where(case1, inv_b * (1 - phi), np.where(case2, inv_r * phi, 1.0))
    dR = np.where(case1, phi - (1 - phi) * inv_b * R, np.where(case3, phi, 0.0))
    dB = np.where(case2, (1 - phi) - phi * inv_r * B, np.where(case3, 1 - phi, 0.0))
    return d, dR, dB, o * s, o * (1 - s)


def close_sums(y, x, x_scale, d, dR, dB, y_scale, linf):
    """The five sums of pgh_lfpr_close over the STORED y (f32 arrays in, f64 arithmetic)."""
    y, x, dR, dB = (np.asarray(v, dtype=np.float64) for v in (y, x, dR, dB))
    t = y * y_scale - x * x_scale
    return [float(y.sum()), float((y * dR).sum()), float((y * dB).sum()), float(np.abs(t).max() if linf else np.abs(t).sum()),
            float((np.sign(t) * y).sum())]


def numpy_entries(lib):
    """{name: callable} with the signatures of include/pgh_lfpr.h, evaluated in numpy through the vector transfers of `lib`."""
    import ctypes as C

    def down(h):
        out = np.empty(lib.pgh_vec_len(h), dtype=np.float32)
        assert lib.pgh_vec_d2h_f32(h, out.ctypes.data_as(C.c_void_p), len(out)) == 0
        return out

    def up(h, values):
        values = np.ascontiguousarray(values, dtype=np.float32)
        assert lib.pgh_vec_h2d_f32(h, values.ctypes.data_as(C.c_void_p), len(values)) == 0

    def setup(s, R, B, o, phi, d, dR, dB, xR, xB, sums):
        made = [np.float32(v) for v in setup_reference(down(s), down(R), down(B), None if o is None else down(o), phi)]
        for h, values in zip((d, dR, dB, xR, xB), made):
            up(h, values)
        sums[0], sums[1] = float(made[3].astype(np.float64).sum()), float(made[4].astype(np.float64).sum())
        return 0

    def close(y0, x, x_scale, xR, xB, d, dR, dB, cR, cB, y_scale, kind, y, u, sums):
        f = lambda h: down(h).astype(np.float64)             # noqa: E731
        stored = np.float32(f(y0) + cR * f(xR) + cB * f(xB))
        got = close_sums(stored, down(x), x_scale, down(d), down(dR), down(dB), y_scale, kind == 2)
        up(y, stored)
        up(u, np.float32(stored.astype(np.float64) * f(d)))
        for k in range(5):
            sums[k] = got[k]
        return 0
    return dict(pgh_lfpr_setup=setup, pgh_lfpr_close=close)
