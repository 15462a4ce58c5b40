"""Child process of tests/test_gpu_loop_switches.py: every fused single-vector loop of the engine under ONE set of the read-once
switches (PGH_POLL, PGH_DEFER_CLOSE, PGH_FUSED_RES, PGH_FIRST_PRED, PGH_PUBLISHED_STATE), which this process inherits from its
environment -- the engine reads them once per process, so each set needs a process of its own.

    python tests/loop_switch_worker.py <cache dir> <label>

Graphs (the smallest shapes at which each route exists, tests/test_gpu_seed_push.py and tests/kernel_checks.py):
  small10    RMAT scale 10 under the defaults: a step is the block partial sums + the one-workgroup tail (k_small_tail)
  general10  the same graph run with PGH_SMALL_TAIL=0: the general launch sequence, no cold image
  cold16     RMAT scale 16 uploaded with PGH_PB=1 PGH_PB_FORCE=1: the smallest size with a cold image -- the in-kernel residual, the
             first-step prediction, the deferred close into k_pb_finish
  csr10      RMAT scale 10 uploaded with PGH_FORMAT=csr: the row-major branch of every loop

Every run is held to oracle/ref_loops.py on the engine's own stored matrix (download_transposed): rel-Linf <= 1e-6 and equal
iteration counts, the bounds of the existing parity tests; every run is done twice and must return the same bits.  The oracle's
results do not depend on the switches: the first child leaves them in <cache dir>, the later ones read them.

One line per run on stdout ("<label> <graph> <case> iterations=... flags=... spmv=... rel=..."), the failed checks behind them,
exit status 1 if there was one."""
import contextlib
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_loops as orc, rmat_np      # noqa: E402

UPLOAD_ENV = ("PGH_PB", "PGH_PB_FORCE", "PGH_FORMAT", "PGH_SMALL_TAIL")
ALPHA = 0.85
EPS32 = float(np.finfo(np.float32).eps)
FAILURES = []


@contextlib.contextmanager
def env(**values):
    saved = {k: os.environ.get(k) for k in UPLOAD_ENV}
    try:
        for k in UPLOAD_ENV:
            os.environ.pop(k, None)
        os.environ.update(values)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def rel(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def adjacency(g):
    from pygrank_amd.preprocessing import Adjacency
    from pygrank_amd.signals import _IdentityMap
    adj = Adjacency(g)
    adj._pygrank_preprocessed = {"hip": adj}
    adj._pygrank_node2id = _IdentityMap(g.shape[0])
    adj.is_directed = lambda: True
    return adj


class Graph:
    def __init__(self, name, scale, upload, run):
        from pygrank_amd.device import DeviceGraph
        A = rmat_np.rmat_csr(scale, 16, seed=2)
        data = np.ones(A.nnz)                                    # multiplicities 1, 2 and 3: the value-free image takes them
        data[::7], data[::31] = 2.0, 3.0
        A = sp.csr_array((data, A.indices, A.indptr), shape=A.shape)
        with env(**upload):
            self.g = DeviceGraph.from_adjacency(A, "col")
        self.name, self.run_env, self.fmt = name, run, self.g.format()
        self.adj = adjacency(self.g)
        self.M = sp.csr_array(self.g.download_transposed().astype(np.float64)).T
        self.n = A.shape[0]
        p = np.zeros(self.n)
        p[np.sort(np.random.default_rng(1).choice(np.flatnonzero(np.diff(A.indptr) > 0), 100, replace=False))] = 1.0
        self.p = p
        self.row_major = "row-major" in self.fmt


def check(ok, what):
    if not ok:
        FAILURES.append(what)
        print("FAILED: " + what, flush=True)


def quiet(**kw):
    """A stopping rule that lets a run end at max_iters without raising (convergence.py:86-89 with no exception type)."""
    import pygrank_amd as pg
    return pg.ConvergenceManager(iter_exception=None, **kw)


def cases(pg, G):
    """(case, ranker factory, rank() keywords, oracle call) of one graph."""
    l1 = dict(error_type=pg.L1, tol=1e-6, max_iters=500)
    ol1 = dict(error_type="l1", tol=1e-6, max_iters=500)
    warm = np.full(G.n, 1.0 / G.n)
    out = [
        ("ppr", lambda: pg.PageRank(ALPHA, **l1), {}, lambda p: orc.pagerank(G.M, p, alpha=ALPHA, **ol1)),
        ("ppr_warm", lambda: pg.PageRank(ALPHA, **l1), dict(warm_start=warm),
         lambda p: orc.pagerank(G.M, p, alpha=ALPHA, warm_start=warm, **ol1)),
        ("ppr_max_iters", lambda: pg.PageRank(ALPHA, convergence=quiet(error_type=pg.L1, tol=1e-6, max_iters=6)), {},
         lambda p: orc.pagerank(G.M, p, alpha=ALPHA, error_type="l1", tol=1e-6, max_iters=6, raise_on_max=False)),
        ("ppr_modulo3", lambda: pg.PageRank(ALPHA, end_modulo=3, **l1), {}, lambda p: orc.pagerank(G.M, p, alpha=ALPHA, end_modulo=3, **ol1)),
        # tol 1e-9: the f64-iterate route on the blocked images.  The row-major graph declines it (filters._f64_image_usable) and runs
        # the f32 loop with the tolerance clamped at fp32 eps (convergence.py:101)
        ("ppr_tol1e-9", lambda: pg.PageRank(ALPHA, error_type=pg.L1, tol=1e-9, max_iters=500), {},
         lambda p: orc.pagerank(G.M, p, alpha=ALPHA, error_type="l1", tol=1e-9, max_iters=500, **(dict(eps=EPS32) if G.row_major else {}))),
        ("absorbing", lambda: pg.AbsorbingWalks(ALPHA, **l1), {}, lambda p: orc.absorbing_walks(G.M, p, alpha=ALPHA, **ol1)),
        ("sarw", lambda: pg.SymmetricAbsorbingRandomWalks(**l1), {}, lambda p: orc.symmetric_absorbing_walks(G.M, p, **ol1)),
    ]
    for form in ("taylor", "chebyshev"):
        out.append(("heat_" + form, lambda form=form: pg.HeatKernel(t=5, coefficient_type=form, error_type=pg.L1, tol=1e-6, max_iters=100), {},
                    lambda p, form=form: orc.heat_kernel(G.M, p, t=5, coefficient_type=form, error_type="l1", tol=1e-6, max_iters=100)))
        for m in (1, 2, 3):                                      # the early exits and the host's mirror of iteration 2
            out.append((f"heat_{form}_max_iters{m}",
                        lambda form=form, m=m: pg.HeatKernel(t=5, coefficient_type=form, convergence=quiet(error_type=pg.L1, tol=1e-6, max_iters=m)), {},
                        lambda p, form=form, m=m: orc.heat_kernel(G.M, p, t=5, coefficient_type=form, error_type="l1", tol=1e-6, max_iters=m,
                                                                  raise_on_max=False)))
    return out


def reference(cache, key, compute):
    path = os.path.join(cache, key.replace("/", "_") + ".npz")
    if os.path.exists(path):
        z = np.load(path)
        return z["ranks"], int(z["iterations"])
    want, iters = compute()
    np.savez(path + ".tmp.npz", ranks=want, iterations=iters)
    os.replace(path + ".tmp.npz", path)
    return want, iters


def run_case(label, cache, G, case, make, kw, oracle, p):
    runs = []
    with env(**G.run_env):
        for _ in range(2):
            ranker = make()
            got = np.asarray(ranker.rank(G.adj, p.copy(), **kw).np, dtype=np.float64)
            runs.append((got, int(ranker.convergence.iteration), dict(getattr(ranker, "last_loop", None) or {})))
    (got, iters, loop), (again, iters2, _) = runs
    want, want_iters = reference(cache, f"{G.name}/{case}", lambda: oracle(p))
    err = rel(got, want) if np.any(want) else float(np.max(np.abs(got)))
    print(f"{label} {G.name} {case} iterations={iters} oracle={want_iters} flags={loop.get('flags')} spmv={loop.get('spmv')} "
          f"converged={loop.get('converged')} rel={err:.3e}", flush=True)
    where = f"{label} {G.name} {case}"
    check(iters == want_iters, f"{where}: {iters} iterations, the oracle {want_iters}")
    check(err <= 1e-6, f"{where}: rel-Linf {err:.3e}")
    check(iters2 == iters and np.array_equal(again, got), f"{where}: the second run differs from the first")
    return loop


def main():
    cache, label = sys.argv[1], sys.argv[2]
    os.makedirs(cache, exist_ok=True)
    import pygrank_amd as pg
    from pygrank_amd import _lib
    pg.load_backend("hip")
    assert _lib.runtime_name().startswith("hip:")
    fused_on = os.environ.get("PGH_FUSED_RES", "1") != "0"
    defaults = label == "defaults"
    small = Graph("small10", 10, {}, {})
    general = Graph("general10", 10, {}, dict(PGH_SMALL_TAIL="0"))
    cold = Graph("cold16", 16, dict(PGH_PB="1", PGH_PB_FORCE="1"), {})
    csr = Graph("csr10", 10, dict(PGH_FORMAT="csr"), {})
    check("propagation-blocking image" in cold.fmt, "cold16 has no cold image: " + cold.fmt)
    check("propagation-blocking image" not in small.fmt and not small.row_major, "small10: " + small.fmt)
    check(csr.row_major, "csr10 is not row-major: " + csr.fmt)
    for G in (small, general, cold, csr):
        for case, make, kw, oracle in cases(pg, G):
            loop = run_case(label, cache, G, case, make, kw, oracle, G.p)
            if G is cold and case == "ppr":
                check(bool(loop["flags"] & 2) == fused_on, f"{label} cold16 ppr: flags {loop['flags']}, in-kernel residual expected {fused_on}")
    # a personalization with negative entries (tests/test_gpu_fullsize.py): the in-kernel residual hands one step back
    signed = cold.p.copy()
    signed[np.flatnonzero(signed)[::4]] = -0.25
    l1 = dict(error_type=pg.L1, tol=1e-6, max_iters=1000)
    loop = run_case(label, cache, cold, "ppr_signed", lambda: pg.PageRank(ALPHA, **l1), {},
                    lambda p: orc.pagerank(cold.M, p, alpha=ALPHA, error_type="l1", tol=1e-6, max_iters=1000), signed)
    if fused_on:
        check(loop["flags"] & 1, f"{label} cold16 ppr_signed: never paused, flags {loop['flags']}")
    loop = run_case(label, cache, cold, "ppr_after_signed", lambda: pg.PageRank(ALPHA, **l1), {},
                    lambda p: orc.pagerank(cold.M, p, alpha=ALPHA, error_type="l1", tol=1e-6, max_iters=1000), cold.p)
    if defaults:
        check(loop["flags"] & 7 == 6, f"{label} cold16 ppr_after_signed: flags {loop['flags']}, expected fused from the first step, unpaused")
    print(f"{label}: {len(FAILURES)} failed checks", flush=True)
    return 1 if FAILURES else 0


if __name__ == "__main__":
    sys.exit(main())
