"""The multi-seed loops under their run switches: PGH_MM_FUSED, PGH_MM_SPARSE, PGH_MM_FIRST_PRED and PGH_MM_AFFINE.
The engine reads all four with getenv on every call, so one process serves every set.

Six switch sets (SETS) x the cases of _build on rmat10_dir at widths 3, 17 and 64 -- one width per lane shape of lanes_per_row, the first
two ending in a partial float4 -- plus a paused batch and a plain PageRank batch on rmat17.  The personalizations are three-seed
columns (and one zero column): the first steps of a run then take the sparse form of the gather pass (non-zero rows x 4 < live rows),
the later ones the dense form.

Every compared column is held to what tests/test_gpu_batch_edges.py holds it to: the fp64 oracle (oracle/ref_loops.py) on the engine's
stored matrix to <= 1e-6 relative L-inf with equal iteration counts, a stop one check apart only under that module's
_stop_margin_ok; zero columns stay exactly zero.  The graph_dropout batch uses the reference and the bound of
test_gpu_gnn.py::test_batched_pagerank_dropout_honours_the_mirrored_words (numpy on the masked stored matrices, 2e-6 * max|want|).
Each oracle result is computed once per (graph, case, width) and shared by the six sets.

The closed-form loops stop on the exact change of an f32 accumulator, which one step's roundings move by up to mass * 2^-24
(tests/test_gpu_mixed_batch.py POLY_RULES): their runs to convergence use that module's L1 tolerance of 2e-4, which the 2 % margin is
wider than.

On top of the references: every case runs twice under its set and returns equal bits and equal (iterations, spmv, flags); flags bit 1
is set on the non-signed L1 PageRank cases exactly when PGH_MM_FUSED is not 0; the signed batch reports its pause (bit 0) exactly when
the residual was fused.  Every test prints `<set> <graph> <case> b=<width> iterations=[...] spmv=[...] flags=[...] rel=<max>`
(profiles/mm_loops/switch_lines_*.log keep those lines of the commit that added the module and of its parent).

Measured on the MI355X: the module takes about 4 s of wall time (252 tests)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import test_gpu_batch_edges as be
import test_gpu_gnn as gnn
import test_gpu_mixed_batch as mb
from oracle import ref_loops as orc
from test_gpu_batch_edges import graphs, pg  # noqa: F401  (module-scoped fixtures: this module gets instances of its own)

pytestmark = pytest.mark.gpu

SWITCHES = ("PGH_MM_FUSED", "PGH_MM_SPARSE", "PGH_MM_FIRST_PRED", "PGH_MM_AFFINE")
SETS = {
    "defaults": {},
    "fused0": {"PGH_MM_FUSED": "0"},
    "sparse0": {"PGH_MM_SPARSE": "0"},
    "first_pred0": {"PGH_MM_FIRST_PRED": "0"},
    "affine1": {"PGH_MM_AFFINE": "1"},
    "fused0_sparse0": {"PGH_MM_FUSED": "0", "PGH_MM_SPARSE": "0"},
}
WIDTHS = (3, 17, 64)
# Rounding two f32 iterates moves their L1 difference by up to 2 * eps32 per unit of mass: 24 % of an L1 tolerance of 1e-6, 0.1 % of 2e-4.
# A column whose f64 residual passes the tolerance more closely than that stops where rounding puts it, in any f32 loop.  The columns
# of this module are drawn so that the oracle's residuals at the stop and at the check before keep that distance from the tolerance
# (as a share of it; a Mabs tolerance counts as n times itself), and never less than 5 %.  The 2 % rule of _stop_margin_ok still
# judges every stop that differs.
def _decided_share(rule, tol, n):
    return max(0.05, 2 * be.EPS32 / (tol * (n if rule == "mabs" else 1)))


POLY_L1 = mb.POLY_RULES["l1"]
PROPAGATE = {
    # case: (family, rule of test_gpu_batch_edges.RULES, extra keywords)
    "ppr_l1": ("pagerank", "l1", {}),
    "ppr_linf": ("pagerank", "linf", {}),
    "ppr_modulo3": ("pagerank", "modulo3", {}),
    "signed": ("pagerank", "l1", {}),
    "heat_iters1": ("heat", "iters1", {}),
    "heat_iters2": ("heat", "iters2", {}),
    "heat_iters3": ("heat", "iters3", {}),
    "heat_converged": ("heat", "l1", dict(tol=POLY_L1["tol"], max_iters=POLY_L1["max_iters"])),
    "absorbing": ("absorbing", "l1", {}),
    "sarw": ("sarw", "default", {}),
}
L1_PPR = ("ppr_l1", "ppr_modulo3", "max_iters2", "mixed_ppr")         # non-signed PageRank under the L1 rule: fused unless switched off
SMALL_CASES = tuple(PROPAGATE) + ("max_iters2", "mixed_ppr", "mixed_poly")
RUNS = ([("rmat10_sym" if case == "sarw" else "rmat10_dir", case, w) for case in SMALL_CASES for w in WIDTHS]
        + [("rmat10_dir", "dropout", 17), ("rmat17", "signed", 17), ("rmat17", "ppr_l1", 64)])


def _three_seeds(G, rng):
    """A non-negative column of three seeds on nodes with edges in both directions, rounded through f32."""
    p = np.zeros(G["n"])
    p[rng.choice(G["live"], 3, replace=False)] = rng.uniform(0.5, 1.5, 3)
    return p.astype(np.float32).astype(np.float64)


def _columns(G, width, seed, ref_of, checked, special=None):
    """-> ([n, width], {j: Ref} for j in checked).  Column 1 is zero, column j of `special` is drawn by special[j](rng), the others by
    _three_seeds.  A checked column is redrawn until its ORACLE run is decided clear of the tolerance (Ref.decided): the draw never looks
    at the engine."""
    rng = np.random.default_rng(seed)
    F, refs = np.zeros((G["n"], width)), {}
    for j in range(width):
        if j == 1:
            continue
        for _ in range(200):
            F[:, j] = (special or {}).get(j, lambda r: _three_seeds(G, r))(rng)
            ref = ref_of(j, F[:, j])
            if j not in checked or ref.decided():
                break
        else:
            raise AssertionError(("no decided column", j))
        if j in checked:
            refs[j] = ref
    return F, refs


class Ref:
    """One column's oracle: the result and the stop under the case's rule (computed on first use), and the iterates by count."""

    def __init__(self, p, oracle, rule, tol, modulo, preserve_norm=True):
        self.p, self.rule, self.tol, self.modulo, self.preserve_norm = p, rule, tol, modulo, preserve_norm
        self.stopped = functools.lru_cache(maxsize=None)(lambda: oracle(p))
        self.after = functools.lru_cache(maxsize=None)(lambda k: oracle(p, error_type="iters", max_iters=k)[0])

    def decided(self):
        """Do the oracle's own residuals at its stopping check and at the check before lie further than _decided_share from the
        tolerance?  (Counting rules: always.)"""
        if self.rule == "iters":
            return True
        delta = _decided_share(self.rule, self.tol, len(self.p))
        scale = (np.abs(self.p).sum() if self.preserve_norm else 1.0) * self.tol
        it = self.stopped()[1]

        def ratio(k):
            d = np.abs(self.after(k) - self.after(k - 1))
            return {"l1": d.sum(), "mabs": d.sum() / len(d), "linf": d.max()}[self.rule] / scale
        return ratio(it) <= 1 - delta and (it - self.modulo < 2 or ratio(it - self.modulo) >= 1 + delta)

    def held(self, col, its, where):
        """-> the column's relative error against the oracle at the engine's stop."""
        want, it = self.stopped()
        if its != it:
            assert self.rule != "iters" and abs(its - it) == self.modulo, where + (its, it)
            ok, want, ratio = be._stop_margin_ok(self.after, self.p, its, it, self.tol, self.rule, self.preserve_norm)
            assert ok, where + (its, it, ratio)
        rel = be._rel(col, want)
        assert rel <= be.BOUND, where + (rel,)
        return rel


def _quiet_two_iterations(pg):
    return pg.PageRank(0.85, convergence=pg.ConvergenceManager(iter_exception=None, error_type=pg.L1, tol=1e-6, max_iters=2))


def _poly_family():
    terms = POLY_L1["max_iters"] - 1
    return [(lambda M, p, **o: orc.heat_kernel(M, p, t=1, **o), mb._schedule(orc.heat_kernel_coefficient(1), terms)),
            (lambda M, p, **o: orc.heat_kernel(M, p, t=3, **o), mb._schedule(orc.heat_kernel_coefficient(3), terms)),
            (lambda M, p, **o: orc.heat_kernel(M, p, t=7, **o), mb._schedule(orc.heat_kernel_coefficient(7), terms)),
            (lambda M, p, **o: orc.pagerank_closed(M, p, alpha=0.85, **o), mb._schedule(orc.pagerank_closed_coefficient(0.85), terms)),
            (lambda M, p, **o: orc.generic_filter(M, p, [1.0, 0.5, 0.25], **o), [1.0, 0.5, 0.25])]


def _from_results(results):
    return [r.iterations for r in results], [r.spmv_count for r in results], [r.flags for r in results]


def _build(pg, G, gkey, case, width):
    """-> (run() -> (out [n, width] f64, iterations, spmv, flags), {column: Ref} of the compared columns, or a callable check(out) -> rel
    for the case with a reference of its own)."""
    M, n = G["M"], G["n"]
    seed = 1000 * WIDTHS.index(width) + len(case)
    checked = set(range(width)) if gkey != "rmat17" else {0, width // 2, width - 1}
    if case in PROPAGATE or case == "max_iters2":
        if case == "max_iters2":
            make, rule, tol, modulo, preserve_norm = (lambda: _quiet_two_iterations(pg)), "iters", 1e-6, 1, True
            oracle = lambda M, p, **o: orc.pagerank(M, p, alpha=0.85, **dict(dict(error_type="iters", max_iters=2, eps=be.EPS32), **o))  # noqa: E731
        else:
            family, rule_name, extra = PROPAGATE[case]
            make, oracle, rule, tol, modulo, preserve_norm = be._make(pg, family, rule_name, **extra)
        special = None
        if case == "signed":                  # the last column is signed, its first iterate holds a negative value: the fused run pauses
            def signed(rng):
                while True:
                    p = be._column("signed", G, rng)
                    if np.any(oracle(M, p, error_type="iters", max_iters=2)[0] < 0):
                        return p
            special = {width - 1: signed}
        F, refs = _columns(G, width, seed, lambda j, p: Ref(p, functools.partial(oracle, M), rule, tol, modulo, preserve_norm), checked, special)

        def run():
            ranker = make()
            out = np.asarray(ranker.propagate(G["adj"], pg.to_primitive(F)), dtype=np.float64)
            assert out.shape == F.shape and len(getattr(ranker, "last_batches", ())) == 1, "the batch route was not taken"
            batch = ranker.last_batches[0]
            return out, [c["iterations"] for c in batch], [c["spmv"] for c in batch], [c["flags"] for c in batch]
        return run, refs
    if case == "mixed_ppr":
        alphas, kw = mb._spread(width), dict(mb.L1, eps=be.EPS32)
        F, refs = _columns(G, width, seed, lambda j, p: Ref(p, lambda q, **o: orc.pagerank(M, q, alpha=alphas[j], **dict(kw, **o)), "l1",
                                                            mb.L1["tol"], 1), checked)

        def run():
            status, out, results = mb._run_ppr(pg, G, F, alphas, mb.L1)
            assert status == 0
            return (out,) + tuple(_from_results(results))
        return run, refs
    if case == "mixed_poly":
        family, kw = _poly_family(), dict(POLY_L1, eps=be.EPS32)
        members = [family[j % len(family)] for j in range(width)]
        F, refs = _columns(G, width, seed, lambda j, p: Ref(p, lambda q, **o: members[j][0](M, q, **dict(kw, **o)), "l1", POLY_L1["tol"], 1),
                           checked)

        def run():
            status, out, results = mb._run_poly(pg, G, F, [m[1] for m in members], POLY_L1)
            assert status == 0
            return (out,) + tuple(_from_results(results))
        return run, refs
    assert case == "dropout"
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix
    F, _ = _columns(G, width, seed, lambda j, p: None, ())
    X = (F / np.maximum(F.sum(axis=0), 1e-300)).astype(np.float32).astype(np.float64)
    stored, rate, seed0, K = G["g"].download_transposed(), 0.3, 77, 6
    want = X.copy()
    for k in range(K):
        want = 0.85 * (gnn.mask_of(stored, rate, seed0 + k) @ want) + 0.15 * X
    cfg = L.LoopCfg(alpha=0.85, use_quotient=0, err_kind=L.ERR_ITERS, tol=1e-6, max_iters=K + 1, end_modulo=1, out_scale=1.0, start_from_p=1)

    def run():
        P, R, results = DeviceMatrix.from_host(X), DeviceMatrix.empty(n, width), (L.LoopResult * width)()
        L.check(L.lib().pgh_ppr_run_batch_dropout(G["g"]._h, P._h, R._h, C.byref(cfg), None, rate, seed0, results))
        assert all(r.spmv_count == K for r in results)
        return (np.asarray(R, dtype=np.float64),) + tuple(_from_results(results))

    def check(out):
        rel = float(np.max(np.abs(out - want)) / np.max(np.abs(want)))
        assert rel <= 2e-6, rel
        return rel
    return run, check


@pytest.fixture(scope="module")
def built(pg, graphs):
    assert not any(name in os.environ for name in SWITCHES), "the switch sets start from an environment without PGH_MM_* run switches"
    made = {}

    def get(gkey, case, width):
        if (gkey, case, width) not in made:
            made[gkey, case, width] = _build(pg, graphs(gkey), gkey, case, width)
        return made[gkey, case, width]
    return get


@pytest.mark.parametrize("gkey,case,width", RUNS, ids=[f"{g}-{c}-b{w}" for g, c, w in RUNS])
@pytest.mark.parametrize("switches", list(SETS))
def test_multi_seed_loops_under_their_switches(built, switches, gkey, case, width):
    run, refs = built(gkey, case, width)
    with be._env(**SETS[switches]):
        out, iters, spmv, flags = run()
        again = run()
    where = (switches, gkey, case, width)
    if callable(refs):
        rel = refs(out)
    else:
        assert np.all(out[:, 1] == 0), where                  # the zero column
        rel = max(ref.held(out[:, j], iters[j], where + (j,)) for j, ref in refs.items())
    print(f"{switches} {gkey} {case} b={width} iterations={iters} spmv={spmv} flags={flags} rel={rel:.3e}")
    assert np.array_equal(out, again[0]) and (iters, spmv, flags) == tuple(again[1:]), where
    fused = SETS[switches].get("PGH_MM_FUSED") != "0"
    if case in L1_PPR:
        assert all(bool(f & 2) == fused for f in flags), where + (flags,)
    if case == "signed":
        assert all(bool(f & 2) == fused and bool(f & 1) == fused for f in flags), where + (flags,)
