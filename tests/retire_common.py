"""What the tests of the retiring multi-seed loops (include/pgh_retire.h) share: the graph upload, the acceptance rule and its helpers
as tests/test_gpu_batch_edges.py has them (_adjacency, _graph, _rel, _stop_margin_ok: copied), the column mix whose columns stop at very
different steps, the oracle's trace of one column, and the stages a list of per-column stopping steps implies.

Acceptance per column (the suite's rule): against the fp64 oracle (oracle/ref_loops.py on the engine's downloaded matrix, eps = fp32 eps)
and against the single-vector device run, relative L-inf <= 1e-6 with equal iteration counts; a stop one check apart only when the
oracle's own residual at the earlier stop lies within 2 % of the tolerance; zero columns exactly zero.

The narrowing rule the engine documents (include/pgh_retire.h), restated in `stages_of`: behind the committed close of step k, with
`live` columns not yet stopped, a slab of width ld narrows to (live + 3) & ~3 when 0 < live <= min(greatest level below ld, ld - 4);
at most 8 stages."""
import collections

import numpy as np
import scipy.sparse as sp

from oracle import ref_loops as orc

EPS32 = float(np.finfo(np.float32).eps)
BOUND = 1e-6
DEFAULT_LEVELS = (32, 16, 8, 4)
WIDE_LEVELS = (48, 20, 12, 4)      # every lanes-per-row transition (16 -> 16, 16 -> 8, 8 -> 4, 4 -> 4) and slabs of 20 and 12 columns
MAX_STAGES = 8
NARROWED = 32                      # bit 5 of pgh_loop_result::flags

RULES = {
    "l1": dict(error_type="l1", tol=1e-6, max_iters=1000),
    "mabs": dict(error_type="mabs", tol=1e-6, max_iters=1000),
    "linf": dict(error_type="linf", tol=1e-6, max_iters=1000),
    "modulo3": dict(error_type="l1", tol=1e-6, max_iters=1000, end_modulo=3),
    "iters": dict(error_type="iters", max_iters=12),
    "default": dict(max_iters=1000),
}


def _adjacency(g):
    """A device graph as a preprocessed graph the filters take as-is (its stored matrix is already normalised)."""
    from pygrank_amd.preprocessing import Adjacency
    from pygrank_amd.signals import _IdentityMap
    adj = Adjacency(g)
    adj._pygrank_preprocessed = {"hip": adj}
    adj._pygrank_node2id = _IdentityMap(g.shape[0])
    adj.is_directed = lambda: True
    return adj


def _graph(pg, A, normalization):
    """Uploads A; returns the wrapped graph, the device graph, the stored M (oracle orientation: x @ M = conv(x)), the rows of M^T
    without entries (nodes nothing propagates into) and the nodes with edges in both directions (where sparse seeds go)."""
    g = pg.DeviceGraph.from_adjacency(A, normalization)
    MT = sp.csr_array(g.download_transposed().astype(np.float64))
    M = sp.csr_array(MT.T)
    has_in, has_out = np.diff(MT.indptr) > 0, np.diff(M.indptr) > 0
    return dict(adj=_adjacency(g), g=g, M=M, n=g.shape[0], dead=np.flatnonzero(~has_in), live=np.flatnonzero(has_in & has_out))


def _rel(got, want):
    scale = np.max(np.abs(want))
    if scale == 0:
        return 0.0 if np.all(got == 0) else np.inf
    return float(np.max(np.abs(got - want)) / scale)


def _stop_margin_ok(run_iters, p, stop, oracle_stop, tol, rule, preserve_norm=True):
    """A stop one check apart is accepted only when the oracle's own residual at the check where the two disagree -- the earlier of
    the two stops -- lies within f32 rounding (2 %) of the tolerance, under the rule in use: the L1 sum, the sum over n for Mabs, the
    max for Linf.  run_iters(k) -> the oracle's ranks after k iterations.  Returns (ok, the oracle's ranks at the engine's stop,
    residual / tol)."""
    k = min(stop, oracle_stop)
    d = np.abs(run_iters(k) - run_iters(k - 1))
    residual = {"l1": d.sum(), "mabs": d.sum() / len(d), "linf": d.max()}[rule]
    if preserve_norm:
        residual /= np.abs(p).sum()
    return abs(residual - tol) <= 0.02 * tol, run_iters(stop), residual / tol


# ------------------------------------------------------------------------------------------------------------- inputs
def mix(G, width, seed, zeros=(), dead=()):
    """[n, width], rounded through f32: per group of four columns a single seed, 20 weighted seeds, a dense uniform column and n / 10
    unit seeds -- columns that stop at very different steps.  zeros: columns left all zero; dead: columns whose only non-zeros sit on
    rows nothing propagates into (they stop at their first check)."""
    rng = np.random.default_rng(seed)
    n, live = G["n"], G["live"]
    F = np.zeros((n, width))
    for j in range(width):
        kind = j % 4
        if j in zeros:
            continue
        if j in dead:
            F[rng.choice(G["dead"], min(len(G["dead"]), 3), replace=False), j] = rng.uniform(0.5, 1.5, min(len(G["dead"]), 3))
        elif kind == 0:
            F[rng.choice(live), j] = 1.0
        elif kind == 1:
            F[rng.choice(live, 20, replace=False), j] = rng.uniform(0.5, 1.5, 20)
        elif kind == 2:
            F[:, j] = rng.uniform(0.0, 1.0, n)
        else:
            F[rng.choice(live, max(n // 10, 1), replace=False), j] = 1.0
    return F.astype(np.float32).astype(np.float64)


def family(pg, name, rule, alpha=0.85, **extra):
    """(ranker factory(**more), oracle(M, p, **override), residual rule, tol, end_modulo) of a filter family under a stopping rule."""
    kw = dict(RULES[rule], **extra)
    err = kw.get("error_type", "mabs")
    engine_kw = dict(kw)
    if "error_type" in engine_kw:
        engine_kw["error_type"] = {"l1": pg.L1, "mabs": pg.Mabs, "linf": pg.MaxDifference, "iters": "iters"}[err]
    oracle_kw = dict(kw, eps=EPS32)
    cls, args, fn = {
        "pagerank": (pg.PageRank, (alpha,), lambda M, p, **o: orc.pagerank(M, p, alpha=alpha, **o)),
        "absorbing": (pg.AbsorbingWalks, (alpha,), lambda M, p, **o: orc.absorbing_walks(M, p, alpha=alpha, **o)),
        "sarw": (pg.SymmetricAbsorbingRandomWalks, (), lambda M, p, **o: orc.symmetric_absorbing_walks(M, p, **o)),
    }[name]
    return (lambda **more: cls(*args, **dict(engine_kw, **more)),
            lambda M, p, **override: fn(M, p, **dict(oracle_kw, **override)), err, kw.get("tol", 1e-6), kw.get("end_modulo", 1))


def oracle_trace(oracle, M, p, rule, tol, modulo, hook=True, **override):
    """One oracle run of a column with its last iterates kept (through the oracle's own conv_fn hook; hook=False, for a family that
    scales the iterate in front of its product: further oracle runs of a fixed length instead): (ranks, iterations, margins) with
    margins = the oracle's residual / tol at the check that stopped it and at the check before (inf where there is none).  Zero columns
    and the "iters" rule: no margins."""
    if not p.any():
        return p, 0, ()
    kept = collections.deque(maxlen=modulo + 2)

    def conv(x, matrix):
        kept.append(x)
        return orc.conv(x, matrix)
    ranks, its = oracle(M, p, conv_fn=conv, **override)
    if rule == "iters":
        return ranks, its, ()
    if not hook:
        kept = [oracle(M, p, **dict(override, error_type="iters", max_iters=k))[0] / np.abs(p).sum()
                for k in range(max(its - modulo - 1, 1), its)]
    seq = list(kept) + [ranks / np.abs(p).sum()]                # the iterates its - len(seq) ... its - 1 (iterate i: after i steps)

    def residual(check):                                        # the check of iteration `check` compares iterates check - 2 and check - 1
        i = len(seq) - 1 - (its - check)
        if i < 1:
            return np.inf
        d = np.abs(seq[i] - seq[i - 1])
        return {"l1": d.sum(), "mabs": d.sum() / len(d), "linf": d.max()}[rule]
    return ranks, its, (residual(its) / tol, residual(its - modulo) / tol)


def near(margins):
    """The column may need the one-check allowance: one of the two residuals lies within 2 % of the tolerance."""
    return any(abs(m - 1.0) <= 0.02 for m in margins)


def vouched(margins):
    """The oracle vouches for the column's stop: the residual that stopped it lies 10 % below the tolerance and the one before 10 % above
    (a column that settles slowly -- its residual falls by a few per cent per step -- has several checks near the tolerance, and f32
    rounding of the iterates moves its stop by more than one of them)."""
    return len(margins) == 0 or (margins[0] <= 0.9 and margins[1] >= 1.1)


def stages_of(steps, stopped, width, levels, last_step):
    """The stages a run of `width` columns takes when column j stops at the close of step steps[j] (stopped[j] false: it never stops) and
    the run executes `last_step` steps: a list of (ld, live, first_step), and the sum over the executed steps of ld."""
    ld = (width + 3) & ~3
    out, streamed = [(ld, width, 1)], 0
    for k in range(1, last_step + 1):
        streamed += ld
        live = sum(1 for s, c in zip(steps, stopped) if not c or s > k)
        below = [level for level in levels if level < ld]
        trigger = min(max(below), ld - 4) if below and len(out) < MAX_STAGES else 0
        if 0 < live <= trigger:
            ld = (live + 3) & ~3
            out.append((ld, live, k + 1))
    return out, streamed


def report_stages(stages):
    """last_batches' "stages" record as the list stages_of returns."""
    return list(zip(stages["ld"], stages["live"], stages["first_step"]))


class References:
    """The two references of the columns `cols` of F, computed once and shared by every run that is held against them: the oracle's
    (ranks, iterations) and the single-vector device run's.  make_kw(j) / rank_kw(j) / oracle_kw(j): what column j's single ranker,
    its rank() call and its oracle run take beyond the family's own (a column's alpha, its warm start, an absorption)."""

    def __init__(self, pg, G, F, spec, cols, make_kw=None, rank_kw=None, oracle_kw=None, label=""):
        self.G, self.F, self.spec, self.cols, self.label = G, F, spec, list(cols), label
        self.oracle_kw = oracle_kw or (lambda j: {})
        make, oracle = spec[0], spec[1]
        self.single, self.oracle = {}, {}
        for j in self.cols:
            p = F[:, j]
            if not p.any():
                continue
            ranker = make(**(make_kw(j) if make_kw else {}))
            got = np.asarray(ranker.rank(G["adj"], p.copy(), **(rank_kw(j) if rank_kw else {})).np, dtype=np.float64)
            self.single[j] = (got, ranker.convergence.iteration)
            self.oracle[j] = oracle(G["M"], p, **self.oracle_kw(j))
            self._held(j, got, ranker.convergence.iteration, "single")     # a failure here lies with the f32 route itself

    def _held(self, j, col, its, who):
        _, oracle, rule, tol, modulo = self.spec
        p, where = self.F[:, j], (self.label, j, who)
        ref, it = self.oracle[j]
        if its != it:
            assert rule != "iters" and abs(its - it) == modulo, where + (its, it)
            ok, ref, ratio = _stop_margin_ok(lambda k: oracle(self.G["M"], p, **dict(self.oracle_kw(j), error_type="iters", max_iters=k))[0],
                                             p, its, it, tol, rule)
            assert ok, where + (its, it, ratio)
        assert _rel(col, ref) <= BOUND, where + (_rel(col, ref),)

    def hold(self, out, iters, who="batch"):
        """Each column of a run against the oracle and the single-vector run, as the module docstring states."""
        for j in self.cols:
            if not self.F[:, j].any():
                assert np.all(out[:, j] == 0), (self.label, j, who)
                continue
            self._held(j, out[:, j], iters[j], who)
            got1, it1 = self.single[j]
            if iters[j] == it1:
                assert _rel(out[:, j], got1) <= BOUND, (self.label, j, who, "against the single run", _rel(out[:, j], got1))
