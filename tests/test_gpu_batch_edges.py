"""The multi-seed loops of propagate() (pgh_ppr_run_batch, pgh_poly_run_batch, pgh_absorb_run_batch, pgh_sarw_run_batch) on the
inputs a GNN-style caller sends them: dense and signed feature columns, every lane shape of the batch kernels, and the stopping rules
the other batch tests never use.

lanes_per_row(ld) gives 4 lanes per row for widths 1-16, 8 for 17-32 and 16 for 33-64; a width that is not a multiple of four ends in
a partial float4, and 81 / 130 columns run a full chunk of 64 followed by a chunk of another shape.  Each batch mixes six kinds of
column: sparse non-negative seeds, sparse seeds with about one entry in four negative, dense columns, an all-negative column, a zero
column and a column whose only non-zeros sit on rows without entries.  A signed value pauses the in-kernel residual of the PageRank
loop (k_mm_step poisons the lane, the host re-runs the close with the separate residual kernel and drops the fusion): the tests read
that from the batch's flags.

Every compared column is held against two references: (i) the fp64 oracle (oracle/ref_loops.py) on the engine's stored matrix at the
engine's fp32 epsilon, (ii) the single-vector device run of the same column.  Both must agree to <= 1e-6 relative L-inf with equal
iteration counts; a stop one check apart is accepted only when the oracle's own residual at the engine's stop lies within 2 % of the
tolerance.  Zero columns stay exactly zero.

Measured on the MI355X: the module takes about 13 s of wall time (108 tests)."""
import contextlib
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cases
from oracle import ref_loops as orc
from oracle import rmat_np

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
BOUND = 1e-6
WIDTHS = (1, 3, 4, 5, 15, 16, 17, 24, 31, 32, 33, 48, 63, 64, 81, 130)
KINDS = ("seeds", "signed", "dense", "negative", "zero", "dead")
W20 = [0.85 ** i for i in range(20)]

# stopping rules: the ranker's keyword arguments with the oracle's name of the error type
RULES = {
    "l1": dict(error_type="l1", tol=1e-6, max_iters=1000),
    "mabs": dict(error_type="mabs", tol=1e-6, max_iters=1000),
    "linf": dict(error_type="linf", tol=1e-6, max_iters=1000),
    "modulo3": dict(error_type="l1", tol=1e-6, max_iters=1000, end_modulo=3),
    "iters1": dict(error_type="iters", max_iters=1),
    "iters2": dict(error_type="iters", max_iters=2),
    "iters3": dict(error_type="iters", max_iters=3),
    "iters31": dict(error_type="iters", max_iters=31),
    "noquot_iters": dict(error_type="iters", max_iters=20, use_quotient=False),
    "noquot_l1": dict(error_type="l1", tol=1e-6, max_iters=1000, use_quotient=False),
    "nonorm": dict(error_type="l1", tol=1e-6, max_iters=1000, preserve_norm=False),
    "absorption": dict(error_type="l1", tol=1e-6, max_iters=1000),
    "default": dict(max_iters=1000),
}


@pytest.fixture(scope="module")
def pg():
    import pygrank_amd
    from pygrank_amd import _lib
    pygrank_amd.load_backend("hip")
    assert _lib.runtime_name().startswith("hip:")
    for name in ("pgh_poly_run_batch", "pgh_absorb_run_batch", "pgh_sarw_run_batch"):
        assert _lib.entry(name) is not None, name
    return pygrank_amd


@contextlib.contextmanager
def _env(**values):
    """Sets PGH_* switches for the block and restores them afterwards (test_gpu_dense_graphs.py)."""
    saved = {k: os.environ.get(k) for k in values}
    try:
        os.environ.update(values)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


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


def _rmat17(weighted):
    """RMAT scale 17 with duplicate edges summed into integer multiplicities (or real weights in [0.5, 2]); every 97th node loses its
    out-edges (dangling rows), every 89th node loses all its edges (isolated), every 83rd keeps only its out-edges (source-only)."""
    A = sp.csr_array(rmat_np.rmat_csr(17, 8, seed=11), dtype=np.float64)
    n = A.shape[0]
    ids = np.arange(n)
    keep_row = (ids % 97 != 5) & (ids % 89 != 7)
    keep_col = (ids % 89 != 7) & (ids % 83 != 3)
    A = sp.csr_array(sp.diags(keep_row.astype(float)) @ A @ sp.diags(keep_col.astype(float)))
    A.eliminate_zeros()
    if weighted:
        A.data = np.random.default_rng(17).uniform(0.5, 2.0, A.nnz)
    A.sort_indices()
    return A


@pytest.fixture(scope="module")
def graphs(pg):
    built = {}

    def get(key):
        if key not in built:
            if key in cases.GRAPHS:
                A, directed, _ = cases.GRAPHS[key]()
                built[key] = _graph(pg, A, "col" if directed else "symmetric")
            elif key == "rmat10_sym":                    # rmat10_dir made undirected: a small symmetric graph
                A, _, _ = cases.GRAPHS["rmat10_dir"]()
                A = sp.csr_array(A + A.T)
                A.sort_indices()
                built[key] = _graph(pg, A, "symmetric")
            elif key in ("rmat17", "rmat17_valued"):
                built[key] = _graph(pg, _rmat17(key == "rmat17_valued"), "col")
                fmt = built[key]["g"].format()
                assert ("f32-valued" if key == "rmat17_valued" else "value-free") in fmt, fmt
            else:
                raise KeyError(key)
        return built[key]
    return get


def _column(kind, G, rng, quotient=True):
    """One feature column of the given kind, rounded through f32 (what the engine receives).  Sparse seeds sit on nodes with edges in
    both directions.  Columns that run with the quotient keep |sum p| >= 0.2 sum |p| by construction: negative entries are at most
    0.3 against positive ones of at least 0.5, dense columns are drawn around 0.3; without the quotient dense columns are symmetric
    N(0, 1)."""
    n, dead, live = G["n"], G["dead"], G["live"]
    p = np.zeros(n)
    if kind in ("seeds", "negative"):
        idx = rng.choice(live, int(rng.integers(8, 17)), replace=False)
        p[idx] = rng.uniform(0.5, 1.5, len(idx))
        if kind == "negative":
            p = -p
    elif kind == "signed":
        idx = rng.choice(live, 16, replace=False)
        p[idx] = rng.uniform(0.5, 1.5, len(idx))
        p[idx[:4]] = -rng.uniform(0.1, 0.3, 4)
    elif kind == "dense":
        p = rng.normal(0.3 if quotient else 0.0, 1.0, n)
    elif kind == "dead":
        if len(dead):
            idx = rng.choice(dead, min(len(dead), 5), replace=False)
            p[idx] = rng.uniform(0.5, 1.5, len(idx))
    return p.astype(np.float32).astype(np.float64)


def _features(width, G, seed, quotient=True, offset=0):
    """[n, width] with the kinds of KINDS in turn (column j: KINDS[(j + offset) % 6]); a graph with no dead rows gives a zero column
    for that kind."""
    rng = np.random.default_rng(seed)
    kinds = [KINDS[(j + offset) % len(KINDS)] for j in range(width)]
    F = np.stack([_column(k, G, rng, quotient) for k in kinds], axis=1)
    if quotient:
        s, a = F.sum(axis=0), np.abs(F).sum(axis=0)
        assert np.all((a == 0) | (np.abs(s) >= 0.2 * a))
    return F, kinds


def _absorption(G, zeros_on_dangling):
    """A custom absorption with zeros: on rows that have out-edges only (degree > 0, the walk stays defined), or also on a dangling row
    (absorption + degree == 0: the batch loop must decline it)."""
    n = G["n"]
    deg = np.asarray(abs(G["M"]).sum(axis=1)).ravel()
    a = 0.5 + np.arange(n, dtype=np.float64) / n
    live = np.flatnonzero(deg > 0)
    a[live[::7]] = 0.0
    if zeros_on_dangling:
        a[np.flatnonzero(deg == 0)[:3]] = 0.0
    return a


def _make(pg, family, rule, **extra):
    """(ranker factory, oracle(p, M, **override), rule name for the residual, tol, end_modulo, preserve_norm)."""
    kw = dict(RULES[rule], **extra)
    err = kw.get("error_type", "mabs")
    names = {"l1": pg.L1, "mabs": pg.Mabs, "linf": pg.MaxDifference, "iters": "iters"}
    engine_kw = dict(kw)
    if "error_type" in engine_kw:
        engine_kw["error_type"] = names[engine_kw["error_type"]]
    oracle_kw = dict(kw, eps=EPS32)
    cls, args, fn = {
        "pagerank": (pg.PageRank, (0.85,), lambda M, p, **o: orc.pagerank(M, p, alpha=0.85, **o)),
        "heat": (pg.HeatKernel, (5,), lambda M, p, **o: orc.heat_kernel(M, p, t=5, **o)),
        "generic": (pg.GenericGraphFilter, (), lambda M, p, **o: orc.generic_filter(M, p, W20, **o)),
        "closed": (pg.PageRankClosed, (0.85,), lambda M, p, **o: orc.pagerank_closed(M, p, alpha=0.85, **o)),
        "absorbing": (pg.AbsorbingWalks, (0.85,), lambda M, p, **o: orc.absorbing_walks(M, p, alpha=0.85, **o)),
        "sarw": (pg.SymmetricAbsorbingRandomWalks, (), lambda M, p, **o: orc.symmetric_absorbing_walks(M, p, **o)),
    }[family]
    if family == "generic":
        engine_kw["weights"] = W20

    def make():
        return cls(*args, **engine_kw)

    def oracle(M, p, absorption=None, **override):
        o = dict(oracle_kw, **override)
        if absorption is not None:
            o["absorption"] = absorption
        return fn(M, p, **o)
    return make, oracle, err, kw.get("tol", 1e-6), kw.get("end_modulo", 1), kw.get("preserve_norm", True)


def _rel(got, want):
    scale = np.max(np.abs(want))
    if scale == 0:
        return 0.0 if np.all(got == 0) else np.inf
    return float(np.max(np.abs(got - want)) / scale)


def _stop_margin_ok(run_iters, p, stop, oracle_stop, tol, rule, preserve_norm=True):
    """A stop one check apart is accepted only when the oracle's own residual at the check where the two disagree -- the earlier of
    the two stops -- lies within f32 rounding (2 %) of the tolerance (test_gpu_batch_filters.py), under the rule in use: the L1 sum,
    the sum over n for Mabs, the max for Linf.  run_iters(k) -> the oracle's ranks after k iterations.  Returns (ok, the oracle's
    ranks at the engine's stop, residual / tol)."""
    k = min(stop, oracle_stop)
    d = np.abs(run_iters(k) - run_iters(k - 1))
    residual = {"l1": d.sum(), "mabs": d.sum() / len(d), "linf": d.max()}[rule]
    if preserve_norm:
        residual /= np.abs(p).sum()
    return abs(residual - tol) <= 0.02 * tol, run_iters(stop), residual / tol


def _iterations(ranker):
    return [c["iterations"] for batch in ranker.last_batches for c in batch]


def _flags(ranker):
    return [c["flags"] for batch in ranker.last_batches for c in batch]


def _sample(width, n_all):
    """Every column on small graphs; on the larger ones the columns on each side of a lane-group boundary and the last one."""
    if n_all:
        return list(range(width))
    return sorted({j for j in (0, 1, 3, 4, 15, 16, 31, 32, 63, 64, width - 1) if j < width})


def _check_columns(pg, G, F, out, iters, spec, cols, call_kw=None, label=""):
    """Each column in `cols` against (i) the oracle and (ii) the single-vector run, as the module docstring states."""
    make, oracle, rule, tol, modulo, preserve_norm = spec
    call_kw = call_kw or {}
    absorption = call_kw.get("absorption")
    M = G["M"]
    for j in cols:
        p = F[:, j]
        where = (label, j)
        if not p.any():
            assert np.all(out[:, j] == 0), where
            continue
        single = make()
        got1 = np.asarray(single.rank(G["adj"], p.copy(), **call_kw).np, dtype=np.float64)
        it1 = single.convergence.iteration
        want, it = oracle(M, p, absorption=absorption)

        def held(col, its, who):
            ref = want
            if its != it:
                assert rule != "iters" and abs(its - it) == modulo, where + (who, its, it)
                ok, ref, ratio = _stop_margin_ok(lambda k: oracle(M, p, absorption=absorption, error_type="iters", max_iters=k)[0], p, its,
                                                 it, tol, rule, preserve_norm)
                assert ok, where + (who, its, it, ratio)
            assert _rel(col, ref) <= BOUND, where + (who, _rel(col, ref))
        held(got1, it1, "single")                     # (ii) against (i): a failure here lies with the f32 route itself
        held(out[:, j], iters[j], "batch")
        if iters[j] == it1:
            assert _rel(out[:, j], got1) <= BOUND, where + ("batch vs single", _rel(out[:, j], got1))


def _run_batch(pg, G, F, spec, call_kw=None):
    make = spec[0]
    ranker = make()
    out = np.asarray(ranker.propagate(G["adj"], pg.to_primitive(F), **(call_kw or {})), dtype=np.float64)
    assert out.shape == F.shape
    assert hasattr(ranker, "last_batches"), "the batch route was not taken"
    assert len(ranker.last_batches) == (F.shape[1] + 63) // 64
    return ranker, out, _iterations(ranker)


# ------------------------------------------------------------------------------------------------------------- the sweep
SMALL = ("rmat10_dir", "weighted300", "rmat12_sym", "er10k")
LARGE = ("rmat17", "rmat17_valued")


def _sweep(family, rules, graphs_cycle):
    """A fixed list: every width once per family, rules and graphs taken in turn."""
    return [(family, rules[i % len(rules)], graphs_cycle[i % len(graphs_cycle)], w) for i, w in enumerate(WIDTHS)]


# (the quotient runs leave out rmat12_sym: on its many small components a dense start takes hundreds of steps to settle, in any precision)
QUOTIENT_GRAPHS = ("rmat10_dir", "weighted300", "er10k") + LARGE
SWEEP = (_sweep("pagerank", ("l1", "mabs", "linf", "modulo3", "noquot_iters"), QUOTIENT_GRAPHS)
         + _sweep("heat", ("iters1", "mabs", "iters2", "l1", "iters3", "linf", "iters31", "modulo3"), SMALL + LARGE[::-1])
         + [(f, r, g, w) for f, r, g, w in _sweep("generic", ("l1", "iters2", "linf", "iters31", "mabs", "iters1", "modulo3", "iters3"),
                                                  SMALL[::-1] + LARGE) if w in (3, 5, 16, 17, 32, 33, 64, 81)]
         + _sweep("closed", ("l1",), SMALL + LARGE)
         + _sweep("absorbing", ("mabs", "l1", "linf", "noquot_l1", "nonorm", "absorption"),
                  ("er10k", "rmat10_dir", "er10k", "weighted300", "rmat17_valued", "rmat17"))
         + _sweep("sarw", ("default",), ("er10k", "rmat10_sym")))
# (AbsorbingWalks keeps its L1 rules off er10k, and SymmetricAbsorbingRandomWalks runs its default rule only: the f32 rounding of the
# iterates moves an L1 sum over them by 3 to 7 % of a 1e-6 tolerance, and the single-vector loop then stops a step from the oracle
# outside the 2 % margin just as the batch does -- on er10k, rmat12_sym and rmat10_sym alike for the symmetric walk)


@pytest.mark.parametrize("family,rule,gkey,width", SWEEP, ids=[f"{f}-{r}-{g}-b{w}" for f, r, g, w in SWEEP])
def test_batch_columns_against_oracle_and_single_runs(pg, graphs, family, rule, gkey, width):
    G = graphs(gkey)
    spec = _make(pg, family, rule)
    quotient = family in ("pagerank", "absorbing", "sarw") and RULES[rule].get("use_quotient", True)
    seed = WIDTHS.index(width) + 100 * ("pagerank", "heat", "generic", "closed", "absorbing", "sarw").index(family)
    F, kinds = _features(width, G, seed, quotient=quotient, offset=seed)
    call_kw = {"absorption": _absorption(G, False)} if rule == "absorption" else None
    ranker, out, iters = _run_batch(pg, G, F, spec, call_kw)
    _check_columns(pg, G, F, out, iters, spec, _sample(width, gkey not in LARGE), call_kw, label=f"{family}/{rule}/{gkey}/b{width}")
    if family == "pagerank" and rule in ("l1", "mabs"):
        # the fused residual starts every batch; a negative value on a row nothing propagates into stays negative in every iterate, so
        # the first checked step pauses and hands the residual to the separate kernel
        # (per chunk of 64 columns: each is a run of its own)
        for c, batch in enumerate(ranker.last_batches):
            flags, chunk = [col["flags"] for col in batch], F[:, 64 * c:64 * (c + 1)]
            assert all(f & 2 for f in flags), (c, flags)
            if (chunk[G["dead"]] < 0).any():
                assert all(f & 1 for f in flags), (c, flags)


def test_appnp_propagation_of_dense_signed_features(pg):
    """The APPNP setting: PageRank(0.9, renormalize=True, use_quotient=False, error_type="iters", max_iters=10) on dense N(0, 1) columns,
    through the ranker's own preprocessor (the renormalised matrix), on a directed and an undirected graph."""
    for gkey, width in (("rmat10_dir", 24), ("er10k", 64)):
        A, directed, _ = cases.GRAPHS[gkey]()
        graph = pg.AdjacencyWrapper(A, directed=directed)
        kw = dict(renormalize=True, use_quotient=False, error_type="iters", max_iters=10)
        ranker = pg.PageRank(0.9, **kw)
        g = ranker.preprocessor(graph).array
        M = sp.csr_array(g.download_transposed().astype(np.float64).T)
        n = A.shape[0]
        F = np.random.default_rng(width).normal(0.0, 1.0, (n, width)).astype(np.float32).astype(np.float64)
        out = np.asarray(ranker.propagate(graph, pg.to_primitive(F)), dtype=np.float64)
        assert hasattr(ranker, "last_batches")
        assert all(it == 10 for it in _iterations(ranker))
        for j in range(width):
            single = pg.PageRank(0.9, **kw)
            single.preprocessor = ranker.preprocessor
            got1 = np.asarray(single.rank(graph, F[:, j].copy()).np, dtype=np.float64)
            want, it = orc.pagerank(M, F[:, j], alpha=0.9, use_quotient=False, error_type="iters", max_iters=10, eps=EPS32)
            assert it == single.convergence.iteration == 10
            assert _rel(got1, want) <= BOUND, (gkey, j, _rel(got1, want))
            assert _rel(out[:, j], want) <= BOUND, (gkey, j, _rel(out[:, j], want))
            assert _rel(out[:, j], got1) <= BOUND, (gkey, j)


def test_absorption_zero_with_zero_degree_is_declined(pg, graphs):
    """absorption + degree == 0 on a dangling row: k_mm_walk_rowops sets `bad`, the batch loop declines and propagate returns what the
    column loop returns."""
    from pygrank_amd.signals import NodeRanking
    G = graphs("rmat10_dir")
    F, _ = _features(17, G, 7)
    absorption = _absorption(G, True)
    make = _make(pg, "absorbing", "absorption")[0]
    X = pg.to_primitive(F)
    ranker = make()
    outcome = []
    for run in (lambda r: r.propagate(G["adj"], X, absorption=absorption),
                lambda r: NodeRanking.propagate(r, G["adj"], X, absorption=absorption)):
        r = make()
        try:
            outcome.append(np.asarray(run(r), dtype=np.float64))
        except Exception as exc:                          # then both must raise alike
            outcome.append((type(exc), str(exc)))
        if len(outcome) == 1:
            ranker = r
    assert not hasattr(ranker, "last_batches")
    if isinstance(outcome[0], tuple) or isinstance(outcome[1], tuple):
        assert outcome[0] == outcome[1]
    else:
        assert np.array_equal(outcome[0], outcome[1], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------- the pause protocol
@pytest.mark.parametrize("width", (1, 3, 4, 5, 15, 16, 17))
def test_non_negative_batches_run_fused(pg, graphs, width):
    """A batch of non-negative seeds does not pause: the fused residual decides every step (flags bit 1, not bit 0), at the 4-lane
    shape with and without idle lanes and at the first 8-lane width.  k_mm_permute_in2 used to return early from the lanes whose
    float4 lies past the row, before the workgroup's fold of the first step's sums: the predicted quotient of the columns those
    lanes stand for was never written, and every such batch paused at its first check."""
    G = graphs("rmat10_dir")
    rng = np.random.default_rng(width)
    F = np.stack([_column("seeds", G, rng) for _ in range(width)], axis=1)
    for rule in ("l1", "mabs"):
        spec = _make(pg, "pagerank", rule)
        ranker, out, iters = _run_batch(pg, G, F, spec)
        assert all(f == 2 for f in _flags(ranker)), (rule, _flags(ranker))
        _check_columns(pg, G, F, out, iters, spec, _sample(width, False), label=f"fused/{rule}/b{width}")


@pytest.mark.parametrize("rule", ["l1", "mabs"])
@pytest.mark.parametrize("gkey", ["rmat10_dir", "rmat17"])
def test_signed_column_pauses_the_fused_residual(pg, graphs, gkey, rule):
    """A batch of non-negative seeds with one signed column: every column reports the pause (flags bit 0), every column still meets
    both references, and the non-negative columns stop where they stop in the all-non-negative batch, which runs fused (bit 1)."""
    G = graphs(gkey)
    spec = _make(pg, "pagerank", rule)
    rng = np.random.default_rng(3)
    width = 20
    F = np.stack([_column("seeds", G, rng) for _ in range(width)], axis=1)
    r0, out0, it0 = _run_batch(pg, G, F, spec)
    assert all(f & 2 for f in _flags(r0)), _flags(r0)
    S = F.copy()
    S[:, 9] = _column("signed", G, rng)
    assert np.any(spec[1](G["M"], S[:, 9], error_type="iters", max_iters=2)[0] < 0)      # the first iterate holds a negative value
    r1, out1, it1 = _run_batch(pg, G, S, spec)
    assert all(f & 1 for f in _flags(r1)), _flags(r1)
    _check_columns(pg, G, S, out1, it1, spec, range(width) if gkey != "rmat17" else (0, 8, 9, 10, 19), label=f"pause/{gkey}/{rule}")
    for j in range(width):
        if j != 9:
            assert it1[j] == it0[j], (j, it1[j], it0[j])
            assert _rel(out1[:, j], out0[:, j]) <= BOUND, j


def _late_pause_graph(pg):
    """rmat10_dir with four extra nodes: h -> a (h source-only, a dangling) and a two-cycle z <-> w.  The column p_h = 1, p_a = -2,
    p_z = 4 keeps the first iterate non-negative (a receives alpha * p_h) and turns a negative at the second (h keeps only its
    (1 - alpha) share, the cycle's mass raises the quotient)."""
    A, _, _ = cases.GRAPHS["rmat10_dir"]()
    n0 = A.shape[0]
    h, a, z, w = n0, n0 + 1, n0 + 2, n0 + 3
    gadget = sp.csr_array((np.ones(3), ([h, z, w], [a, w, z])), shape=(n0 + 4, n0 + 4))
    B = sp.csr_array(sp.block_diag([A, sp.csr_array((4, 4))]).tocsr() + gadget)
    B.sort_indices()
    G = _graph(pg, B, "col")
    p = np.zeros(n0 + 4)
    p[[h, a, z]] = (1.0, -2.0, 4.0)
    return G, p


@pytest.mark.parametrize("rule", ["l1", "mabs"])
def test_pause_after_the_first_step(pg, rule):
    """The pause arrives at step 2: the signed column's first iterate is non-negative (checked on the oracle), its second is not.  The
    steps enqueued behind the pause must be re-run without the fusion."""
    G, p = _late_pause_graph(pg)
    spec = _make(pg, "pagerank", rule)
    make, oracle = spec[0], spec[1]
    x1 = oracle(G["M"], p, error_type="iters", max_iters=2)[0]
    x2 = oracle(G["M"], p, error_type="iters", max_iters=3)[0]
    assert np.all(x1 >= 0) and np.any(x2 < 0)
    rng = np.random.default_rng(4)
    width = 20
    rmat_part = dict(G, live=G["live"][G["live"] < G["n"] - 4])        # the other columns stay off the four extra nodes
    F = np.stack([_column("seeds", rmat_part, rng) for _ in range(width)], axis=1)
    r0, out0, it0 = _run_batch(pg, G, F, spec)
    assert all(f & 1 == 0 for f in _flags(r0)), _flags(r0)
    F[:, 17] = p
    ranker, out, iters = _run_batch(pg, G, F, spec)
    assert all(f & 1 for f in _flags(ranker)), _flags(ranker)
    _check_columns(pg, G, F, out, iters, spec, range(width), label=f"late pause/{rule}")
    for j in range(width):
        if j != 17:
            assert iters[j] == it0[j], (j, iters[j], it0[j])
            assert _rel(out[:, j], out0[:, j]) <= BOUND, j


# ------------------------------------------------------------------------------------------------------------- column independence
@pytest.mark.parametrize("family,rule,kind", [("pagerank", "l1", "signed"), ("pagerank", "mabs", "seeds"), ("heat", "l1", "dense"),
                                              ("absorbing", "linf", "signed")])
def test_a_column_does_not_depend_on_its_neighbours(pg, graphs, family, rule, kind):
    """The same column at positions 0, 17 and the last of width-40 batches of non-negative neighbours: bit-identical values and equal
    iteration counts.  Across lane shapes (widths 5, 20, 40) and beside a signed neighbour: equal iterations (or one check apart under
    the margin rule) and <= 1e-6.  Two identical propagate calls: bit-identical."""
    G = graphs("rmat10_dir")
    spec = _make(pg, family, rule)
    rng = np.random.default_rng(11)
    col = _column(kind, G, rng)
    others = np.stack([_column("seeds", G, rng) for _ in range(40)], axis=1)
    runs = []
    for pos in (0, 17, 39):
        F = others.copy()
        F[:, pos] = col
        ranker, out, iters = _run_batch(pg, G, F, spec)
        runs.append((out[:, pos], iters[pos]))
        if pos == 17:
            ranker2, again, iters2 = _run_batch(pg, G, F, spec)
            assert np.array_equal(out, again) and iters == iters2
    for got, its in runs[1:]:
        assert its == runs[0][1] and np.array_equal(got, runs[0][0])
    ref, ref_it = runs[0]
    signed_neighbour = _column("signed", G, np.random.default_rng(12))
    for width, pos in ((5, 3), (20, 17), (2, 0)):
        F = others[:, :width].copy()
        F[:, pos] = col
        if width == 2:
            F[:, 1] = signed_neighbour
        _, out, iters = _run_batch(pg, G, F, spec)
        if iters[pos] != ref_it:
            _check_columns(pg, G, F, out, iters, spec, [pos], label=f"independence/{width}")
        else:
            assert _rel(out[:, pos], ref) <= BOUND, (width, _rel(out[:, pos], ref))


# ------------------------------------------------------------------------------------------------------------- relabelling
def test_relabelled_and_original_ids_agree(pg):
    """The value-free RMAT graph uploaded with PGH_RELABEL=0 and with PGH_RELABEL=1 (a fresh graph after each change): every column
    within 1e-6 with equal iteration counts, for PageRank, HeatKernel and AbsorbingWalks at 33 columns."""
    A = _rmat17(False)
    uploads = {}
    for value in ("0", "1"):
        with _env(PGH_RELABEL=value):
            uploads[value] = _graph(pg, A, "col")
    assert "original ids" in uploads["0"]["g"].format(), uploads["0"]["g"].format()
    assert "relabelled" in uploads["1"]["g"].format(), uploads["1"]["g"].format()
    F, _ = _features(33, uploads["0"], 21)
    for family, rule in (("pagerank", "l1"), ("heat", "mabs"), ("absorbing", "l1")):
        spec = _make(pg, family, rule)
        results = [_run_batch(pg, uploads[v], F, spec) for v in ("0", "1")]
        assert results[0][2] == results[1][2], family
        for j in range(33):
            assert _rel(results[1][1][:, j], results[0][1][:, j]) <= BOUND, (family, j)
        _check_columns(pg, uploads["1"], F, results[1][1], results[1][2], spec, (0, 16, 32), label=f"relabel/{family}")
