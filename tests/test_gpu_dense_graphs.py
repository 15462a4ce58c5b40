"""The blocked SpMV image on DENSE graphs: rows with hundreds of cold entries each (a cold entry's source lies outside the
PGH_BSF_HOT = 29 696-slot LDS hot cache of its column block; csrc/pgh_pb.hip moves them into the propagation-blocking image).

Every other parity test runs on sparse graphs (edge factor <= 30).  The planner of the cold image hands the per-row cold counts to
the host as bytes and lists the rows with 255 or more beside them (pb_plan); kNN / co-occurrence graphs put nearly every row in
that list.  Three parts:

  A  a uniform graph of 131 072 nodes and ~400 in-edges per node (nearly every row listed), value-free and valued: upload under the
     default heuristics, products against scipy in fp64, with and without the image, signed inputs over 30 decades, determinism;
  B  filters on that graph against the oracle (equal iteration counts, 1e-6): f32 loops, the f64 routes, 64-column propagate;
  C  graphs whose every row has a cold count known by construction -- the boundary counts of the byte transport, of the hub rows
     and of the split hub rows, the planner's list filled to exactly its first size and one beyond -- checked through the entry
     counts of format() and row by row; the f64 image's counts with its 20 224-slot hot cache.

References are fp64: scipy on the engine's own stored matrix (download_transposed) and oracle/ref_loops.py."""
import contextlib
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ref_loops as orc

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
HOT, HOT64 = 29696, 20224                      # PGH_BSF_HOT (f32 image), kHot64 (f64 image): hot sources per column block
PB_ENV = ("PGH_PB", "PGH_PB_FORCE", "PGH_PB_HEAVY", "PGH_PB_HUBMAX", "PGH_BLOCKS", "PGH_BLOCKS64", "PGH_PB64")


@pytest.fixture(scope="module")
def pg():
    import pygrank_amd
    from pygrank_amd import _lib
    pygrank_amd.load_backend("hip")
    assert _lib.runtime_name().startswith("hip:")
    return pygrank_amd


@contextlib.contextmanager
def _env(**values):
    """Sets the PGH_* layout switches for the block (the others of PB_ENV unset) and restores all of them afterwards."""
    saved = {k: os.environ.get(k) for k in PB_ENV}
    try:
        for k in PB_ENV:
            os.environ.pop(k, None)
        os.environ.update(values)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _np(v):
    return np.asarray(v, dtype=np.float64)


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def _adjacency(g):
    """A device graph as a preprocessed graph the filters take as-is (its stored matrix is already normalised)."""
    from pygrank_amd.preprocessing import Adjacency
    from pygrank_amd.signals import _IdentityMap
    adj = Adjacency(g)
    adj._pygrank_preprocessed = {"hip": adj}
    adj._pygrank_node2id = _IdentityMap(g.shape[0])
    adj.is_directed = lambda: True
    return adj


def _stored(g):
    """(MT, M): the engine's stored M^T in fp64 (CSR: MT @ x = conv(x)), and M as the oracle takes it (x @ M = MT @ x)."""
    MT = sp.csr_array(g.download_transposed().astype(np.float64))
    return MT, MT.T


def _cold_entries(fmt, f64=False):
    pat = r"f64 propagation-blocking image of (\d+) entries" if f64 else r"cold tail: propagation-blocking image in \d+ slices, first: (\d+) entries"
    m = re.search(pat, fmt)
    return None if m is None else int(m.group(1))


def _check_products(pg, g, MT, rng, label, bound=2.5):
    """conv(x) against scipy fp64 on the stored matrix, row by row: positive inputs within `bound` f32 roundings of the sum of
    |products|, signed inputs over 30 decades within the image's bound (kernel_checks.check_propagation_blocking_image); repeated
    launches bit-identical.  Returns the positive input's product."""
    n = MT.shape[1]
    x = rng.random(n).astype(np.float32).astype(np.float64)
    y = _np(pg.conv(pg.to_array(x), g))
    ref = MT @ x
    scale = abs(MT) @ np.abs(x)
    err = np.abs(y - ref)
    assert np.all(err <= bound * EPS32 * scale + 1e-30), (label, float(np.max(err / (EPS32 * scale + 1e-30))))
    assert np.array_equal(_np(pg.conv(pg.to_array(x), g)), y), label
    xw = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-30, 0, n)).astype(np.float32).astype(np.float64)
    yw = _np(pg.conv(pg.to_array(xw), g))
    exact = MT @ xw
    wb = 8 * EPS32 * (abs(MT) @ np.abs(xw)) + 1e-11 * np.max(np.abs(xw)) * np.max(np.abs(MT.data))
    assert np.all(np.abs(yw - exact) <= wb), (label, float(np.max(np.abs(yw - exact) / wb)))
    assert np.array_equal(_np(pg.conv(pg.to_array(xw), g)), yw), label
    return x, y


# ------------------------------------------------------------------------------------------------------------------- A
DENSE_SCALE, DENSE_EF = 17, 400                # uniform: ~309 cold entries per row against one hot cache; nearly every row >= 255


@pytest.fixture(scope="module")
def dense(pg):
    from pygrank_amd.synthetic import rmat_graph
    with _env():
        adj = rmat_graph(DENSE_SCALE, DENSE_EF, a=0.25, b=0.25, c=0.25, seed=3, normalization="col")
    g = adj.array
    MT, M = _stored(g)
    n = g.shape[0]
    cand = np.flatnonzero(np.asarray(pg.degrees(g)) > 0)

    def seeds(k, count=100):
        p = np.zeros(n)
        p[np.sort(np.random.default_rng(100 + k).choice(cand, count, replace=False))] = 1.0
        return p
    return dict(adj=adj, g=g, MT=MT, M=M, n=n, seeds=seeds)


def test_dense_graph_is_beyond_the_planner_list(dense):
    """The premise: one column block, and more rows with >= 255 cold entries than the planner's first list holds
    (max(65 536, n / 16))."""
    g, MT = dense["g"], dense["MT"]
    fmt = g.format()
    assert "bsf: 1 column blocks" in fmt, fmt
    # relabelled by reference count: the HOT most referenced sources are hot, every other entry is cold (up to ties and integer
    # weights: the margin is tens of thousands of rows)
    refs = np.bincount(MT.indices, minlength=dense["n"])
    hot = np.zeros(dense["n"], dtype=bool)
    hot[np.argsort(-refs, kind="stable")[:HOT]] = True
    cum = np.concatenate([[0], np.cumsum(~hot[MT.indices])])
    cold_per_row = cum[MT.indptr[1:]] - cum[MT.indptr[:-1]]
    assert np.count_nonzero(cold_per_row >= 255) > max(65536, dense["n"] // 16)


@pytest.mark.parametrize("weights", ["value-free", "valued"])
def test_dense_upload_products(pg, dense, weights):
    """Upload under the default heuristics (the image without PGH_PB_FORCE), products against scipy fp64, the same products
    without the image (PGH_PB=0), signed inputs over 30 decades, determinism."""
    from pygrank_amd.device import DeviceGraph
    from pygrank_amd.synthetic import rmat_device_graph
    rng = np.random.default_rng(7)
    if weights == "value-free":
        g, MT = dense["g"], dense["MT"]
        with _env(PGH_PB="0"):
            g0 = rmat_device_graph(DENSE_SCALE, DENSE_EF, a=0.25, b=0.25, c=0.25, seed=3, normalization="col")
    else:
        # the same edges with real weights in [0.5, 2): the valued stream (4 more bytes per entry)
        A = dense["M"].tocsr()
        W = sp.csr_array((rng.uniform(0.5, 2.0, A.nnz), A.indices, A.indptr), shape=A.shape)
        del A
        with _env():
            g = DeviceGraph.from_adjacency(W, "col")
        with _env(PGH_PB="0"):
            g0 = DeviceGraph.from_adjacency(W, "col")
        del W
        MT, _ = _stored(g)
    fmt, fmt0 = g.format(), g0.format()
    assert "propagation-blocking image" in fmt and "propagation-blocking" not in fmt0, (fmt, fmt0)
    assert ("f32-valued" in fmt) == (weights == "valued"), fmt
    assert _cold_entries(fmt) > 0.7 * MT.nnz, fmt
    x, y = _check_products(pg, g, MT, rng, weights)
    y0 = _np(pg.conv(pg.to_array(x), g0))
    scale = abs(MT) @ x
    assert np.all(np.abs(y - y0) <= 8 * EPS32 * scale + 1e-30), (weights, float(np.max(np.abs(y - y0) / (EPS32 * scale + 1e-30))))


# ------------------------------------------------------------------------------------------------------------------- B
def test_dense_f32_filters_vs_oracle(pg, dense):
    adj, M = dense["adj"], dense["M"]
    p = dense["seeds"](0)
    runs = ((pg.PageRank(0.85, error_type=pg.L1, tol=1e-6, max_iters=1000),
             lambda: orc.pagerank(M, p, alpha=0.85, error_type="l1", tol=1e-6, max_iters=1000)),
            (pg.AbsorbingWalks(0.85, error_type=pg.L1, tol=1e-6, max_iters=1000),
             lambda: orc.absorbing_walks(M, p, alpha=0.85, error_type="l1", tol=1e-6, max_iters=1000)),
            (pg.HeatKernel(5), lambda: orc.heat_kernel(M, p, t=5, eps=EPS32)))
    for ranker, oracle in runs:
        got = _np(ranker.rank(adj, p.copy()).np)
        want, want_iters = oracle()
        name = type(ranker).__name__
        assert ranker.convergence.iteration == want_iters, (name, ranker.convergence.iteration, want_iters)
        assert _rel(got, want) <= 1e-6, (name, _rel(got, want))


def test_dense_f64_routes_vs_oracle(pg, dense):
    """HeatKernel "chebyshev" and PageRank at tol = 1e-9 run with f64 iterates on the f64 image.  Here its eight column blocks of
    16 384 sources each fit the 20 224-slot hot cache: no cold image (part C covers the f64 cold image of a dense graph)."""
    adj, M = dense["adj"], dense["M"]
    p = dense["seeds"](1)
    cheb = pg.HeatKernel(5, coefficient_type="chebyshev", error_type=pg.L1, tol=1e-9, max_iters=40)
    got = _np(cheb.rank(adj, p.copy()).np)
    want, want_iters = orc.heat_kernel(M, p, t=5, coefficient_type="chebyshev", tol=1e-9, max_iters=40, error_type="l1")
    assert cheb.convergence.iteration == want_iters and _rel(got, want) <= 1e-6, (cheb.convergence.iteration, want_iters, _rel(got, want))
    pr = pg.PageRank(0.85, error_type=pg.L1, tol=1e-9, max_iters=1000)
    got = _np(pr.rank(adj, p.copy()).np)
    want, want_iters = orc.pagerank(M, p, alpha=0.85, error_type="l1", tol=1e-9, max_iters=1000)
    assert pr.convergence.iteration == want_iters and _rel(got, want) <= 1e-6, (pr.convergence.iteration, want_iters, _rel(got, want))
    fmt = dense["g"].format()
    assert "f64 image: 8 column blocks" in fmt and "f64 propagation-blocking" not in fmt, fmt


def _stop_margin_ok(run_iters, p, stop, tol):
    """One iteration apart is accepted only when the oracle's own L1 change at that stop lies within f32 rounding (2 %) of the
    tolerance (test_gpu_batch_filters.py).  run_iters(k) -> the oracle's ranks after k iterations."""
    at_stop, before = run_iters(stop), run_iters(stop - 1)
    residual = np.abs(at_stop - before).sum() / np.abs(p).sum()
    return abs(residual - tol) <= 0.02 * tol, at_stop


def test_dense_propagate_64_columns(pg, dense):
    """64 personalizations through the multi-seed loops (one column block: the cold gathers stay in the stream, and here nearly
    every row is almost entirely cold): PageRank, HeatKernel and AbsorbingWalks; sampled columns against the oracle with the
    tolerances of test_gpu_batch_filters.test_scale23_batch_of_64; two runs bit-identical."""
    adj, M, n = dense["adj"], dense["M"], dense["n"]
    F = np.stack([dense["seeds"](10 + k) for k in range(64)], axis=1)
    X = pg.to_primitive(F)
    runs = (("pagerank", lambda: pg.PageRank(0.85, error_type=pg.L1, tol=1e-6, max_iters=1000),
             lambda p, **kw: orc.pagerank(M, p, alpha=0.85, eps=EPS32, **(kw or dict(error_type="l1", tol=1e-6, max_iters=1000)))),
            ("heat", lambda: pg.HeatKernel(5), lambda p, **kw: orc.heat_kernel(M, p, t=5, eps=EPS32, **kw)),
            ("absorbing", lambda: pg.AbsorbingWalks(0.85, error_type=pg.L1, tol=1e-6, max_iters=1000),
             lambda p, **kw: orc.absorbing_walks(M, p, alpha=0.85, eps=EPS32, **(kw or dict(error_type="l1", tol=1e-6, max_iters=1000)))))
    for name, make, oracle in runs:
        ranker = make()
        out = np.asarray(ranker.propagate(adj, X), dtype=np.float64)
        assert out.shape == (n, 64)
        iters = [c["iterations"] for batch in ranker.last_batches for c in batch]
        again = np.asarray(ranker.propagate(adj, X), dtype=np.float64)
        assert np.array_equal(out, again), name
        for j in (0, 37):
            want, it = oracle(F[:, j])
            if iters[j] != it:
                # (the L1 rules only: a residual within f32 rounding of the tolerance is decided one step apart; the heat kernel's
                # stops must agree)
                assert name != "heat" and abs(iters[j] - it) == 1, (name, j, iters[j], it)
                ok, want = _stop_margin_ok(lambda m: oracle(F[:, j], error_type="iters", max_iters=m)[0], F[:, j], iters[j], 1e-6)
                assert ok, (name, j, iters[j], it)
            assert _rel(out[:, j], want) <= 1e-6, (name, j, _rel(out[:, j], want))


# ------------------------------------------------------------------------------------------------------------------- C
N_C = 1 << 18                                  # one column block (n <= 2 M), list size max(65 536, n / 16) = 65 536
LIST_CAP = 65536
# the byte transport (254 / 255 / 256), kPbHeavyRow (16 384: a bin row; 16 385: a hub bin), kPbHubMax (65 536: one piece; 65 537:
# the first split hub row)
SPECIAL = (0, 1, 254, 255, 256, 16384, 16385, 65536, 65537)


def _known_cold_graph(listed):
    """Raw adjacency W (n x n, unit weights; W[i, j] = an edge from source i to output j, i.e. row j of the stored M^T references
    source i) whose every row of M^T has a cold count fixed by construction, `listed` rows with >= 255 of them.

    bsf_build counts the references of every source (the columns of M^T: k_source_counts), relabels the sources of a block by
    descending count (a stable sort: ties keep ascending ids) and makes the first min(HOT, blk) of them hot (k_bsf_is_hot).  Sources
    0 .. HOT - 1 get strictly more references than any other, so they are exactly the hot set, whatever the ties among them; sources
    0 .. HOT64 - 1 more than HOT64 .. HOT - 1, so the f64 image's hot set is known too.  Returns (W, cold per row, f64 cold per row)."""
    n, n_cold = N_C, N_C - HOT
    r = np.arange(n)
    cold = (r % 5).astype(np.int64)                               # 0 .. 4 cold entries on most rows
    special_rows = 28000 * np.arange(len(SPECIAL)) + 8            # (== 0 mod 4)
    listed_rows = np.flatnonzero(r % 4 == 1)[:listed - sum(c >= 255 for c in SPECIAL)]
    cold[listed_rows] = 255 + (listed_rows // 4) % 8              # 255 .. 262
    cold[special_rows] = SPECIAL
    assert np.count_nonzero(cold >= 255) == listed
    total = int(cold.sum())
    # cold entries: row after row, the next c sources of the cold ones round robin (distinct within a row: c < n_cold)
    cold_rows = np.repeat(r, cold)
    cold_src = HOT + np.arange(total) % n_cold
    most_cold_refs = -(-total // n_cold)
    # hot entries: every hot source referenced more often than any cold one, by rows round robin (distinct: refs < n)
    refs = np.where(np.arange(HOT) < HOT64, most_cold_refs + 2, most_cold_refs + 1)
    hot_src = np.repeat(np.arange(HOT), refs)
    hot_rows = np.arange(len(hot_src)) % n
    cold64 = cold + np.bincount(hot_rows[hot_src >= HOT64], minlength=n)
    src = np.concatenate([cold_src, hot_src])
    out = np.concatenate([cold_rows, hot_rows])
    W = sp.csr_array((np.ones(len(src)), (src, out)), shape=(n, n))
    assert W.nnz == len(src)                                      # no duplicate edges
    got_refs = np.diff(W.indptr)
    assert got_refs[HOT:].max() < got_refs[HOT64:HOT].min() and got_refs[HOT64:HOT].max() < got_refs[:HOT64].min()
    return W, cold, cold64


@pytest.fixture(scope="module")
def known_cold():
    built = {}

    def get(listed):
        if listed not in built:
            built[listed] = _known_cold_graph(listed)
        return built[listed]
    return get


@pytest.mark.parametrize("listed", [LIST_CAP, LIST_CAP + 1])
def test_known_cold_counts_fill_the_planner_list(pg, known_cold, listed):
    """The planner's list of rows with >= 255 cold entries filled to exactly its first size, and one beyond: the image holds every
    constructed cold entry (format()), every row's product matches fp64, hub and split hub rows included."""
    from pygrank_amd.device import DeviceGraph
    W, cold, _ = known_cold(listed)
    rng = np.random.default_rng(listed)
    with _env(PGH_PB_FORCE="1"):
        g = DeviceGraph.from_adjacency(W, "col")
    fmt = g.format()
    assert "bsf: 1 column blocks" in fmt and "heavy rows stay" not in fmt, fmt
    assert _cold_entries(fmt) == int(cold.sum()), (fmt, int(cold.sum()))
    MT, _ = _stored(g)
    _check_products(pg, g, MT, rng, listed)


@pytest.mark.parametrize("hub_max,in_stream", [(8192, (65537,)), (16, (16385, 65536, 65537))])
def test_known_cold_counts_hub_rows_in_the_stream(pg, known_cold, hub_max, in_stream):
    """PGH_PB_HUBMAX: 8 192 entries per piece splits the 16 385 / 65 536-entry rows into 3 / 8 pieces (8 = the number of source
    chunks) and leaves the 65 537-entry row (9 pieces) in the blocked stream; 16 gives the hub rows more than kPbMaxPieces = 1024
    pieces each: all three stay in the stream.  The image holds exactly the other rows' cold entries; every row's product matches."""
    from pygrank_amd.device import DeviceGraph
    W, cold, _ = known_cold(LIST_CAP + 1)
    rng = np.random.default_rng(hub_max)
    with _env(PGH_PB_FORCE="1", PGH_PB_HUBMAX=str(hub_max)):
        g = DeviceGraph.from_adjacency(W, "col")
    fmt = g.format()
    assert "(heavy rows stay in the stream)" in fmt, fmt
    assert _cold_entries(fmt) == int(cold.sum()) - sum(in_stream), (fmt, int(cold.sum()) - sum(in_stream))
    MT, _ = _stored(g)
    _check_products(pg, g, MT, rng, hub_max)


def test_known_cold_counts_f64_image(pg, known_cold):
    """The f64 image (one column block, PGH_BLOCKS64=1) of the graph whose f32 image fills the list exactly: the f64 hot cache holds
    20 224 sources, so every row's cold count grows by its references to sources 20 224 .. 29 695 and the f64 planner lists more
    rows than the f32 one -- beyond the list's first size (the graph uploads, and its first f64 route used to fail).  The f64 image
    holds every cold entry, and the "chebyshev" recurrence at tol = 1e-9 on it matches the oracle with equal iteration counts."""
    from pygrank_amd.device import DeviceGraph
    W, cold, cold64 = known_cold(LIST_CAP)
    assert np.count_nonzero(cold >= 255) == LIST_CAP < np.count_nonzero(cold64 >= 255)
    with _env(PGH_PB_FORCE="1", PGH_BLOCKS64="1"):
        g = DeviceGraph.from_adjacency(W, "col")
        _, M = _stored(g)
        p = np.zeros(N_C)
        p[np.random.default_rng(3).choice(N_C, 200, replace=False)] = 1.0
        cheb = pg.HeatKernel(5, coefficient_type="chebyshev", error_type=pg.L1, tol=1e-9, max_iters=40)
        got = _np(cheb.rank(_adjacency(g), p.copy()).np)
    fmt = g.format()
    assert "f64 image: 1 column blocks" in fmt, fmt
    assert _cold_entries(fmt, f64=True) == int(cold64.sum()), (fmt, int(cold64.sum()))
    want, want_iters = orc.heat_kernel(M, p, t=5, coefficient_type="chebyshev", tol=1e-9, max_iters=40, error_type="l1")
    assert cheb.convergence.iteration == want_iters and _rel(got, want) <= 1e-6, (cheb.convergence.iteration, want_iters, _rel(got, want))
