"""Subgraph, Supergraph, MabsMaintain, SeparateNormalization, Sequential, GraphSignal.top / nonzero and DeviceMatrix.top on the host test
double (no GPU) against the reference's recorded outcomes (tests/golden/golden_subgraph.npz).  The double lacks include/pgh_select.h, so
every caller takes its numpy route on the downloaded values here; numpy stand-ins put into ``_pgh_select_entries`` then show that the
engine routes hand over the right arguments and honour DECLINED.  tests/test_gpu_subgraph.py runs the same cases on the engine."""
import os
import re

import numpy as np
import pytest

import subgraph_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["pgh_mat_col_scale", "pgh_mat_split_blend", "pgh_mat_split_sums", "pgh_mat_topk", "pgh_vec_gather", "pgh_vec_scatter",
           "pgh_vec_select"]


@pytest.fixture(scope="module")
def fx():
    return np.load(sc.GOLDEN)


@pytest.fixture()
def stand_ins(host_engine):
    """The host double with numpy stand-ins for include/pgh_select.h; yields (pg, the log of their calls)."""
    from pygrank_amd import _lib as L
    cdll, log = L.lib(), []
    assert L.entry("pgh_vec_select") is None
    saved = cdll._pgh_select_entries
    cdll._pgh_select_entries = sc.numpy_entries(cdll, log)
    try:
        yield host_engine, log
    finally:
        cdll._pgh_select_entries = saved


def test_header_table_makefile_and_exports():
    from pygrank_amd import _lib
    import pygrank_amd as pg
    text = open(os.path.join(ROOT, "include", "pgh_select.h")).read()
    assert sorted(_lib.SELECT_SIGNATURES) == sorted(set(re.findall(r"\b(pgh_[a-z0-9_]+)\s*\(", text))) == ENTRIES
    assert _lib.TABLES["pgh_select.h"] is _lib.SELECT_SIGNATURES and "pgh_select.h" not in _lib.OPTIONAL
    for header, other in [("pgh.h", _lib.SIGNATURES), *[(h, t) for h, t in _lib.TABLES.items() if h != "pgh_select.h"]]:
        assert set(ENTRIES).isdisjoint(other), header

    def defined(name):
        return int(re.search(r"#define\s+" + name + r"\s+(\d+)", text).group(1))
    assert _lib.DECLINED == defined("PGH_SELECT_DECLINED") == 2
    assert (_lib.SELECT_NONZERO, _lib.SELECT_GT, _lib.SELECT_GE) == tuple(defined("PGH_SELECT_" + m) for m in ("NONZERO", "GT", "GE"))
    assert _lib.TOPK_MAX_K == defined("PGH_TOPK_MAX_K") == 4096 and _lib.SELECT_MAX_COLS == defined("PGH_SELECT_MAX_COLS") == 64
    makefile = open(os.path.join(ROOT, "pygrank_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bpgh_select\.hip\b", makefile, re.M)
    assert re.search(r"^_build/%\.o:.*include/pgh_select\.h\b", makefile, re.M)
    for name in ("Subgraph", "Supergraph", "MabsMaintain", "Sequential", "SeparateNormalization"):
        assert issubclass(getattr(pg, name), pg.Postprocessor), name


def test_host_double_has_no_select_entry(host_engine):
    from pygrank_amd import _lib
    assert all(_lib.entry(name) is None for name in ENTRIES)


def test_every_chain_has_a_case():
    have = sc.golden_stems()
    assert {name for _, name, _ in have} == {name for name, _ in sc.CHAINS}
    assert all(any(key == graph for graph, _, _ in have) for key in sc.GRAPHS) and len(have) >= 40


@pytest.mark.parametrize("wrapper", [False, True], ids=["networkx", "wrapper"])
@pytest.mark.parametrize("key,name,k", sc.golden_stems(), ids=lambda value: str(value))
def test_golden(host_engine, fx, key, name, k, wrapper):
    sc.check_case(host_engine, fx, key, name, k, wrapper)


@pytest.mark.parametrize("key,name,k", [case for case in sc.golden_stems() if case[1] in ("sub", "super", "noedge")],
                         ids=lambda value: str(value))
def test_golden_through_the_entries(stand_ins, fx, key, name, k):
    """The same cases with stand-ins for the entries: Subgraph asks pgh_vec_select for the non-zeros once and keeps its values vector,
    Supergraph scatters once, and neither looks at the host mirror."""
    pg, log = stand_ins
    sc.check_case(pg, fx, key, name, k, True)
    names = [call[0] for call in log]
    assert names.count("pgh_vec_select") == 1 and log[names.index("pgh_vec_select")][1] == 0
    assert names.count("pgh_vec_scatter") == (0 if name == "sub" else 1)
    if name != "sub":
        assert log[names.index("pgh_vec_scatter")][1] == (6 if name == "noedge" else k)


def test_subgraph_keeps_the_signal_on_the_device(stand_ins):
    pg, log = stand_ins
    A, directed, p = sc.adjacency("rmat10_dir")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    ranks = (sc.first_ranker(pg) >> pg.Top(8)).rank(graph, p.copy())
    sub = pg.Subgraph().transform(ranks)
    assert ranks._host is None and sub._host is None and isinstance(sub._np, pg.DeviceVector) and len(sub._np) == 8
    inner = sc.inner_ranker(pg).rank(sub.graph, sub)
    back = pg.Supergraph().transform(inner)
    assert inner._host is None and back._host is None and back.graph is graph
    assert [call[0] for call in log] == ["pgh_vec_select", "pgh_vec_scatter"]
    slow = pg.Supergraph()
    slow.fused = False
    assert np.array_equal(np.asarray(slow.transform(inner).np), np.asarray(back.np))
    assert len(log) == 2
    off = pg.Subgraph()
    off.fused = False
    again = off.transform(ranks)
    assert len(log) == 2 and np.array_equal(again.graph.original_nodes, sub.graph.original_nodes)
    assert np.array_equal(np.asarray(again.np), np.asarray(sub.np))


def test_select_comes_back_for_a_longer_list(stand_ins):
    pg, log = stand_ins
    n = 70001
    values = np.where(np.arange(n) % 40 == 0, 0.0, 1.0 + np.arange(n) % 7)
    values[5] = -0.0
    signal = pg.to_signal(pg.AdjacencyWrapper(__import__("scipy.sparse").sparse.eye_array(n, format="csr"), directed=True), values)
    positions, kept = signal.nonzero()
    want = np.flatnonzero(values != 0)
    assert positions.dtype == np.int32 and np.array_equal(positions, want) and isinstance(kept, pg.DeviceVector)
    assert np.array_equal(kept.numpy(), values[want]) and signal._host is None
    assert log == [("pgh_vec_select", 0, 0.0, 65536), ("pgh_vec_select", 0, 0.0, len(want))]
    slow_positions, slow_kept = signal.nonzero(fused=False)
    assert np.array_equal(slow_positions, positions) and np.array_equal(slow_kept, values[want]) and len(log) == 2


def _ties(n):
    values = np.asarray([3.0, 1.0, 3.0, -0.0, 0.0, 7.5, 1.0, 3.0, -2.0, 0.0][:n])
    return values


@pytest.mark.parametrize("engine", ["double", "stand_ins"])
def test_signal_top_and_matrix_top(host_engine, engine):
    from pygrank_amd import _lib as L
    pg, log = host_engine, []
    cdll = L.lib()
    assert L.entry("pgh_mat_topk") is None
    saved = cdll._pgh_select_entries
    if engine == "stand_ins":
        cdll._pgh_select_entries = sc.numpy_entries(cdll, log)
    try:
        import networkx as nx
        values = _ties(10)
        named = nx.path_graph(["a", "b", "c", "d", "e", "f", "g", "h", "i", "j"])
        signal = pg.to_signal(named, dict(zip(named, values.tolist())))
        assert signal.top(4) == [("f", 7.5), ("a", 3.0), ("c", 3.0), ("h", 3.0)]
        assert [node for node, _ in signal.top(99)] == ["f", "a", "c", "h", "b", "g", "d", "e", "j", "i"]     # clipped to the ten nodes
        assert signal.top(0) == []
        positions = pg.to_signal(pg.AdjacencyWrapper(nx.to_scipy_sparse_array(named), directed=False), values)
        assert positions.top(3) == [(5, 7.5), (0, 3.0), (2, 3.0)]
        rng = np.random.default_rng(4)
        wide = np.round(rng.standard_normal((50, 70)) * 2) / 2                  # many ties; 70 columns: two chunks
        slab = pg.DeviceMatrix.from_host(wide)
        for k in (1, 7, 50):
            rows, scores = slab.top(k)
            order = np.stack([np.lexsort((np.arange(50), -wide[:, j])) for j in range(70)], axis=1)[:k]
            assert rows.dtype == np.int32 and rows.shape == scores.shape == (k, 70)
            assert np.array_equal(rows, order) and np.array_equal(scores, np.take_along_axis(wide, order, axis=0))
        for k in (0, 51):
            with pytest.raises(L.EngineError, match="outside"):
                slab.top(k)
        tall = pg.DeviceMatrix.from_host(rng.standard_normal((5000, 2)))
        before = len(log)
        rows, _ = tall.top(4097)                                                # above PGH_TOPK_MAX_K: numpy, the entry is not asked
        assert len(log) == before and np.array_equal(rows[:, 1], np.lexsort((np.arange(5000), -tall.numpy()[:, 1]))[:4097])
        if engine == "stand_ins":
            assert [call for call in log if call[0] == "pgh_mat_topk"][:4] == [("pgh_mat_topk", 4), ("pgh_mat_topk", 10),
                                                                               ("pgh_mat_topk", 3), ("pgh_mat_topk", 1)]
            cdll._pgh_select_entries = dict(cdll._pgh_select_entries, pgh_mat_topk=lambda *args: (log.append("declined"), 2)[1])
            rows, scores = slab.top(7)                                          # DECLINED: the numpy route, the same lists
            order = np.stack([np.lexsort((np.arange(50), -wide[:, j])) for j in range(70)], axis=1)[:7]
            assert log[-1] == "declined" and np.array_equal(rows, order)
        else:
            assert log == []
    finally:
        cdll._pgh_select_entries = saved


def test_refusals(host_engine):
    pg = host_engine
    A, directed, p = sc.adjacency("weighted300_dir")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    with pytest.raises(Exception, match="no non-zero score: the subgraph would be empty"):
        pg.Subgraph().transform(pg.to_signal(graph, np.zeros(300)))
    with pytest.raises(Exception, match="no non-zero score"):
        pg.Subgraph().rank(graph, np.zeros(300))

    class Bare:
        def __len__(self):
            return 3

        def __iter__(self):
            return iter(range(3))
    with pytest.raises(Exception, match="Subgraph needs an AdjacencyWrapper or a graph with a networkx-style subgraph"):
        pg.Subgraph().transform(pg.to_signal(Bare(), [1.0, 0.0, 2.0]))
    with pytest.raises(Exception, match="no outcome of Subgraph"):
        pg.Supergraph().transform(pg.to_signal(graph, p.copy()))
    with pytest.raises(Exception, match="Subgraph has no propagate"):
        (sc.first_ranker(pg) >> pg.Top(8) >> pg.Subgraph()).propagate(graph, np.stack([p, p], axis=1))
    with pytest.raises(Exception, match="outside the graph"):
        graph.subgraph([1, 300])
    sub = graph.subgraph([7, 2, 2, 250])
    assert sub.original_nodes.tolist() == [2, 7, 250] and len(sub) == 3 and sub.directed == directed
    assert (sub.adj != A[[2, 7, 250]][:, [2, 7, 250]]).nnz == 0


@pytest.mark.parametrize("engine", ["double", "stand_ins"])
@pytest.mark.parametrize("width", [1, 5, 65])
def test_propagate_routes(host_engine, engine, width):
    """MabsMaintain and SeparateNormalization keep the inner batch; a chain that ends in Supergraph runs column by column."""
    from pygrank_amd import _lib as L
    pg, log = host_engine, []
    cdll = L.lib()
    L.entry("pgh_mat_col_scale")
    saved = cdll._pgh_select_entries
    if engine == "stand_ins":
        cdll._pgh_select_entries = sc.numpy_entries(cdll, log)
    try:
        A, directed, _ = sc.adjacency("weighted300_dir")
        graph = pg.AdjacencyWrapper(A, directed=directed)
        F = np.abs(np.random.default_rng(width).standard_normal((300, width))) * (np.random.default_rng(1).random((300, width)) < 0.2)
        F[0, :] = 1.0
        route = "slab" if engine == "stand_ins" else "columns"
        chunks = [min(64, width - first) for first in range(0, width, 64)] if route == "slab" else [width]
        for make in (lambda: pg.MabsMaintain(sc.first_ranker(pg)),
                     lambda: pg.SeparateNormalization(sc.separator(300, False), sc.first_ranker(pg)),
                     lambda: pg.SeparateNormalization(sc.first_ranker(pg), sc.separator(300, True))):
            post = make()
            got = post.propagate(graph, F).numpy()
            assert post.last_propagate["route"] == route and post.last_propagate["chunks"] == chunks
            assert len(post.ranker.last_batches) >= 1                          # the inner ranker ran as a batch
            for j in range(0, width, 7):
                alone = np.asarray(make().rank(graph, F[:, j].copy()).np, dtype=np.float64)
                assert sc.rel_linf(got[:, j], alone) <= 1e-6
            for switch, other in (("fused", "columns"), ("batch", "ranks")):
                off = make()
                setattr(off, switch, False)
                again = off.propagate(graph, F).numpy()
                assert off.last_propagate["route"] == other and sc.rel_linf(again, got) <= 1e-6
        if engine == "stand_ins":
            assert {call[0] for call in log} == {"pgh_mat_col_scale", "pgh_mat_split_sums", "pgh_mat_split_blend"}
        if width == 5:
            def chain():
                inner = pg.PageRank(0.5, tol=1e-6, error_type=pg.L1, max_iters=1000)
                return sc.first_ranker(pg) >> pg.Top(8) >> pg.Subgraph() >> inner >> pg.Supergraph()
            whole = chain()
            many = whole.propagate(graph, F).numpy()
            assert whole.last_propagate["route"] == "ranks" and np.all((many != 0).sum(axis=0) == 8)
            for j in range(width):
                assert np.array_equal(many[:, j], np.asarray(chain().rank(graph, F[:, j].copy()).np, dtype=np.float64))
    finally:
        cdll._pgh_select_entries = saved
