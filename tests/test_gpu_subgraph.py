"""Subgraph, Supergraph, MabsMaintain, SeparateNormalization and Sequential on the GPU against the reference's recorded outcomes
(tests/golden/golden_subgraph.npz; the cases and their bars are those of tests/test_subgraph_host.py), on networkx graphs and on
AdjacencyWrapper graphs, where the selection must leave the device as a list: no host mirror of a signal exists after Subgraph and
Supergraph.

The slab routes of MabsMaintain and SeparateNormalization (include/pgh_select.h) against the same propagate's column route and against one
rank() per column, widths 1, 5, 64, 65.  Both routes start from the same inner columns (the column route cuts them out of the same batch;
where one rank() per column is the partner the inner ranker is the elementwise Transformer, whose slab pass and column pass store the same
bits).  They differ only in the order of an f64 sum of n f32 terms, which can move each of a column's two f32 scalars by one rounding, and
each scalar enters one f32 operation per element; every operand here is non-negative, so nothing cancels.  The bound is therefore 4 f32
ulps per element -- derived, not measured; the largest difference seen is printed (DESIGN.md section 22 records it).  Where a column's
scalars are bit-equal on both routes, the column must be bit-equal."""
import numpy as np
import pytest

import subgraph_common as sc

pytestmark = pytest.mark.gpu

WIDTHS = (1, 5, 64, 65)
ULPS = 4


@pytest.fixture(scope="module")
def fx():
    return np.load(sc.GOLDEN)


@pytest.mark.parametrize("wrapper", [False, True], ids=["networkx", "wrapper"])
@pytest.mark.parametrize("key,name,k", sc.golden_stems(), ids=lambda value: str(value))
def test_golden(gpu_engine, fx, key, name, k, wrapper):
    from pygrank_amd import _lib as L
    assert all(L.entry(entry) is not None for entry in L.SELECT_SIGNATURES)
    sc.check_case(gpu_engine, fx, key, name, k, wrapper)


@pytest.mark.parametrize("key", sc.GRAPHS)
@pytest.mark.parametrize("k", sc.KS)
def test_nothing_is_downloaded_on_a_wrapper(gpu_engine, key, k):
    pg = gpu_engine
    A, directed, p = sc.adjacency(key)
    graph = pg.AdjacencyWrapper(A, directed=directed)
    ranks = (sc.first_ranker(pg) >> pg.Top(k)).rank(graph, p.copy())
    sub = pg.Subgraph().transform(ranks)
    assert ranks._host is None and sub._host is None and isinstance(sub._np, pg.DeviceVector) and len(sub._np) == k
    inner = pg.PageRank(0.5, tol=1e-6, error_type=pg.L1, max_iters=1000).rank(sub.graph, sub)
    back = pg.Supergraph().transform(inner)
    assert inner._host is None and back._host is None and back.graph is graph and isinstance(back._np, pg.DeviceVector)
    mirror = pg.Supergraph()
    mirror.fused = False
    assert np.array_equal(np.asarray(mirror.transform(inner).np), np.asarray(back.np))
    assert np.array_equal(np.flatnonzero(np.asarray(back.np)), sub.graph.original_nodes)
    top = ranks.top(k)
    assert ranks._host is None and sorted(node for node, _ in top) == sub.graph.original_nodes.tolist()
    positions, values = ranks.nonzero()
    assert ranks._host is None and np.array_equal(positions, sub.graph.original_nodes) and np.all(values.numpy() == 1.0)


def _ordered(values):
    """f32 values as integers whose order and spacing are those of the values: neighbours differ by 1."""
    bits = np.asarray(values, dtype=np.float64).astype(np.float32).view(np.int32).astype(np.int64)
    return np.where(bits < 0, -(bits & 0x7FFFFFFF), bits)


def _ulps_apart(a, b):
    return np.abs(_ordered(a) - _ordered(b))


def _f32(value):
    return np.float32(value).view(np.uint32)


def _features(n, width):
    rng = np.random.default_rng(100 + width)
    return np.abs(rng.standard_normal((n, width))) * (rng.random((n, width)) < 0.3) + (np.arange(n) % 97 == 0)[:, None]


def _mabs_scalars(pg, F, inner):
    """Per column {route: its f32 factor}: the slab route takes both sums from slab reductions, the column route the ranks' sum from a
    vector reduction, one rank() per column both."""
    norms, totals = F.col_abssum(), inner.col_abssum()
    scalars = []
    for j, column in enumerate(inner.columns()):
        alone_norm, alone_total = float(pg.sum(pg.abs(F.column(j)))), float(pg.sum(pg.abs(column)))
        scalars.append(dict(slab=(_f32(norms[j] * (1.0 / totals[j])),), columns=(_f32(norms[j] * (1.0 / alone_total)),),
                            ranks=(_f32(alone_norm * (1.0 / alone_total)),)))
    return scalars


def _split_scalars(pg, separator, inner):
    sums = np.concatenate([part.split_sums(separator) for _, part in inner.chunks()])      # (an entry takes at most 64 columns)
    scalars = []
    for j, column in enumerate(inner.columns()):
        first, second = float(pg.sum(column * separator)), float(pg.sum(column * (1 - separator)))
        alone = tuple(_f32(pg.safe_div(1., s)) for s in (first, second))
        scalars.append(dict(slab=tuple(_f32(pg.safe_div(1., float(s))) for s in sums[j]), columns=alone, ranks=alone))
    return scalars


@pytest.mark.parametrize("inner_kind", ["pagerank", "transformer"])
@pytest.mark.parametrize("post_kind", ["mabs", "sep_fraction", "sep_binary"])
@pytest.mark.parametrize("width", WIDTHS)
def test_slab_routes(gpu_engine, width, post_kind, inner_kind):
    pg = gpu_engine
    A, directed, _ = sc.adjacency("rmat10_dir")
    n = A.shape[0]
    graph = pg.AdjacencyWrapper(A, directed=directed)
    F = _features(n, width)
    separator = sc.separator(n, post_kind == "sep_binary")

    def inner():
        return sc.first_ranker(pg) if inner_kind == "pagerank" else pg.Transformer()

    def make():
        return pg.MabsMaintain(inner()) if post_kind == "mabs" else pg.SeparateNormalization(separator, inner())
    post = make()
    got = post.propagate(graph, F).numpy()
    assert post.last_propagate["route"] == "slab"
    assert post.last_propagate["chunks"] == [min(64, width - first) for first in range(0, width, 64)]
    columns = make()
    columns.fused = False
    partner = columns.propagate(graph, F).numpy()
    assert columns.last_propagate["route"] == "columns"
    batch = inner().propagate(graph, F)
    slab = pg.DeviceMatrix.from_host(F)
    device_separator = pg.to_signal(graph, separator).np
    scalars = _mabs_scalars(pg, slab, batch) if post_kind == "mabs" else _split_scalars(pg, device_separator, batch)
    partners = [("columns", partner)]
    if inner_kind == "transformer":                                            # one rank() per column starts from the same bits
        ranks = make()
        ranks.batch = False
        partners.append(("ranks", ranks.propagate(graph, F).numpy()))
        assert ranks.last_propagate["route"] == "ranks"
    for label, other in partners:
        apart = _ulps_apart(got, other)
        equal = [j for j, column in enumerate(scalars) if column["slab"] == column[label]]
        print(f"slab route of {post_kind} over {inner_kind}, width {width}, against {label}: largest difference {int(apart.max())} ulp, "
              f"{len(equal)} of {width} columns with equal scalars")
        assert apart.max() <= ULPS, (label, int(apart.max()))
        for j in equal:
            assert np.array_equal(got[:, j], other[:, j]), (label, j)


def test_chain_propagate_runs_column_by_column(gpu_engine):
    pg = gpu_engine
    A, directed, _ = sc.adjacency("weighted300_dir")
    graph = pg.AdjacencyWrapper(A, directed=directed)
    F = _features(300, 3)

    def chain():
        inner = pg.PageRank(0.5, tol=1e-6, error_type=pg.L1, max_iters=1000)
        return sc.first_ranker(pg) >> pg.Top(8) >> pg.Subgraph() >> inner >> pg.Supergraph()
    whole = chain()
    many = whole.propagate(graph, F).numpy()
    assert whole.last_propagate["route"] == "ranks" and np.all((many != 0).sum(axis=0) == 8)
    for j in range(3):
        assert np.array_equal(many[:, j], np.asarray(chain().rank(graph, F[:, j].copy()).np, dtype=np.float64))
    with pytest.raises(Exception, match="Subgraph has no propagate"):
        (sc.first_ranker(pg) >> pg.Top(8) >> pg.Subgraph()).propagate(graph, F)
