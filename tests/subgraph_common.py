"""Shared by tests/golden/make_golden_subgraph.py, tests/test_subgraph_host.py and tests/test_gpu_subgraph.py: the graphs, the chains and
the cases of tests/golden/golden_subgraph.npz.  Every builder takes the package as `pg`, so the generator hands in the reference and the
tests pygrank_amd: one text builds both sides of a comparison."""
import os

import numpy as np
import scipy.sparse as sp

import cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_subgraph.npz")
GRAPHS = ["rmat10_dir", "rmat10_und", "weighted300_dir", "weighted300_und"]
KS = (8, 100)
# name -> k (None: the chain has no Top of its own)
CHAINS = [("top", k) for k in KS] + [("sub", k) for k in KS] + [("super", k) for k in KS] + \
         [("noedge", None), ("mabs", None), ("sep_binary", None), ("sep_fraction", None), ("sequential", None)]


def stem(key, name, k):
    return f"{key}/{name}" + ("" if k is None else f"_k{k}")


def adjacency(key):
    """(A csr, directed, personalization array); "_und" is the symmetric graph max(A, A^T)."""
    base, kind = key.rsplit("_", 1)
    A, _, p = cases.GRAPHS["rmat10_dir" if base == "rmat10" else base]()
    A = sp.csr_array(A, dtype=np.float64)
    if kind == "und":
        A = sp.csr_array(A.maximum(A.T))
    A.sort_indices()
    return A, kind == "dir", p


def nx_graph(key):
    """(networkx graph over the nodes 0 .. n - 1, personalization {node: value})."""
    import networkx as nx
    A, directed, p = adjacency(key)
    G = nx.from_scipy_sparse_array(A, create_using=nx.DiGraph if directed else nx.Graph)
    return G, {int(i): float(p[i]) for i in np.flatnonzero(p)}


def independent_scores(A, count=6):
    """{node: score} over `count` nodes no two of which share an edge and none of which has a self loop: their induced subgraph has no
    edge."""
    S = sp.csr_array(A + A.T)
    chosen = []
    for u in range(A.shape[0] // 3, A.shape[0]):
        near = set(S.indices[S.indptr[u]:S.indptr[u + 1]].tolist())
        if u not in near and not near.intersection(chosen):
            chosen.append(u)
            if len(chosen) == count:
                break
    assert len(chosen) == count
    return {int(u): 1.0 + 0.25 * i for i, u in enumerate(chosen)}


def separator(n, binary):
    rng = np.random.default_rng(17)
    return (rng.random(n) < 0.4).astype(np.float64) if binary else np.round(rng.random(n) * 8) / 8


def first_ranker(pg):
    return pg.PageRank(0.85)


def inner_ranker(pg, error_type=None):
    return pg.PageRank(0.9, tol=1e-6, error_type=pg.L1 if error_type is None else error_type)


def build(pg, name, k=None, inner=None, n=None):
    """(the chain, its inner PageRank or None)."""
    if name == "top":
        return first_ranker(pg) >> pg.Top(k), None
    if name == "sub":
        return first_ranker(pg) >> pg.Top(k) >> pg.Subgraph(), None
    inner = inner_ranker(pg) if inner is None else inner
    if name == "super":
        return first_ranker(pg) >> pg.Top(k) >> pg.Subgraph() >> inner >> pg.Supergraph(), inner
    if name == "noedge":
        return pg.Subgraph() >> inner >> pg.Supergraph(), inner
    if name == "mabs":
        return pg.MabsMaintain(first_ranker(pg)), None
    if name in ("sep_binary", "sep_fraction"):
        return pg.SeparateNormalization(separator(n, name == "sep_binary"), first_ranker(pg)), None
    if name == "sequential":
        return pg.Sequential(first_ranker(pg), pg.Normalize(), pg.Top(3)), None
    raise KeyError(name)


def run(pg, graph, personalization, A, name, k, inner=None):
    """(the outcome signal, the inner PageRank or None) of one chain on `graph`."""
    chain, inner = build(pg, name, k, inner, A.shape[0])
    given = independent_scores(A) if name == "noedge" else personalization
    return chain(graph, pg.to_signal(graph, given)), inner


def dense(signal, n=None):
    """The signal's scores by node as an f64 array over the nodes 0 .. n - 1 of the graph it lives on (n = None: all of them)."""
    n = len(signal) if n is None else n
    out = np.zeros(n)
    for node, value in signal.items():
        out[int(node)] = float(value)
    return out


# ---- comparisons
def rel_linf(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = float(np.max(np.abs(want))) if want.size else 0.0
    return float(np.max(np.abs(got - want))) / scale if scale > 0 else float(np.max(np.abs(got), initial=0.0))


def golden_stems():
    """[(graph, chain, k)] of the cases the fixture file holds (the generator leaves out what misses its conditions)."""
    with np.load(GOLDEN) as fx:
        have = {key.rsplit("/", 1)[0] for key in fx.files}
    return [(key, name, k) for key in GRAPHS for name, k in CHAINS if stem(key, name, k) in have]


def check_case(pg, fx, key, name, k, wrapper):
    """One golden case through pygrank_amd on the networkx graph (wrapper = False) or on an AdjacencyWrapper: node sets exactly, scores
    within parity_common.tolerance_for, the inner run's iterations exactly.  Returns the outcome signal."""
    import parity_common
    bar = parity_common.tolerance_for({})
    A, directed, p = adjacency(key)
    n = A.shape[0]
    if wrapper:
        graph, personalization = pg.AdjacencyWrapper(A, directed=directed), p.copy()
    else:
        graph, personalization = nx_graph(key)
    signal, inner = run(pg, graph, personalization, A, name, k)
    want = {part: fx[stem(key, name, k) + "/" + part] for part in ("nodes", "ranks", "iterations") if stem(key, name, k) + "/" + part in fx}
    if name == "top":
        assert signal.graph is graph
        assert np.array_equal(np.flatnonzero(dense(signal, n)), want["nodes"])
    elif name == "sub":
        sub = signal.graph
        assert sub._pygrank_original_graph is graph and len(sub) == len(signal) == k
        if wrapper:
            assert isinstance(sub, pg.AdjacencyWrapper) and sub.directed == directed and sub.original_nodes.dtype == np.int32
            assert np.array_equal(sub.original_nodes, want["nodes"])
            assert (sub.adj != A[want["nodes"]][:, want["nodes"]]).nnz == 0
            scores = np.asarray(signal.np, dtype=np.float64)
        else:
            assert sorted(int(node) for node in signal) == want["nodes"].tolist()
            scores = np.asarray([signal[int(node)] for node in want["nodes"]])
        assert rel_linf(scores, want["ranks"]) <= bar
    else:
        assert signal.graph is graph and len(signal) == n
        if name == "sequential":
            assert np.array_equal(dense(signal, n), want["ranks"])
        else:
            assert rel_linf(dense(signal, n), want["ranks"]) <= bar, rel_linf(dense(signal, n), want["ranks"])
        if inner is not None:
            assert int(inner.convergence.iteration) == int(want["iterations"])
    return signal


# ---- include/pgh_select.h in numpy through the transfers of `lib`: stand-ins that let the engine routes run on the host test double
def numpy_entries(lib, log):
    """{name: callable} with the signatures of include/pgh_select.h; every call is noted in `log` as (name, its plain arguments)."""
    import ctypes as C

    def vec_down(h):
        out = np.empty(lib.pgh_vec_len(h), dtype=np.float32)
        if len(out):
            assert lib.pgh_vec_d2h_f32(h, out.ctypes.data_as(C.c_void_p), len(out)) == 0
        return out

    def vec_up(h, values):
        values = np.ascontiguousarray(values, dtype=np.float32)
        if len(values):
            assert lib.pgh_vec_h2d_f32(h, values.ctypes.data_as(C.c_void_p), len(values)) == 0

    def mat_down(h):
        n, b = C.c_int64(), C.c_int32()
        assert lib.pgh_mat_shape(h, C.byref(n), C.byref(b)) == 0
        out = np.empty((n.value, b.value), dtype=np.float64)
        assert lib.pgh_mat_d2h_f64(h, out.ctypes.data_as(C.c_void_p)) == 0
        return out.astype(np.float32)

    def mat_up(h, values):
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert lib.pgh_mat_h2d_f64(h, values.ctypes.data_as(C.c_void_p)) == 0

    def select(x, mode, cut, capacity, idx_host, values, count):
        log.append(("pgh_vec_select", mode, cut, capacity))
        host = vec_down(x)
        hit = np.flatnonzero(host != 0 if mode == 0 else (host > np.float32(cut) if mode == 1 else host >= np.float32(cut)))
        C.cast(count, C.POINTER(C.c_int64))[0] = len(hit)
        if len(hit) <= capacity:
            for t, at in enumerate(hit):
                idx_host[t] = int(at)
            if values is not None:
                assert lib.pgh_vec_len(values) >= capacity
                stored = vec_down(values)
                stored[:len(hit)] = host[hit]
                vec_up(values, stored)
        return 0

    def listed(idx_host, count):
        return np.asarray([idx_host[t] for t in range(count)], dtype=np.int64)

    def gather(x, idx_host, count, out):
        log.append(("pgh_vec_gather", count))
        stored = vec_down(out)
        stored[:count] = vec_down(x)[listed(idx_host, count)]
        vec_up(out, stored)
        return 0

    def scatter(dst, idx_host, count, src):
        log.append(("pgh_vec_scatter", count))
        at = listed(idx_host, count)
        assert np.all(np.diff(at) > 0)
        stored = vec_down(dst)
        stored[at] = vec_down(src)[:count]
        vec_up(dst, stored)
        return 0

    def topk(m, k, idx_host, val_host):
        log.append(("pgh_mat_topk", k))
        host = mat_down(m)
        if k > 4096 or host.shape[1] > 64:
            return 2
        for j in range(host.shape[1]):
            order = np.lexsort((np.arange(len(host)), -host[:, j]))[:k]
            for t, row in enumerate(order):
                idx_host[t * host.shape[1] + j] = int(row)
                val_host[t * host.shape[1] + j] = float(host[row, j])
        return 0

    def col_scale(m, scale_host, out):
        host = mat_down(m)
        log.append(("pgh_mat_col_scale", host.shape[1]))
        mat_up(out, host * np.asarray([scale_host[j] for j in range(host.shape[1])], dtype=np.float32)[None, :])
        return 0

    def split_sums(m, s, sums_host):
        host, sep = mat_down(m), vec_down(s)
        log.append(("pgh_mat_split_sums", host.shape[1]))
        first, second = host * sep[:, None], host * (np.float32(1) - sep)[:, None]
        for j in range(host.shape[1]):
            sums_host[2 * j], sums_host[2 * j + 1] = float(first[:, j].astype(np.float64).sum()), float(second[:, j].astype(np.float64).sum())
        return 0

    def split_blend(m, s, a_host, b_host, out):
        host, sep = mat_down(m), vec_down(s)
        log.append(("pgh_mat_split_blend", host.shape[1]))
        a = np.asarray([a_host[j] for j in range(host.shape[1])], dtype=np.float32)[None, :]
        b = np.asarray([b_host[j] for j in range(host.shape[1])], dtype=np.float32)[None, :]
        mat_up(out, (host * sep[:, None]) * a + (host * (np.float32(1) - sep)[:, None]) * b)
        return 0
    return dict(pgh_vec_select=select, pgh_vec_gather=gather, pgh_vec_scatter=scatter, pgh_mat_topk=topk, pgh_mat_col_scale=col_scale,
                pgh_mat_split_sums=split_sums, pgh_mat_split_blend=split_blend)
