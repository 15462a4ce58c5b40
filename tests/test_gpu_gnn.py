"""include/pgh_gnn.h and pygrank_amd.gnn on the GPU: the transposed graph, its mirrored mask, the resident linear loop and
differentiable_propagate under graph_dropout.

Every reference is numpy in f64 on the downloaded stored matrix MT = CSR(M^T) and the mask twin of tests/kernel_checks.py
(check_graph_dropout_batched: splitmix64 of (seed, index of the entry in CSR(M^T) order)); an adjoint is computed with the explicit .T
of each step's masked matrix, by the chain rule, never with the plans of gnn.linear_plan.  Tolerances are the project's own:
2.5 * EPS32 * (|A| @ |X|) for a product, 2e-6 * max|want| for a loop."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cases
from oracle import rmat_np

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
WIDTHS = (3, 20, 64, 70)          # the three lanes-per-row shapes of k_mm_partial, and two chunks
RATES = (0.5, 0.3)
STEPS = (6, 10)


@pytest.fixture(scope="module")
def pg():
    import pygrank_amd
    from pygrank_amd import _lib
    pygrank_amd.load_backend("hip")
    assert _lib.runtime_name().startswith("hip:")
    return pygrank_amd


def mask_of(MT, rate, seed):
    e = np.arange(MT.nnz, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = rmat_np.splitmix64(np.uint64(seed) ^ (e * np.uint64(0xD6E8FEB86659FD93)))
    keep = (h >> np.uint64(32)).astype(np.int64) >= int(np.floor(rate * 4294967296.0))
    data = (MT.data.astype(F32) * np.float32(1.0 / (1.0 - rate))).astype(F32).astype(np.float64) * keep
    return sp.csr_array((data, MT.indices, MT.indptr), shape=MT.shape)


class Case:
    """One graph: its wrapper and preprocessor, the device graph g, its transposed graph gt, MT in f64, and the masked matrices by
    (rate, seed), each built once."""

    def __init__(self, pg, adjacency, directed, normalization):
        self.graph = pg.AdjacencyWrapper(adjacency, directed=directed)
        self.pre = pg.preprocessor(normalization=normalization, assume_immutability=True)
        M = self.pre(self.graph)
        self.g = getattr(M, "array", M)
        self.n = adjacency.shape[0]
        self.stored = self.g.download_transposed()                 # f32 values
        self.MT = sp.csr_array((self.stored.data.astype(np.float64), self.stored.indices, self.stored.indptr), shape=self.stored.shape)
        self.gt = self.g.transposed()
        self._masked = {}

    def A(self, rate, seed):
        """The matrix step `seed` multiplies with: MT under its mask (MT itself for rate 0)."""
        if rate == 0:
            return self.MT
        key = (rate, int(seed))
        if key not in self._masked:
            self._masked[key] = mask_of(self.stored, rate, seed)
        return self._masked[key]


@pytest.fixture(scope="module")
def graph_cases(pg):
    rng = np.random.default_rng(21)
    A = rmat_np.rmat_csr(11, 8, seed=5)                            # directed multigraph: value-free stream, repeated entries share a bit
    W = sp.csr_array(A)
    W.data = rng.uniform(0.5, 2.0, W.nnz)                          # valued stream
    E, directed, _ = cases.GRAPHS["er10k"]()
    assert not directed
    out = dict(multi=Case(pg, A, True, "col"), weighted=Case(pg, W, True, "col"), sym=Case(pg, E, False, "symmetric"))
    assert "f32-valued" in out["weighted"].g.format()
    assert abs(out["sym"].MT - out["sym"].MT.T).max() == 0         # M = M^T
    return out


def _slab(rng, n, b):
    """Non-negative, a zero column when there is room for one."""
    X = rng.random((n, b)).astype(F32).astype(np.float64)
    if b >= 3:
        X[:, 1] = 0.0
    return X


def _product_bound(A, X):
    return 2.5 * EPS32 * (abs(A) @ np.abs(X)) + 1e-30


def _spmm_dropout(pg, g, X, rate, seed):
    from pygrank_amd.device import DeviceMatrix, DroppedGraph
    parts = [np.asarray(DroppedGraph(g, rate, seed).conv(DeviceMatrix.from_host(np.ascontiguousarray(X[:, s:s + 64]))))
             for s in range(0, X.shape[1], 64)]
    return np.concatenate(parts, axis=1)


# ------------------------------------------------------------------------------------------------- 1. the transposed graph
@pytest.mark.parametrize("name", ["multi", "weighted", "sym"])
def test_transposed_graph_is_the_scipy_transpose(pg, graph_cases, name):
    case = graph_cases[name]
    assert case.gt is not None and case.gt.shape == case.g.shape and case.gt.nnz == case.g.nnz
    got, want = case.gt.download_transposed(), sp.csr_array(case.stored.T.tocsr())
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.data.view(np.uint32), want.data.astype(F32).view(np.uint32))
    assert ("value-free" in case.gt.format()) == ("value-free" in case.g.format())
    rng = np.random.default_rng(3)
    T = case.MT.T.tocsr()                                          # what gt stores: its conv is x -> M x
    x = rng.random(case.n).astype(F32).astype(np.float64)
    got = np.asarray(pg.conv(pg.to_primitive(x), case.gt))
    assert np.all(np.abs(got - T @ x) <= _product_bound(T, x)), name
    X = _slab(rng, case.n, 20)
    got = np.asarray(pg.conv(pg.to_primitive(X), case.gt))
    assert np.all(np.abs(got - T @ X) <= _product_bound(T, X)), name
    deg = np.asarray(pg.degrees(case.gt))                          # row sums of gt's M = of the stored matrix of g
    want = np.asarray(case.MT.sum(axis=1)).ravel()
    assert np.all(np.abs(deg - want) <= 2.5 * EPS32 * np.abs(want) + 1e-30)


def test_transposed_graph_refusals(pg, monkeypatch):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceGraph
    entry = L.entry("pgh_graph_transposed")
    rect = DeviceGraph.from_scipy(sp.random(40, 30, density=0.2, random_state=1, format="csr"))
    monkeypatch.setenv("PGH_FORMAT", "csr")                        # read when a graph is built: no blocked layout
    plain = DeviceGraph.from_scipy(sp.random(50, 50, density=0.2, random_state=2, format="csr"))
    monkeypatch.delenv("PGH_FORMAT")
    assert "row-major" in plain.format()
    for g in (rect, plain):
        h = L.c_graph()
        assert entry(g._h, C.byref(h)) == L.DECLINED and h.value is None
        assert g.transposed() is None
    h = L.c_graph()
    assert entry(None, C.byref(h)) not in (0, L.DECLINED) and h.value is None


# ------------------------------------------------------------------------------------------------- 2. the mirrored mask
@pytest.mark.parametrize("name", ["multi", "weighted", "sym"])
def test_mirrored_mask(pg, graph_cases, name):
    """gt under the mask of a seed is the TRANSPOSE of g under that mask: a wrong pairing of entries is an error of the size of
    the values themselves."""
    case = graph_cases[name]
    rng = np.random.default_rng(31)
    for rate, seed in ((0.5, 7), (0.3, 12345), (0.5, 2 ** 40 + 3)):
        AT = case.A(rate, seed).T.tocsr()
        for b in WIDTHS:
            X = _slab(rng, case.n, b)
            got = _spmm_dropout(pg, case.gt, X, rate, seed)
            assert got.shape == X.shape and np.all(np.abs(got - AT @ X) <= _product_bound(AT, X)), (name, rate, seed, b)
        if name == "sym":                                          # M = M^T, but the mask is not symmetric
            own = _spmm_dropout(pg, case.g, X, rate, seed)
            assert np.all(np.abs(own - case.A(rate, seed) @ X) <= _product_bound(case.A(rate, seed), X))
            assert np.max(np.abs(own - got)) > 0.01 * np.max(np.abs(got))


def test_single_vector_dropout_is_refused_on_a_transposed_graph(pg, graph_cases):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceVector, DroppedGraph
    case = graph_cases["weighted"]
    x = DeviceVector.from_host(np.ones(case.n))
    dropped = DroppedGraph(case.gt, 0.5, 9)
    with pytest.raises(L.EngineError, match="pgh_gnn.h"):
        dropped.conv(x)
    with pytest.raises(L.EngineError, match="pgh_gnn.h"):
        dropped.degrees()
    cfg = L.LoopCfg(alpha=0.85, use_quotient=0, err_kind=L.ERR_ITERS, tol=1e-6, max_iters=3, end_modulo=1, out_scale=1.0)
    out, res = DeviceVector.empty(case.n), L.LoopResult()
    assert L.lib().pgh_ppr_run_dropout(case.gt._h, x._h, out._h, C.byref(cfg), 0.5, 9, C.byref(res)) not in (0, L.DECLINED)
    assert b"pgh_gnn.h" in L.lib().pgh_last_error()
    assert np.all(np.isfinite(np.asarray(DroppedGraph(case.g, 0.5, 9).conv(x))))        # the partner still serves them


def test_batched_pagerank_dropout_honours_the_mirrored_words(pg, graph_cases):
    """pgh_ppr_run_batch_dropout on gt (step k under seed0 + k - 1) against numpy on the transposed masked matrices."""
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix
    case = graph_cases["multi"]
    rng = np.random.default_rng(5)
    X, seed0, K = _slab(rng, case.n, 5), 77, 6
    X /= np.maximum(X.sum(axis=0), 1e-300)
    X = X.astype(F32).astype(np.float64)
    cfg = L.LoopCfg(alpha=0.85, use_quotient=0, err_kind=L.ERR_ITERS, tol=1e-6, max_iters=K + 1, end_modulo=1, out_scale=1.0, start_from_p=1)
    P, R, results = DeviceMatrix.from_host(X), DeviceMatrix.empty(case.n, 5), (L.LoopResult * 5)()
    L.check(L.lib().pgh_ppr_run_batch_dropout(case.gt._h, P._h, R._h, C.byref(cfg), None, 0.3, seed0, results))
    want = X.copy()
    for k in range(K):
        want = 0.85 * (case.A(0.3, seed0 + k).T @ want) + 0.15 * X
    assert all(r.spmv_count == K for r in results)
    assert np.max(np.abs(np.asarray(R) - want)) <= 2e-6 * np.max(np.abs(want))


# ------------------------------------------------------------------------------------------------- 3. the loop
def _forward_np(case, kind, params, K, rate, seed0, X):
    if kind == "pagerank":
        x = X.copy()
        for k in range(K):
            x = params * (case.A(rate, seed0 + k) @ x) + (1 - params) * X
        return x
    term, out = X.copy(), params[0] * X
    for k in range(1, K + 1):
        term = case.A(rate, seed0 + k - 1) @ term
        out = out + params[k] * term
    return out


def _adjoint_np(case, kind, params, K, rate, seed0, W):
    """dL/dX for L = <F X, W>, by the chain rule through the forward recurrence with the explicit transpose of every step's matrix."""
    if kind == "pagerank":
        lam, total = W.copy(), np.zeros_like(W)
        for k in range(K, 0, -1):                                  # x_k = alpha A_k x_{k-1} + (1 - alpha) X
            total += (1 - params) * lam
            lam = params * (case.A(rate, seed0 + k - 1).T @ lam)
        return total + lam                                         # x_0 = X
    mu = params[K] * W
    for k in range(K, 0, -1):                                      # term_k = A_k term_{k-1}, out += c_k term_k
        mu = case.A(rate, seed0 + k - 1).T @ mu + params[k - 1] * W
    return mu


def _run_loop(case, g, plan, rate, X):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix
    s0, a, b, c, first, stride = plan
    arr = lambda q: (C.c_double * max(len(q), 1))(*q)
    V, out, ms = DeviceMatrix.from_host(X), DeviceMatrix.empty(*X.shape), C.c_double(-1.0)
    status = L.entry("pgh_linear_run_batch")(g._h, V._h, s0, len(a), arr(a), arr(b), arr(c), out._h, rate, first, stride, C.byref(ms))
    assert status == 0, L.lib().pgh_last_error()
    assert ms.value >= 0.0
    return np.asarray(out)


GENERIC = [1.0, 0.8, 0.0, 0.5, 0.0, 0.3, 0.25, 0.2, 0.1, 0.05, 0.02]       # c_0 .. c_10, with zeros


@pytest.mark.parametrize("b", WIDTHS[:3])
@pytest.mark.parametrize("name", ["multi", "weighted", "sym"])
def test_linear_loop_all_four_passes(pg, graph_cases, name, b):
    from pygrank_amd.gnn import linear_plan
    case = graph_cases[name]
    rng = np.random.default_rng(100 + b)
    X, seed0 = _slab(rng, case.n, b), 1000
    for K, rate in zip(STEPS + (6,), RATES + (0.0,)):
        for kind, params in (("pagerank", 0.9), ("taylor", GENERIC[:K + 1])):
            want = _forward_np(case, kind, params, K, rate, seed0, X)
            got = _run_loop(case, case.g, linear_plan(kind, params, K, seed0), rate, X)
            assert np.max(np.abs(got - want)) <= 2e-6 * np.max(np.abs(want)), (name, b, K, rate, kind, "forward")
            want = _adjoint_np(case, kind, params, K, rate, seed0, X)
            got = _run_loop(case, case.gt, linear_plan(kind, params, K, seed0, backward=True), rate, X)
            assert np.max(np.abs(got - want)) <= 2e-6 * np.max(np.abs(want)), (name, b, K, rate, kind, "backward")
            if b >= 3:
                assert not got[:, 1].any()                         # a zero column stays zero


def test_linear_loop_edges(pg, graph_cases):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix
    case = graph_cases["weighted"]
    rng = np.random.default_rng(9)
    X = _slab(rng, case.n, 5)
    # steps = 0: out = c[0] * s0 * v
    got = _run_loop(case, case.g, (0.5, [], [], [3.0], 5, 1), 0.5, X)
    assert np.max(np.abs(got - 1.5 * X)) <= 2 * EPS32 * np.max(X)
    # the recurrence as written, every coefficient different, the seeds descending
    a, b, c = [0.7, 1.1, 0.9], [0.2, 0.0, 0.4], [0.0, 2.0, 0.0, 0.5]
    s = 1.5 * X
    want = c[0] * s
    for k in range(1, 4):
        s = a[k - 1] * (case.A(0.3, 50 - (k - 1) * 2) @ s) + b[k - 1] * X
        want = want + c[k] * s
    got = _run_loop(case, case.g, (1.5, a, b, c, 50, -2), 0.3, X)
    assert np.max(np.abs(got - want)) <= 2e-6 * np.max(np.abs(want))
    # declined with nothing written: more than 64 columns; errors: a bad rate, aliasing
    entry, one = L.entry("pgh_linear_run_batch"), (C.c_double * 1)(1.0)
    wide, out = DeviceMatrix.from_host(np.ones((case.n, 70))), DeviceMatrix.from_host(np.full((case.n, 70), 7.0))
    assert entry(case.g._h, wide._h, 1.0, 0, None, None, one, out._h, 0.0, 0, 1, None) == L.DECLINED
    assert np.all(np.asarray(out) == 7.0)
    V = DeviceMatrix.from_host(X)
    assert entry(case.g._h, V._h, 1.0, 0, None, None, one, V._h, 0.0, 0, 1, None) not in (0, L.DECLINED)
    out5 = DeviceMatrix.empty(case.n, 5)
    assert entry(case.g._h, V._h, 1.0, 0, None, None, one, out5._h, 1.0, 0, 1, None) not in (0, L.DECLINED)


# ------------------------------------------------------------------------------------------------- 4. autograd
def _rankers(pg, pre):
    return dict(pagerank=(pg.PageRank(0.9, preprocessor=pre, use_quotient=False, error_type="iters", max_iters=10), "pagerank", 0.9, 9),
                generic=(pg.GenericGraphFilter(GENERIC[:10], preprocessor=pre, error_type="iters", max_iters=11), "taylor", GENERIC[:10], 9))


@pytest.mark.parametrize("which", ["pagerank", "generic"])
@pytest.mark.parametrize("name, b", [("multi", 3), ("sym", 20), ("weighted", 70)])
def test_autograd_under_graph_dropout(pg, graph_cases, name, b, which):
    import torch
    from pygrank_amd import gnn
    from pygrank_amd.backend import hip
    case = graph_cases[name]
    ranker, kind, params, K = _rankers(pg, case.pre)[which]
    rng = np.random.default_rng(17)
    Xn, Wn = _slab(rng, case.n, b), rng.random((case.n, b)).astype(F32).astype(np.float64)
    rate, start = 0.5, 4000
    chunks = [(s, min(s + 64, b)) for s in range(0, b, 64)]

    def run(fused):
        hip.set_dropout_seed(start)
        X = torch.tensor(Xn, dtype=torch.float32, requires_grad=True)
        Y = gnn.differentiable_propagate(ranker, case.graph, X, graph_dropout=rate, fused=fused)
        record = dict(gnn.last_call)
        after = hip.peek_dropout_seed()
        (Y * torch.tensor(Wn, dtype=torch.float32)).sum().backward(retain_graph=True)
        assert hip.peek_dropout_seed() == after                    # backward draws no seed
        return X, Y, record, after

    X, Y, record, after = run(True)
    assert record["fused"] is True and record["route"] == "host" and record["widths"] == [e - s for s, e in chunks]
    assert record["products"] == [K] * len(chunks) and record["seed0"][0] == start + 1 and len(record["seed0"]) == len(chunks)
    want_y, want_g = np.empty_like(Xn), np.empty_like(Xn)
    for (s, e), seed0 in zip(chunks, record["seed0"]):
        want_y[:, s:e] = _forward_np(case, kind, params, K, rate, seed0, Xn[:, s:e])
        want_g[:, s:e] = _adjoint_np(case, kind, params, K, rate, seed0, Wn[:, s:e])
    tol_y, tol_g = 2e-6 * np.max(np.abs(want_y)), 2e-6 * np.max(np.abs(want_g))
    assert np.max(np.abs(Y.detach().numpy() - want_y)) <= tol_y
    first = X.grad.numpy().copy()
    assert np.max(np.abs(first - want_g)) <= tol_g
    # backward once more: bit-identical, and still no seed
    X.grad = None
    (Y * torch.tensor(Wn, dtype=torch.float32)).sum().backward()
    assert np.array_equal(X.grad.numpy(), first) and hip.peek_dropout_seed() == after
    # the seed counter is where PageRank.propagate(graph_dropout=) leaves it (its reservation per chunk of 64 columns)
    probe = pg.PageRank(0.9, preprocessor=case.pre, use_quotient=False, error_type="iters", max_iters=int(ranker.convergence.max_iters))
    hip.set_dropout_seed(start)
    probe.propagate(case.graph, pg.to_primitive(Xn), graph_dropout=rate)
    assert hip.peek_dropout_seed() == after
    # one product at a time
    X2, Y2, record2, _ = run(False)
    assert record2["fused"] is False and record2["seed0"] == record["seed0"]
    assert np.max(np.abs(Y2.detach().numpy() - want_y)) <= tol_y and np.max(np.abs(X2.grad.numpy() - want_g)) <= tol_g
    # a second forward draws other seeds
    Y3 = gnn.differentiable_propagate(ranker, case.graph, torch.tensor(Xn, dtype=torch.float32), graph_dropout=rate)
    assert gnn.last_call["seed0"][0] == after and not np.array_equal(Y3.numpy(), Y.detach().numpy())


# ------------------------------------------------------------------------------------------------- 5. eval mode
def test_eval_mode_is_unchanged(pg, graph_cases):
    import torch
    from pygrank_amd import gnn
    rng = np.random.default_rng(2)
    for name in ("multi", "sym"):
        case = graph_cases[name]
        ranker = _rankers(pg, case.pre)["pagerank"][0]
        Xn, W = _slab(rng, case.n, 3), torch.tensor(rng.random((case.n, 3)), dtype=torch.float32)
        outs = []
        for kwargs in ({}, dict(graph_dropout=0)):
            X = torch.tensor(Xn, dtype=torch.float32, requires_grad=True)
            Y = gnn.differentiable_propagate(ranker, case.graph, X, **kwargs)
            (Y * W).sum().backward()
            outs.append((Y.detach().numpy().copy(), X.grad.numpy().copy()))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        want = _adjoint_np(case, "pagerank", 0.9, 9, 0, 0, W.numpy().astype(np.float64))
        assert np.max(np.abs(outs[0][1] - want)) <= 2e-6 * np.max(np.abs(want))
        operator = gnn.transposed_operator(ranker, case.graph)
        if name == "sym":
            assert operator is case.pre(case.graph)
        else:                                                      # built on the device, no scipy round trip
            assert operator is not case.pre(case.graph) and getattr(operator.array, "mask_mirrored", False)


# ------------------------------------------------------------------------------------------------- 6. device tensors
def test_device_tensors_are_not_staged():
    """In a process of its own (tests/gnn_device_worker.py), which imports torch BEFORE the engine library loads: torch's ROCm wheel
    brings its own HIP runtime, and only in that order does one runtime serve both -- the other way round torch sees no GPU.  The
    worker runs device_tensor_checks below for one and for two chunks."""
    import subprocess
    import sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gnn_device_worker.py")
    done = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "device tensors: ok [20, 70]" in done.stdout, done.stdout[-2000:] + done.stderr[-4000:]


def device_tensor_checks(pg, case, b):
    import torch
    from pygrank_amd import gnn
    from pygrank_amd.backend import hip
    assert torch.cuda.is_available()
    ranker = _rankers(pg, case.pre)["pagerank"][0]
    rng = np.random.default_rng(6)
    left = torch.tensor(rng.random((case.n, 8)), dtype=torch.float32, device="cuda")
    right = torch.tensor(rng.random((8, b)), dtype=torch.float32, device="cuda")
    W = torch.tensor(rng.random((case.n, b)), dtype=torch.float32, device="cuda")
    hip.set_dropout_seed(70)
    X = (left @ right).requires_grad_(True)                         # produced by a torch kernel immediately before the call
    Y = gnn.differentiable_propagate(ranker, case.graph, X, graph_dropout=0.5)
    assert Y.is_cuda and gnn.last_call["route"] == "device" and gnn.last_call["staged_bytes"] == 0 and gnn.last_call["fused"]
    (Y * W).sum().backward()
    assert X.grad.is_cuda and gnn.last_call["backward"] == dict(route="device", staged_bytes=0)
    # the host-tensor route with the same seed: the same bits
    hip.set_dropout_seed(70)
    Xh = X.detach().cpu().requires_grad_(True)
    Yh = gnn.differentiable_propagate(ranker, case.graph, Xh, graph_dropout=0.5)
    assert gnn.last_call["route"] == "host" and gnn.last_call["staged_bytes"] > 0
    (Yh * W.cpu()).sum().backward()
    assert torch.equal(Y.detach().cpu(), Yh.detach()) and torch.equal(X.grad.cpu(), Xh.grad)
    # f64 and non-contiguous tensors on the GPU take the host route and agree
    for other in (X.detach().double(), X.detach().t().contiguous().t()):
        assert other.dtype == torch.float64 or not other.is_contiguous()
        hip.set_dropout_seed(70)
        other = other.requires_grad_(True)
        Yo = gnn.differentiable_propagate(ranker, case.graph, other, graph_dropout=0.5)
        assert Yo.is_cuda and Yo.dtype == other.dtype and gnn.last_call["route"] == "host"
        (Yo * W.to(other.dtype)).sum().backward()
        assert float((Yo.detach().float() - Y.detach()).abs().max()) <= 2e-6 * float(Y.detach().abs().max())
        assert float((other.grad.float() - X.grad).abs().max()) <= 2e-6 * float(X.grad.abs().max())


# ------------------------------------------------------------------------------------------------- 7. a training step end to end
def planted_partition(seed=0, groups=3, size=60, p_in=0.15, p_out=0.01, noise=0.8):
    """(adjacency, noisy one-hot features [n, groups], labels), generated here: nothing is loaded."""
    rng = np.random.default_rng(seed)
    n = groups * size
    labels = np.repeat(np.arange(groups), size)
    prob = np.where(labels[:, None] == labels[None, :], p_in, p_out)
    upper = np.triu(rng.random((n, n)) < prob, 1)
    A = sp.csr_array((upper | upper.T).astype(np.float64))
    feats = np.eye(groups)[labels] + noise * rng.standard_normal((n, groups))
    return A, feats.astype(F32), labels


def initial_weights(seed=1, inputs=3, hidden=16, classes=3):
    rng = np.random.default_rng(seed)
    return [(0.5 * rng.standard_normal((inputs, hidden))).astype(F32), np.zeros(hidden, F32),
            (0.5 * rng.standard_normal((hidden, classes))).astype(F32), np.zeros(classes, F32)]


def mlp_loss(torch, params, feats, labels, propagate):
    hidden = torch.relu(feats @ params[0] + params[1])
    logits = propagate(hidden @ params[2] + params[3])
    return torch.nn.functional.cross_entropy(logits, labels), logits


def twin_propagate(torch, stored, rate, seed0, K, alpha, dtype):
    """PageRank's K masked steps on dense torch-CPU matrices built from the stored CSR(M^T) and the mask twin."""
    mats = [torch.tensor(mask_of(stored, rate, seed0 + k).toarray(), dtype=dtype) for k in range(K)]

    def propagate(z):
        x = z
        for A in mats:
            x = alpha * (A @ x) + (1 - alpha) * z
        return x
    return propagate


LR, TRAIN_SEED, TRAIN_STEPS = 0.5, 300, 30


def test_training_step_end_to_end(pg):
    """A two-layer MLP under differentiable_propagate(PageRank(0.9, 10 iterations), graph_dropout=0.5) and softmax cross-entropy on a
    planted partition of 3 x 60 nodes, against a torch-CPU f64 twin with the same initial weights that applies the explicit masked
    matrices of the recorded seeds.
    Fixed in advance: the first step's loss agrees within 1e-5 * max(1, max|Y|) (a 2e-6 relative error of the logits moves a log-softmax
    by at most twice that; margin 2.5); after 30 SGD steps the loss is finite and below the initial loss.
    LR and TRAIN_SEED were chosen on the twin alone (no GPU; the stored matrix rebuilt with numpy): see MEASURED below for its losses.
    The MLP weight gradients of the first step: the twin's own f32-against-f64 difference was measured (MEASURED), and four times it is
    allowed, since the two routes round independently."""
    import torch
    from pygrank_amd import gnn
    from pygrank_amd.backend import hip
    A, feats, labels = planted_partition()
    graph = pg.AdjacencyWrapper(A, directed=False)
    pre = pg.preprocessor(normalization="symmetric", assume_immutability=True)
    ranker = pg.PageRank(0.9, preprocessor=pre, use_quotient=False, error_type="iters", max_iters=10)
    stored = getattr(pre(graph), "array", pre(graph)).download_transposed()
    X, y = torch.tensor(feats), torch.tensor(labels, dtype=torch.long)
    params = [torch.tensor(w, requires_grad=True) for w in initial_weights()]
    twin = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in initial_weights()]
    hip.set_dropout_seed(TRAIN_SEED)
    losses = []
    for step in range(TRAIN_STEPS):
        loss, logits = mlp_loss(torch, params, X, y, lambda z: gnn.differentiable_propagate(ranker, graph, z, graph_dropout=0.5))
        loss.backward()
        if step == 0:
            seed0, K = gnn.last_call["seed0"][0], gnn.last_call["products"][0]
            assert (seed0, K) == (TRAIN_SEED + 1, 9)
            want, want_logits = mlp_loss(torch, twin, X.double(), y, twin_propagate(torch, stored, 0.5, seed0, K, 0.9, torch.float64))
            want.backward()
            print("first loss", float(loss.detach()), "twin", float(want.detach()))
            assert abs(float(loss.detach()) - float(want.detach())) <= 1e-5 * max(1.0, float(want_logits.detach().abs().max()))
            for got, ref in zip(params, twin):
                diff = float((got.grad.double() - ref.grad).abs().max()) / float(ref.grad.abs().max())
                print("weight gradient: relative difference", diff)
                assert diff <= 4 * MEASURED["twin_f32_vs_f64_weight_grad"]
        with torch.no_grad():
            for w in params:
                w -= LR * w.grad
                w.grad = None
        losses.append(float(loss.detach()))
    print("losses", losses[0], losses[-1])
    assert np.isfinite(losses[-1]) and losses[-1] < losses[0]


# measured with the twin alone on a CPU (tests/test_gpu_gnn.py twin_alone()): its losses over TRAIN_STEPS steps, and the largest relative
# difference max|grad32 - grad64| / max|grad64| over the four weight tensors between the twin run in f32 and in f64 at the first step
MEASURED = dict(twin_first_loss=1.3772474, twin_last_loss=0.2773268, twin_f32_vs_f64_weight_grad=2.81e-7)


def twin_alone(steps=TRAIN_STEPS):
    """The twin without a GPU: the stored matrix is rebuilt with numpy (symmetric normalisation, f32 values in canonical CSR order)."""
    import torch
    A, feats, labels = planted_partition()
    deg = np.asarray(A.sum(axis=1)).ravel()
    scale = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1e-300)), 0.0)
    M = sp.csr_array(sp.diags(scale) @ A @ sp.diags(scale))
    stored = sp.csr_array(M.T.tocsr())
    stored.sort_indices()
    stored = sp.csr_array((stored.data.astype(F32), stored.indices, stored.indptr), shape=stored.shape)
    y = torch.tensor(labels, dtype=torch.long)
    grads = {}
    for dtype in (torch.float32, torch.float64):
        params = [torch.tensor(w, dtype=dtype, requires_grad=True) for w in initial_weights()]
        loss, _ = mlp_loss(torch, params, torch.tensor(feats, dtype=dtype), y, twin_propagate(torch, stored, 0.5, TRAIN_SEED + 1, 9, 0.9, dtype))
        loss.backward()
        grads[dtype] = [w.grad.double() for w in params]
    rel = max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(grads[torch.float32], grads[torch.float64]))
    params = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in initial_weights()]
    losses, seed = [], TRAIN_SEED
    for _ in range(steps):
        seed0, seed = seed + 1, seed + 10                           # PageRank.propagate reserves max_iters seeds per chunk
        loss, _ = mlp_loss(torch, params, torch.tensor(feats, dtype=torch.float64), y, twin_propagate(torch, stored, 0.5, seed0, 9, 0.9, torch.float64))
        loss.backward()
        with torch.no_grad():
            for w in params:
                w -= LR * w.grad
                w.grad = None
        losses.append(float(loss.detach()))
    return losses, rel
