"""Differentiable ``propagate`` for APPNP-style use (pygrank tests/test_gnn.py:22-28: a ranker's ``propagate`` inside a
model's forward pass, ``graph_dropout=0.5 if training else 0``; the reference gets its gradients from running the filter on a tensorflow
/ pytorch backend).

This backend's loops are not an autograd tape, but the filters a GNN propagates with are LINEAR maps of the feature matrix -- a fixed number
of steps (``error_type="iters"``), no L1 quotient: Y = F X with F = sum_k c_k (M^T)^k -- so the gradient of a loss with respect to the
features is the SAME filter run on the transposed operator: dL/dX = F^T dL/dY, F^T = sum_k c_k M^k.  ``differentiable_propagate`` is a
``torch.autograd.Function`` whose backward pass is one more run on the transposed graph.

Eval mode (``graph_dropout == 0``): forward and backward are ``ranker.propagate`` (pgh_ppr_run_batch for PageRank, pgh_poly_run_batch
for the taylor form of the closed-form filters, include/pgh_batch.h), the backward on the transposed operator -- the same graph when the
normalised matrix is symmetric, otherwise built once per graph on the device (include/pgh_gnn.h pgh_graph_transposed).

Training mode (``0 < graph_dropout < 1``): step k multiplies by the matrix masked with seed0 + k - 1, so F = sum_k c_k A_k ... A_1 and
F^T = sum_k c_k A_1^T ... A_k^T: the masks are replayed in reverse order on the transposed graph, whose multi-seed image applies, for
every seed, the transpose of the masked matrix its partner applies (include/pgh_gnn.h).  A symmetric M needs that graph too: the mask is
not symmetric.  The forward reserves its seeds as ``PageRank.propagate(..., graph_dropout=)`` does (one reservation per chunk of 64
columns) and remembers (seed0, products) per chunk; the backward draws none and may be repeated.  Both passes are ONE resident loop per
chunk (pgh_linear_run_batch, ``linear_plan`` gives its coefficients); ``fused=False`` and a library without that loop step the same
recurrence one masked product at a time.  A contiguous f32 tensor on the GPU goes in and out as a view (pgh_mat_wrap): no byte is staged
through the host.  (torch's ROCm wheels bring their own HIP runtime: ``import torch`` before the engine library loads, so that one
runtime serves both -- loaded the other way round, torch sees no GPU and its tensors are CPU tensors, which take the host route.)
Memory: the transposed graph is a second set of images plus 4 bytes per stream entry of index words.

``last_call`` describes the latest forward (and, under "backward", the latest backward): route ("device": views of the tensors' memory,
"host": slabs staged through numpy), fused, the chunks' widths, seed0 and products per chunk, staged_bytes."""
import ctypes as C

import numpy as np

from pygrank_amd import _lib as L
from pygrank_amd import backend
from pygrank_amd.device import DeviceGraph, DeviceMatrix, DroppedGraph
from pygrank_amd.preprocessing import Adjacency

last_call = {}


def _is_linear(ranker):
    """A fixed number of steps and no L1 quotient (RecursiveGraphFilter.use_quotient, abstract_filters.py:133-134): then rank() is linear in
    the personalization -- the L1 normalisation of GraphFilter.rank (:52-55) and preserve_norm (:63-64) cancel."""
    counts_only = getattr(ranker.convergence, "_counts_only", lambda: False)()
    quotient = getattr(ranker, "use_quotient", False)
    return counts_only and (quotient is False or quotient == 0) and getattr(ranker, "preserve_norm", True) \
        and not getattr(ranker, "converge_to_eigenvectors", False)


def _device_graph_of(M):
    g = getattr(M, "array", M)
    if not isinstance(g, DeviceGraph):
        raise Exception("differentiable_propagate needs a graph of the hip backend")
    return g


def mirrored_graph(ranker, graph):
    """The transposed DeviceGraph with the preprocessed graph as its mask partner (cached on the preprocessed graph), or None where the
    library has no pgh_graph_transposed or declines the graph."""
    M = ranker.preprocessor(graph)
    cached = getattr(M, "_pgh_mirrored", None)
    if cached is None:
        cached = _device_graph_of(M).transposed()
        if cached is not None:
            M._pgh_mirrored = cached
    return cached


def transposed_operator(ranker, graph):
    """The preprocessed graph whose conv multiplies by M instead of M^T (cached on the preprocessed graph); the graph itself when M = M^T."""
    M = ranker.preprocessor(graph)
    cached = getattr(M, "_pgh_transposed", None)
    if cached is not None:
        return cached
    g = _device_graph_of(M)
    MT = g.download_transposed()                              # scipy CSR of the stored M^T (f32 values)
    diff = MT - MT.T
    if diff.nnz == 0 or abs(diff).max() == 0:
        out = M
    else:
        gt = mirrored_graph(ranker, graph)                    # built in HBM; the scipy round trip where the library cannot
        out = Adjacency(gt if gt is not None else DeviceGraph.from_scipy(MT))     # stores (M^T)^T = M: its conv is x -> M x
        out._pygrank_preprocessed = {backend.backend_name(): out}
        out._pygrank_node2id = M._pygrank_node2id
        out.is_directed = getattr(M, "is_directed", lambda: True)
    M._pgh_transposed = out
    return out


def _run(ranker, graph, array):
    F = DeviceMatrix.from_host(np.ascontiguousarray(array, dtype=np.float64))
    out = ranker.propagate(graph, F)
    if not isinstance(out, DeviceMatrix):                     # the per-column fallback of NodeRanking.propagate
        out = backend.combine_cols([getattr(col, "np", col) for col in out])
    return np.asarray(out, dtype=np.float64)


# ------------------------------------------------------------------------------------------------- the linear recurrences
def linear_plan(kind, params, products, seed0=0, backward=False):
    """(s0, a, b, c, seed_first, stride) of include/pgh_gnn.h pgh_linear_run_batch:
        s_0 = s0 v, acc = c[0] s_0;   s_k = a[k-1] A_k s_{k-1} + b[k-1] v, acc += c[k] s_k  (k = 1 .. K);   out = acc,
    A_k = the operator under the mask of seed_first + (k - 1) stride (the transposed operator in a backward pass).
    kind "pagerank" (params = alpha): K = `products` steps x <- alpha A x + (1 - alpha) v from x = v, masks seed0 .. seed0 + K - 1.
    kind "taylor" (params = c_0 .. c_K): sum_k c_k A_k ... A_1 v.
    backward: the adjoint map, for the transposed operators, masks in descending order:
      pagerank   F^T g = alpha^K B_K..B_1 g + (1 - alpha) sum_{j<K} alpha^j B_j..B_1 g,  B_k = A_{K-k+1}^T: plain powers, c collects them;
      taylor     F^T g = c_0 g + A_1^T (c_1 g + A_2^T (... + A_K^T c_K g)): Horner, from the innermost term outwards."""
    K = int(products)
    if K < 0:
        raise Exception("linear_plan: a negative number of products")
    ones, zeros = [1.0] * K, [0.0] * K
    unit = [0.0] * K + [1.0]
    first, stride = (int(seed0) + K - 1, -1) if backward else (int(seed0), 1)
    if kind == "pagerank":
        alpha = float(params)
        if not backward:
            return 1.0, [alpha] * K, [1.0 - alpha] * K, unit, first, stride
        return 1.0, ones, zeros, [(1.0 - alpha) * alpha ** j for j in range(K)] + [alpha ** K], first, stride
    if kind == "taylor":
        c = [float(v) for v in params]
        if len(c) != K + 1:
            raise Exception("linear_plan: the taylor form needs products + 1 coefficients")
        if not backward:
            return 1.0, ones, zeros, c, first, stride
        return c[K], ones, [c[K - k] for k in range(1, K + 1)], unit, first, stride
    raise Exception("linear_plan: unknown kind " + str(kind))


def run_plan(apply, v, plan):
    """The recurrence of `plan` on any array type with * and +; apply(seed, s) -> A s under the mask of `seed`."""
    s0, a, b, c, first, stride = plan
    s = v * s0
    acc = s * c[0]
    for k in range(1, len(a) + 1):
        s = apply(first + (k - 1) * stride, s) * a[k - 1] + v * b[k - 1]
        acc = acc + s * c[k]
    return acc


def _filter_of(ranker):
    """(kind, params, products, seeds one chunk reserves) of a ranker this module runs under graph_dropout: PageRank and the taylor form of
    the closed-form filters, on the ranker's own class with its own hooks -- the configurations their propagate runs as one device loop."""
    from pygrank_amd import filters as F
    from pygrank_amd.postprocess import Tautology
    transform = getattr(ranker, "personalization_transform", None)
    plain = isinstance(ranker, F.GraphFilter) and isinstance(transform, Tautology) and transform.ranker is None \
        and type(ranker)._prepare_graph is F.GraphFilter._prepare_graph and ranker.dtype != "float64"
    iters = int(ranker.convergence.max_iters)
    if plain and isinstance(ranker, F.PageRank) and type(ranker)._formula is F.PageRank._formula \
            and type(ranker)._step is F.RecursiveGraphFilter._step and type(ranker)._start is F.PageRank._start:
        return "pagerank", float(ranker.alpha), max(iters - 1, 0), max(iters, 1)
    own = F.ClosedFormGraphFilter
    if plain and isinstance(ranker, own) and ranker.coefficient_type == "taylor" and ranker.optimization_dict is None \
            and ranker.krylov_dims is None and all(getattr(type(ranker), hook) is getattr(own, hook)
                                                   for hook in ("_step", "_recursion", "_start", "_retrieve_power", "_prepare")):
        coeffs = ranker._coefficient_schedule(max(iters - 1, 0))
        if coeffs:
            return "taylor", coeffs, len(coeffs) - 1, max(iters, 1)
    raise Exception("differentiable_propagate: graph_dropout is served for PageRank and the taylor form of the closed-form filters, on "
                    "the ranker's own class with its own hooks")


def _loop(g, rate, fused):
    """The function (v: DeviceMatrix, out: DeviceMatrix or None, plan) -> DeviceMatrix that runs a plan on the DeviceGraph `g`."""
    entry = L.entry("pgh_linear_run_batch") if fused else None

    def stepwise(v, out, plan):
        # slab arithmetic in numpy f32, one masked multi-seed product per step
        def apply(seed, s):
            slab = DeviceMatrix.from_host(s)
            graph = DroppedGraph(g, rate, int(seed) & 0xFFFFFFFFFFFFFFFF) if rate else g
            return np.asarray(graph.conv(slab)).astype(np.float32)
        return DeviceMatrix.from_host(run_plan(apply, np.asarray(v).astype(np.float32), plan))     # (f32 array * Python float stays f32)

    def resident(v, out, plan):
        s0, a, b, c, first, stride = plan
        K = len(a)
        out = DeviceMatrix.empty(v.n, v.b) if out is None else out
        arr = lambda q: (C.c_double * max(len(q), 1))(*q)
        status = entry(g._h, v._h, float(s0), K, arr(a), arr(b), arr(c), out._h, float(rate), int(first) & 0xFFFFFFFFFFFFFFFF, int(stride), None)
        if not L.accepted(status):
            return stepwise(v, None, plan)
        return out
    return resident if entry is not None else stepwise


def _on_device(x):
    import torch
    return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2 and L.entry("pgh_mat_wrap") is not None


def _apply_chunks(g, rate, fused, x, plans, record):
    """x [n, B] torch tensor -> the plans' maps of its column chunks (plans[i] for chunk i of 64 columns), as a tensor like x."""
    import torch
    run = _loop(g, rate, fused)
    resident = fused and L.entry("pgh_linear_run_batch") is not None
    n, B = x.shape
    bounds = [(s, min(s + 64, B)) for s in range(0, B, 64)]
    if resident and _on_device(x):
        # views of torch's memory; whatever torch has queued on its stream is finished first, the engine finishes its own loop itself
        torch.cuda.current_stream(x.device).synchronize()
        y = torch.empty_like(x)
        for (s, e), plan in zip(bounds, plans):
            xin = x if len(bounds) == 1 else x[:, s:e].contiguous()
            yout = y if len(bounds) == 1 else torch.empty_like(xin)
            if len(bounds) > 1:
                torch.cuda.current_stream(x.device).synchronize()
            view = DeviceMatrix.wrap(yout.data_ptr(), n, e - s, yout)
            out = run(DeviceMatrix.wrap(xin.data_ptr(), n, e - s, xin), view, plan)
            if out is not view:                                                    # the loop declined: its stepwise outcome, staged
                yout.copy_(torch.as_tensor(np.asarray(out), dtype=x.dtype))
                record["staged_bytes"] += 8 * n * (e - s)
            if yout is not y:
                y[:, s:e] = yout
        record["route"] = "device"
        return y
    host = x.detach().cpu().numpy()
    out = np.empty(host.shape, dtype=np.float64)
    for (s, e), plan in zip(bounds, plans):
        out[:, s:e] = np.asarray(run(DeviceMatrix.from_host(np.ascontiguousarray(host[:, s:e], dtype=np.float64)), None, plan))
    record["route"] = "host"
    record["staged_bytes"] += 2 * host.shape[0] * host.shape[1] * x.element_size()
    return torch.as_tensor(out, dtype=x.dtype, device=x.device)


def differentiable_propagate(ranker, graph, features, graph_dropout=0, fused=True):
    """ranker.propagate(graph, features, graph_dropout=graph_dropout) as a differentiable torch operation.  features: torch tensor [n, B]
    (any device / float dtype); returns a tensor of the same device and dtype.  The ranker must be linear in its personalization:
    error_type="iters", use_quotient=False (what the reference's APPNP example configures, tests/test_gnn.py:24-25).
    graph_dropout in (0, 1): training mode (module docstring); fused=False steps the recurrences one masked product at a time."""
    import torch
    if not _is_linear(ranker):
        raise Exception("differentiable_propagate: the ranker must run a fixed number of steps without the L1 quotient "
                        "(error_type='iters', use_quotient=False): only then is propagate a linear map with a transposed-operator gradient")
    rate = float(graph_dropout or 0)
    if not 0 <= rate < 1:
        raise Exception("differentiable_propagate: graph_dropout must lie in [0, 1)")
    widths = [min(64, features.shape[1] - s) for s in range(0, features.shape[1], 64)] if features.dim() == 2 else []

    if rate == 0:
        class _Propagate(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x):
                y = _run(ranker, graph, x.detach().cpu().numpy())
                last_call.clear()
                last_call.update(route="host", fused=bool(fused), widths=widths, seed0=[], products=[],
                                 staged_bytes=2 * x.numel() * x.element_size())
                return torch.as_tensor(y, dtype=x.dtype, device=x.device)

            @staticmethod
            def backward(ctx, grad_out):
                gx = _run(ranker, transposed_operator(ranker, graph), grad_out.detach().cpu().numpy())
                last_call["backward"] = dict(route="host", staged_bytes=2 * grad_out.numel() * grad_out.element_size())
                return torch.as_tensor(gx, dtype=grad_out.dtype, device=grad_out.device)

        return _Propagate.apply(features)

    from pygrank_amd.backend import hip as _hip
    if L.entry("pgh_graph_transposed") is None:
        raise Exception("differentiable_propagate: graph_dropout needs the transposed graph with a mirrored mask, which this engine "
                        "library does not export (include/pgh_gnn.h: pgh_graph_transposed)")
    kind, params, products, reserve = _filter_of(ranker)
    g = _device_graph_of(ranker.preprocessor(graph))
    if features.dim() != 2 or g.shape[0] != g.shape[1] or features.shape[0] != g.shape[0]:
        raise Exception("differentiable_propagate: features must be [n, B] on a square graph of n nodes")

    class _Dropped(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            seeds = [_hip.take_dropout_seeds(reserve) for _ in widths]             # as PageRank.propagate: one reservation per chunk
            ctx.seeds = seeds
            record = dict(route=None, fused=bool(fused) and L.entry("pgh_linear_run_batch") is not None, widths=widths, seed0=seeds,
                          products=[products] * len(widths), staged_bytes=0)
            y = _apply_chunks(g, rate, fused, x.detach(), [linear_plan(kind, params, products, s) for s in seeds], record)
            last_call.clear()
            last_call.update(record)
            return y

        @staticmethod
        def backward(ctx, grad_out):
            gt = mirrored_graph(ranker, graph)
            if gt is None:
                raise Exception("differentiable_propagate: the engine declined to transpose this graph (include/pgh_gnn.h)")
            record = dict(route=None, staged_bytes=0)
            grad = grad_out.detach()
            if grad.is_cuda and not grad.is_contiguous():
                grad = grad.contiguous()
            gx = _apply_chunks(gt, rate, fused, grad, [linear_plan(kind, params, products, s, backward=True) for s in ctx.seeds], record)
            last_call["backward"] = record
            return gx

    return _Dropped.apply(features)
