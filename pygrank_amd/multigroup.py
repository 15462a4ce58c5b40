"""Measures of a SET of communities at once: restates pygrank/measures/multigroup.py (LinkAssessment :30-107, i.e. LinkAUC / HopAUC,
ClusteringCoefficient :110-146, MultiUnsupervised :149-158, MultiSupervised :161-170) on the [n, b] slab a multi-seed ``propagate``
returns, one column per group.

Scores are given as a dict ``{group: GraphSignal | dict | vector}`` (a node a dict does not name counts as 0, as ``.get(u, 0)`` does),
as a list of such columns, or as a ``DeviceMatrix``.  The column order is the group order; the last column is the "last group".

THE SIMILARITY KEEPS THE REFERENCE'S QUIRK.  ``_dot_similarity`` and ``_cos_similarity`` (multigroup.py:8-27) assign ``dot = ui * vi``
inside their loop over the groups instead of accumulating it: the numerator of a pair is the product of the LAST group's two scores
alone.  The cos denominator is ``sqrt(l2u * l2v)`` with l2 the row's sum of squares over all groups, added in column order, and a zero
denominator gives 0.  It is kept as it stands (as krylov.py keeps H's), so that values stay comparable with the reference's.

Departures from the reference, all documented here:
  * the sample comes from a PRIVATE ``numpy.random.RandomState(seed)`` -- the reference reseeds numpy's global generator on every
    evaluation; the draws are the same (``choice(n, k)`` for the candidates when n > max_positive_samples, then one
    ``choice(n, min(max_negative_samples, n))`` per candidate, with replacement: duplicates stay and count).  ``seed=None`` draws from
    numpy's global functions;
  * the sample and the pair list are built ONCE per instance (they depend on the graph and the seed alone) and kept as a plan: a
    tuner's repeated evaluations cost the device passes only;
  * for hops >= 3 the reference's stack walk labels nodes by a set's iteration order and can miss nodes of the ball; here the positives
    of a candidate are the true BFS ball of `hops` steps (for hops 1 and 2 the reference's walk IS that ball);
  * ``nodes=`` is accepted and ignored: the reference stores it and never reads it;
  * a graph's structure is the non-zero pattern of its adjacency matrix (``G.neighbors``: successors on a directed graph, weights
    ignored); a bare scipy matrix is taken as directed unless its pattern is symmetric.

With the entries of include/pgh_link.h the slab never leaves the device: a row pass, a pair pass, one radix sort
and an integer count give the AUC.  ``fused=False``, a library without the entries and a declined call all run the same restatement in
numpy on the downloaded slab; ``last_route`` says which ("device" or "host").
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from pygrank_amd import _lib as L
from pygrank_amd import backend
from pygrank_amd.device import DeviceGraph, DeviceMatrix, DeviceVector, EnginePlan
from pygrank_amd.measures import AUC
from pygrank_amd.preprocessing import AdjacencyWrapper, graph_to_scipy
from pygrank_amd.signals import GraphSignal, to_signal

_SIMILARITIES = {"cos": L.LINK_COS, "dot": L.LINK_DOT}
_SAME_CLASS = "Cannot evaluate AUC when all labels are the same"


def _as_graph(graph):
    """A bare matrix becomes a graph over the nodes 0 .. n - 1; directed unless its pattern is symmetric."""
    if sp.issparse(graph) or isinstance(graph, np.ndarray):
        M = sp.csr_array(graph)
        P = _pattern_of(M)
        return AdjacencyWrapper(M, directed=(P != P.T).nnz != 0)
    return graph


def _pattern_of(M):
    """The 0/1 pattern of a matrix as CSR with int64 ones and sorted indices (explicit zeros are no edges)."""
    M = sp.csr_array(M).copy()
    M.sum_duplicates()
    M.eliminate_zeros()
    M.sort_indices()
    return sp.csr_array((np.ones(M.nnz, dtype=np.int64), M.indices, M.indptr), shape=M.shape)


def pattern(graph):
    """(graph, P): what `graph` is taken as (_as_graph) and the 0/1 pattern of its adjacency matrix, rows = successors."""
    graph = _as_graph(graph)
    return graph, _pattern_of(graph_to_scipy(graph))


def sample(n, max_positive_samples, seed):
    """(candidates, generator): the reference's candidate draw -- every node once, in order, and no draw when n <= max_positive_samples;
    else ``choice(n, max_positive_samples)`` -- and the generator that made it, from which the negatives follow."""
    generator = np.random if seed is None else np.random.RandomState(seed)
    if n > max_positive_samples:
        return np.asarray(generator.choice(n, max_positive_samples), dtype=np.int64), generator
    return np.arange(n, dtype=np.int64), generator


def slab_of(graph, scores):
    """The [n, b] DeviceMatrix of the groups' scores, columns in the groups' order."""
    n = len(graph)
    if isinstance(scores, DeviceMatrix):
        if scores.n != n:
            raise Exception(f"a slab of {scores.n} rows cannot hold scores of {n} nodes")
        return scores
    columns = list(scores.values()) if hasattr(scores, "values") and not isinstance(scores, GraphSignal) else list(scores)
    if not columns:
        raise Exception("the scores of at least one group are needed")
    vectors = []
    for column in columns:
        if isinstance(column, GraphSignal) and len(column.np) == n:
            vector = column.np
        elif isinstance(column, DeviceVector):
            vector = column
        else:
            vector = to_signal(graph, column).np
        if len(vector) != n:
            raise Exception(f"a column of {len(vector)} scores cannot go with a graph of {n} nodes")
        vector._h                           # noqa: B018 -- an unevaluated expression (device.LazyVector) is evaluated first
        vectors.append(vector)
    return DeviceMatrix.from_columns(vectors)


def host_row_squares(S):
    """l2[i] = sum_j S[i, j]^2 added in column order: the order is the reference's (and the device row pass's)."""
    l2 = np.zeros(S.shape[0], dtype=np.float64)
    for j in range(S.shape[1]):
        l2 += S[:, j] * S[:, j]
    return l2


def host_predictions(S, first, second, similarity):
    """The similarity of every pair (first[k], second[k]) under the f64 slab S, as Python computes it pair by pair."""
    last = S[:, -1]
    with np.errstate(all="ignore"):
        predicted = last[second] * last[first]
        if similarity == "cos":
            l2 = host_row_squares(S)
            denominator = np.sqrt(l2[second] * l2[first])
            zero = denominator == 0
            predicted = np.where(zero, 0.0, predicted / np.where(zero, 1.0, denominator))
    return predicted


def host_factors(S, similarity):
    """t with similarity(v, u) = t_v t_u up to rounding: the last column, for "cos" over the root of the row's sum of squares."""
    last = S[:, -1]
    if similarity == "dot":
        return last.copy()
    with np.errstate(all="ignore"):
        denominator = np.sqrt(host_row_squares(S))
        zero = denominator == 0
        return np.where(zero, 0.0, last / np.where(zero, 1.0, denominator))


def host_auc(predicted, labels):
    """(auc, P, N) with ties at their mid-rank, counted in integers: two_wins / (2.0 * P * N), one rounding."""
    labels = np.asarray(labels) != 0
    P = int(labels.sum())
    N = len(labels) - P
    if P == 0 or N == 0:
        return float("nan"), P, N
    predicted = np.asarray(predicted, dtype=np.float64) + 0.0        # -0.0 and +0.0 are one score
    if np.isnan(predicted).any():
        return float("nan"), P, N
    order = np.argsort(predicted, kind="stable")
    ordered, negative = predicted[order], ~labels[order]
    before = np.concatenate(([0], np.cumsum(negative, dtype=np.int64)))
    at = np.flatnonzero(~negative)
    begin = np.searchsorted(ordered, ordered[at], side="left")
    end = np.searchsorted(ordered, ordered[at], side="right")
    two_wins = int(np.sum(2 * before[begin] + (before[end] - before[begin]), dtype=np.int64))
    return two_wins / (2.0 * P * N), P, N


class _LinkPlan(EnginePlan):
    """The pairs of one (graph, hops, samples, seed): ids and labels on the host, and -- once a fused evaluation asked for it -- on the
    device (pgh_link_plan_create)."""
    _DESTROY = "pgh_link_plan_destroy"

    def __init__(self, n, candidates, first, second, label):
        self.n = int(n)
        self.candidates = candidates
        self.first = np.ascontiguousarray(first, dtype=np.int32)
        self.second = np.ascontiguousarray(second, dtype=np.int32)
        self.label = np.ascontiguousarray(label, dtype=np.uint8)
        self.num_pairs = len(self.label)
        self.num_positive = int(self.label.sum())
        self._h = None

    def handle(self):
        if self._h is None:
            if self.num_pairs > L.LINK_MAX_PAIRS:
                raise Exception(f"{self.num_pairs} pairs exceed the {L.LINK_MAX_PAIRS} a plan holds: "
                                "take smaller max_positive_samples / max_negative_samples")
            L.ensure_init()
            handle = L.c_link_plan()
            L.check(L.entry("pgh_link_plan_create")(
                self.n, self.num_pairs, self.first.ctypes.data_as(L.c_i32p), self.second.ctypes.data_as(L.c_i32p),
                self.label.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(handle)))
            self._h = handle
        return self._h


def _identity(x):
    return x


class LinkAssessment:
    """multigroup.py:30-107.  For every sampled candidate v: a positive pair (v, u) for every other node u of v's `hops`-ball, a
    negative pair for every negative draw outside the ball; the value is ``measure(labels)(similarities)``, by default the AUC.
    hops=1 is LinkAUC, hops=2 HopAUC.  See the module's text for the similarity's quirk and the departures from the reference."""

    def __init__(self, graph, nodes=None, measure=AUC, similarity="cos", hops=1, max_positive_samples=2000, max_negative_samples=2000,
                 seed=0, progress=_identity, fused=True):
        if similarity not in _SIMILARITIES:
            raise Exception(f"similarity {similarity!r}: expected cos or dot")
        self.G = _as_graph(graph)
        self.nodes = nodes                                   # stored and never read, as in the reference
        self.measure = measure
        self.similarity = similarity
        self.hops = hops
        self.max_positive_samples = max_positive_samples
        self.max_negative_samples = max_negative_samples
        self.seed = seed
        self.fused = fused
        self.last_route = None
        self.plans_built = 0
        self._progress = progress
        self._plan = None
        if self.G.is_directed():
            import warnings
            warnings.warn("LinkAssessment is designed for undirected graphs", stacklevel=2)

    def plan(self):
        """The sample and its pairs, built on first use with numpy on the CSR pattern and kept."""
        if self._plan is not None and self.seed is not None:
            return self._plan
        _, P = pattern(self.G)
        n = P.shape[0]
        indptr, indices = P.indptr, P.indices
        candidates, generator = sample(n, self.max_positive_samples, self.seed)
        draws = min(self.max_negative_samples, n)
        first, second, label = [], [], []
        for v in self._progress(candidates):
            v = int(v)
            ball = np.array([v], dtype=np.int64)
            frontier = ball
            for _ in range(int(self.hops)):
                if len(frontier) == 0:
                    break
                reached = np.unique(np.concatenate([indices[indptr[u]:indptr[u + 1]] for u in frontier] + [ball[:0]]))
                frontier = np.setdiff1d(reached, ball, assume_unique=True)
                ball = np.union1d(ball, frontier)
            positives = ball[ball != v]
            negatives = np.asarray(generator.choice(n, draws), dtype=np.int64) if n > 0 else ball[:0]
            negatives = negatives[~np.isin(negatives, ball)]
            second.append(positives)
            second.append(negatives)
            label.append(np.ones(len(positives), dtype=np.uint8))
            label.append(np.zeros(len(negatives), dtype=np.uint8))
            first.append(np.full(len(positives) + len(negatives), v, dtype=np.int64))
        empty = np.zeros(0, dtype=np.int64)
        self._plan = _LinkPlan(n, candidates, np.concatenate(first + [empty]), np.concatenate(second + [empty]),
                               np.concatenate(label + [empty.astype(np.uint8)]))
        self.plans_built += 1
        return self._plan

    def _device_available(self):
        return self.fused and all(L.entry(name) is not None for name in L.LINK_SIGNATURES)

    def predictions(self, scores):
        """(similarities, labels) of the plan's pairs as f64 / uint8 host arrays."""
        plan = self.plan()
        matrix = slab_of(self.G, scores)
        if self._device_available() and plan.num_pairs <= L.LINK_MAX_PAIRS:
            out = np.empty(plan.num_pairs, dtype=np.float64)
            status = L.entry("pgh_link_predictions")(matrix._h, plan.handle(), _SIMILARITIES[self.similarity], 0, plan.num_pairs,
                                                     out.ctypes.data_as(L.c_f64p))
            if L.accepted(status):
                self.last_route = "device"
                return out, plan.label
        self.last_route = "host"
        return host_predictions(matrix.numpy(), plan.first, plan.second, self.similarity), plan.label

    def _auc(self, scores):
        plan = self.plan()
        if plan.num_positive == 0 or plan.num_positive == plan.num_pairs:
            raise Exception(_SAME_CLASS)
        matrix = slab_of(self.G, scores)
        value = None
        if self._device_available():
            auc, positive, negative = C.c_double(), C.c_int64(), C.c_int64()
            status = L.entry("pgh_link_auc")(matrix._h, plan.handle(), _SIMILARITIES[self.similarity], C.byref(auc), C.byref(positive),
                                             C.byref(negative))
            if L.accepted(status):
                self.last_route = "device"
                value = auc.value
        if value is None:
            self.last_route = "host"
            value, _, _ = host_auc(host_predictions(matrix.numpy(), plan.first, plan.second, self.similarity), plan.label)
        if value != value:
            raise ValueError("Input contains NaN")           # what sklearn says to the reference for non-finite scores
        return value

    def evaluate(self, scores):
        if self.measure is AUC:
            return self._auc(scores)
        predicted, real = self.predictions(scores)
        return self.measure([float(x) for x in real])([float(x) for x in predicted])

    def __call__(self, scores):
        return self.evaluate(scores)


class ClusteringCoefficient:
    """multigroup.py:110-146 (doi of the weighted coefficient: Opsahl et al. 2009).  Over the sampled nodes v, with multiplicity c_v:
        numerator   = sum_v c_v sum_{u1, u2 in N(v)} similarity(u1, u2) = sum_v c_v ((P t)_v)^2      (the u1 = u2 terms included)
        denominator = sum_v c_v sum_{u in N(v)} |N(v) & N(u)|
    with t the similarity's per-row factor (pgh_link_factors).  The closed form replaces the reference's triple loop; its denominator
    depends on the graph and the sample alone and is computed once, on the host.  0 when the denominator is 0.  The numerator is one
    ``conv`` on the 0/1 pattern; fused=False (or a library without include/pgh_link.h) evaluates it with numpy on the downloaded slab."""

    def __init__(self, G, similarity="cos", max_positive_samples=2000, seed=1, fused=True):
        if similarity not in _SIMILARITIES:
            raise Exception(f"similarity {similarity!r}: expected cos or dot")
        self.G = _as_graph(G)
        self.similarity = similarity
        self.max_positive_samples = max_positive_samples
        self.seed = seed
        self.fused = fused
        self.last_route = None
        self._prepared = None
        if self.G.is_directed():
            import warnings
            warnings.warn("ClusteringCoefficient is designed for undirected graphs", stacklevel=2)

    def _prepare(self):
        if self._prepared is not None and self.seed is not None:
            return self._prepared
        _, P = pattern(self.G)
        n = P.shape[0]
        candidates, _ = sample(n, self.max_positive_samples, self.seed)
        counts = np.bincount(candidates, minlength=n).astype(np.int64)
        rows = np.flatnonzero(counts)
        PS = P[rows]
        closed = np.asarray((PS @ P).multiply(PS).sum(axis=1)).ravel().astype(np.int64) if len(rows) else np.zeros(0, dtype=np.int64)
        self._prepared = dict(P=P, counts=counts, denominator=int(np.dot(closed, counts[rows])), graph=None, device_counts=None)
        return self._prepared

    def evaluate(self, scores):
        prepared = self._prepare()
        matrix = slab_of(self.G, scores)
        if prepared["denominator"] == 0:
            return 0
        entry = L.entry("pgh_link_factors") if self.fused else None
        if entry is not None:
            if prepared["graph"] is None:
                # the engine's conv(x, M) is M^T x and P t is wanted: upload P^T
                prepared["graph"] = DeviceGraph.from_scipy(sp.csr_array(prepared["P"].T, dtype=np.float64))
                prepared["device_counts"] = DeviceVector.from_host(prepared["counts"].astype(np.float64))
            t = DeviceVector.empty(matrix.n)
            L.check(entry(matrix._h, _SIMILARITIES[self.similarity], t._h))
            y = prepared["graph"].conv(t)
            self.last_route = "device"
            numerator = float((prepared["device_counts"] * y).dot(y))
        else:
            self.last_route = "host"
            y = prepared["P"].astype(np.float64) @ host_factors(matrix.numpy(), self.similarity)
            numerator = float(np.dot(prepared["counts"] * y, y))
        return numerator / prepared["denominator"]

    def __call__(self, scores):
        return self.evaluate(scores)


def _groups(scores):
    """[(group id or position, scores)] in the groups' order."""
    if isinstance(scores, DeviceMatrix):
        return list(enumerate(scores.columns()))
    if hasattr(scores, "items") and not isinstance(scores, GraphSignal):
        return list(scores.items())
    return list(enumerate(scores))


def _mean(evaluations):
    return sum(evaluations) / len(evaluations)


class MultiUnsupervised:
    """multigroup.py:149-158: the mean over the groups of one unsupervised measure of the graph.  evaluate(scores, exact=False) hands
    all groups to the measure's ``evaluate_many`` once -- on the engine its slab route, two passes over the adjacency for 64 groups --
    and agrees with the loop to that measure's tolerance."""

    def __init__(self, metric_type, G, **kwargs):
        self.metric = metric_type(G, **kwargs)

    def evaluate(self, scores, exact=True):
        many = getattr(self.metric, "evaluate_many", None)
        if not exact and many is not None:
            return _mean(many(scores if isinstance(scores, DeviceMatrix) else [group for _, group in _groups(scores)]))
        return _mean([self.metric.evaluate(group) for _, group in _groups(scores)])

    def __call__(self, scores):
        return self.evaluate(scores)


class MultiSupervised:
    """multigroup.py:161-170: the mean over the groups of one supervised measure, each group against its own ground truth (and its own
    exclude list).  Scores given as a list or a DeviceMatrix meet the ground truths in their order.  evaluate(scores, exact=False)
    stacks the groups' ground truths (and exclude values) into slabs and hands all groups to ONE measure's ``evaluate_many`` -- for the
    closed-form measures one pgh_pair_forms pass per 64 groups -- and agrees with the loop to that measure's tolerance."""

    def __init__(self, metric_type, ground_truth, exclude=None):
        self.metric_type = metric_type
        self.ground_truth = ground_truth
        self.exclude = exclude
        self.metrics = {group_id: metric_type(group_truth) if exclude is None else metric_type(group_truth, exclude[group_id])
                        for group_id, group_truth in ground_truth.items()}

    def _keyed(self, scores):
        if hasattr(scores, "items") and not isinstance(scores, (GraphSignal, DeviceMatrix)):
            return list(scores.items())
        return list(zip(self.ground_truth, scores.columns() if isinstance(scores, DeviceMatrix) else scores))

    def evaluate(self, scores, exact=True):
        keyed = self._keyed(scores)
        if not exact and hasattr(self.metric_type, "evaluate_many"):
            ids = [group_id for group_id, _ in keyed]
            columns = [group for _, group in keyed]
            truths = [self.ground_truth[group_id] for group_id in ids]
            anchor = next((value for value in columns + truths if isinstance(value, GraphSignal)), None)

            def dense(obj):
                vector = to_signal(anchor, obj).np if anchor is not None else backend.to_array(obj)
                vector._h                   # noqa: B018 -- an unevaluated expression (device.LazyVector) is evaluated first
                return vector
            known = DeviceMatrix.from_columns([dense(truth) for truth in truths])
            if self.exclude is None:
                measure = self.metric_type(known)
            else:
                if anchor is None:
                    raise Exception("Needs to parse graph signal scores or known_scores to be able to exclude specific nodes")
                measure = self.metric_type(known, DeviceMatrix.from_columns([dense(self.exclude[group_id]) for group_id in ids]))
            # a bare slab names no graph, and a measure excludes nodes only where a graph signal does: its columns then go as signals
            many = measure.evaluate_many(scores if isinstance(scores, DeviceMatrix) and self.exclude is None else
                                         [to_signal(anchor, column) if anchor is not None else column for column in columns])
            return _mean(many)
        return _mean([self.metrics[group_id].evaluate(group) for group_id, group in keyed])

    def __call__(self, scores):
        return self.evaluate(scores)
