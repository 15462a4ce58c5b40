"""Residual measures used as convergence criteria -- Mabs (default), L1, MaxDifference -- and the residual-style supervised
measures on vectors already in HBM (RMabs, MSQ, MSQRT, L2, Euclidean, Cos, Dot; supervised.py:109-154,208-222).

Restates pygrank/measures/supervised.py:18-47 (Supervised.to_numpy), :93-98 (MaxDifference), :101-106 (Mabs),
:133-138 (L1).  When both operands are HBM vectors the residual is ONE fused HIP reduction
(pgh_residual: |a - b| folded into an f64 sum / max) instead of the reference's three passes
(subtract, abs, sum).  AUC (supervised.py:255-263) is one device sort (pgh_auc); the other evaluation measures of the
reference (NDCG, ...) are out of scope.

The unsupervised measures Conductance and Density (pygrank/measures/unsupervised.py:8-145) score a ranking without ground truth.  They are
the reference's only measures that run `conv` themselves: two passes over the adjacency per score column.  Here the columns of a batch
travel as one slab (include/pgh_measure.h: pgh_mat_col_stats + pgh_cut_forms): 64 columns cost two passes.
"""
import collections.abc
import ctypes as C
import numbers
import random

from pygrank_amd import _lib as L
from pygrank_amd import backend
from pygrank_amd.device import DeviceGraph, DeviceMatrix, DeviceVector, lazy_residual
from pygrank_amd.preprocessing import AdjacencyWrapper, preprocessor as default_preprocessor
from pygrank_amd.signals import GraphSignal, to_signal

# private: True sends Conductance / Density down the per-column route (backend.conv, dot, sum, max) even where the library has the slab
# entries -- a GPU test compares the two routes with it
_FORCE_PER_COLUMN = False


class Measure:
    def __call__(self, scores):
        return self.evaluate(scores)

    def evaluate(self, scores):
        raise Exception("Non-abstract subclasses of Measure should implement an evaluate method")

    def best_direction(self):                                # measures/utils.py:15-24
        return 1


class Supervised(Measure):
    """supervised.py:18-55."""
    _KIND = None

    def __init__(self, known_scores, exclude=None):
        self.known_scores = known_scores
        self.exclude = exclude

    def to_numpy(self, scores, normalization=False):
        """supervised.py:36-47 -> (known, scores) as two aligned vectors.  Two plain numbers become one-element vectors.  When
        either side is a graph signal it lends its graph to the other, the scores are (optionally) normalised and both lose the
        excluded nodes; two plain vectors are taken as they are (nothing to exclude nodes by)."""
        known = self.known_scores
        if all(isinstance(value, numbers.Number) for value in (scores, known)):
            return backend.to_array([known]), backend.to_array([scores])
        anchor = next((value for value in (scores, known) if isinstance(value, GraphSignal)), None)
        if anchor is not None:
            aligned = (to_signal(anchor, known), to_signal(anchor, scores).normalized(normalization))
            return tuple(signal.filter(exclude=self.exclude) for signal in aligned)
        if self.exclude is not None:
            raise Exception("Needs to parse graph signal scores or known_scores to be able to exclude specific nodes")
        plain = backend.to_array(scores, copy_array=bool(normalization))
        return backend.to_array(known), (backend.self_normalize(plain) if normalization else plain)

    def best_direction(self):
        """supervised.py:49-54: 1 when larger values of the measure are better, -1 otherwise -- found once per class by scoring a
        perfect and an inverted answer."""
        cls = type(self)
        found = cls.__dict__.get("_best_direction")
        if found is None:
            found = 1 if cls([1, 0])([1, 0]) > cls([1, 0])([0, 1]) else -1
            cls._best_direction = found
        return found

    def evaluate(self, scores):
        known, scores = self.to_numpy(scores)
        if isinstance(known, DeviceVector) and isinstance(scores, DeviceVector):
            # two iterates of one graph that are still in the engine's id space (device.LazyVector): the residual is taken there
            resident = lazy_residual(self._KIND, known, scores)
            if resident is not None:
                return resident
            out = C.c_double()
            L.check(L.lib().pgh_residual(self._KIND, known._h, scores._h, C.byref(out)))
            return out.value
        raise Exception("residual measures expect backend vectors")


class MaxDifference(Supervised):                             # supervised.py:93-98
    _KIND = L.ERR_LINF


class Mabs(Supervised):                                      # supervised.py:101-106
    _KIND = L.ERR_MABS


class L1(Supervised):                                        # supervised.py:133-138
    _KIND = L.ERR_L1


class _Pairwise(Supervised):
    """Measures that are a handful of device reductions over the two score vectors."""

    def _pair(self, scores):
        known, scores = self.to_numpy(scores)
        if not (isinstance(known, DeviceVector) and isinstance(scores, DeviceVector)):
            raise Exception("residual measures expect backend vectors")
        return known, scores

    def _squared_distance(self, scores):
        known, scores = self._pair(scores)
        d = known - scores
        return d.dot(d), len(scores)


class RMabs(_Pairwise):                                      # supervised.py:109-114
    def evaluate(self, scores):
        known, scores = self._pair(scores)
        out = C.c_double()
        L.check(L.lib().pgh_residual(L.ERR_L1, known._h, scores._h, C.byref(out)))
        return out.value / known.abssum()


class MSQ(_Pairwise):                                        # supervised.py:117-122
    def evaluate(self, scores):
        total, n = self._squared_distance(scores)
        return total / n


class MSQRT(_Pairwise):                                      # supervised.py:125-130
    def evaluate(self, scores):
        total, n = self._squared_distance(scores)
        return (total / n) ** 0.5


class L2(_Pairwise):                                         # supervised.py:141-146 (the squared distance, as the reference)
    def evaluate(self, scores):
        return self._squared_distance(scores)[0]


class Euclidean(_Pairwise):                                  # supervised.py:149-154
    def evaluate(self, scores):
        return self._squared_distance(scores)[0] ** 0.5


class Cos(_Pairwise):                                        # supervised.py:208-214
    def evaluate(self, scores):
        known, scores = self._pair(scores)
        return backend.safe_div(known.dot(scores), (known.dot(known) * scores.dot(scores)) ** 0.5)


class AUC(_Pairwise):                                        # supervised.py:255-263 (sklearn roc_curve + auc in the reference)
    """Area under the ROC curve of the scores against binary known scores, ties at their mid-rank, with ONE device sort
    (pgh_auc) instead of a trip through sklearn on the host."""

    def evaluate(self, scores):
        known, scores = self._pair(scores)
        out, positives = C.c_double(), C.c_int64()
        L.check(L.lib().pgh_auc(known._h, scores._h, C.byref(out), C.byref(positives)))
        if positives.value == 0 or positives.value == len(scores):
            raise Exception("Cannot evaluate AUC when all labels are the same")
        return out.value


class Dot(_Pairwise):                                        # supervised.py:217-222
    def evaluate(self, scores):
        known, scores = self._pair(scores)
        return known.dot(scores)


class Unsupervised(Measure):
    """unsupervised.py:8-49: a measure of the scores and the graph alone.  `graph` may be left out when graph signals are evaluated;
    without a preprocessor the graph is taken unnormalised (normalization="none") unless a normalization is named."""

    def __init__(self, graph=None, preprocessor=None, **kwargs):
        self.graph = graph
        if preprocessor is None and "normalization" not in kwargs:
            kwargs["normalization"] = "none"
        self.preprocessor = default_preprocessor(**kwargs) if preprocessor is None else preprocessor
        self.last_route = None                               # "slab" or "columns": the route the last evaluation took

    def to_numpy(self, scores=None):                         # unsupervised.py:30-33
        scores = to_signal(self.graph, scores)
        return self.preprocessor(scores.graph), scores.np

    def get_graph(self, scores=None):                        # unsupervised.py:35-39
        if scores is not None and isinstance(scores, GraphSignal):
            return to_signal(self.graph, scores).graph
        return self.graph

    def best_direction(self):
        """unsupervised.py:41-49: 1 when larger is better, found once per class on two triangles joined by an edge (A-B, B-C, C-A, C-D,
        D-E, E-F, F-D): one triangle {A, B, C} against the scattered {A, C, F}.  The probe graph is a scipy matrix behind
        AdjacencyWrapper(directed=False), nodes A .. F = 0 .. 5."""
        cls = type(self)
        found = cls.__dict__.get("_best_direction")
        if found is None:
            import numpy as np
            import scipy.sparse as sp
            edges = [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 5), (5, 3)]
            rows = [a for a, b in edges] + [b for a, b in edges]
            cols = [b for a, b in edges] + [a for a, b in edges]
            graph = AdjacencyWrapper(sp.csr_array((np.ones(len(rows)), (rows, cols)), shape=(6, 6)), directed=False)
            found = 1 if cls(graph)([0, 1, 2]) > cls(graph)([0, 2, 5]) else -1
            cls._best_direction = found
        return found

    # ---- the two routes ------------------------------------------------------------------------------------------------------
    _FORMS = L.CUT_ALL

    def _empty(self):
        raise NotImplementedError

    def _plan(self, stats):
        """Per-column factors of a slab from its column statistics [b, 4] = sum, sum of squares, max, min (or None: all ones)."""
        return None

    def _from_forms(self, graph, forms, stats):
        raise NotImplementedError

    def _one(self, graph, adjacency, scores):
        """The reference's route for one column, one backend primitive at a time."""
        raise NotImplementedError

    def _slab(self, graph, device_graph, matrix):
        """The slab route over a DeviceMatrix, 64 columns at a time; None when the engine declines."""
        stats_fn, forms_fn = L.measure_entry("pgh_mat_col_stats"), L.measure_entry("pgh_cut_forms")
        import numpy as np
        out = []
        for first in range(0, matrix.b, 64):
            part = matrix if matrix.b <= 64 else matrix.get_cols(first, min(64, matrix.b - first))
            stats = np.empty((part.b, 4), dtype=np.float64)
            L.check(stats_fn(part._h, stats.ctypes.data_as(C.c_void_p)))
            factors = self._plan(stats)
            forms = np.empty((part.b, 4), dtype=np.float64)
            status = forms_fn(device_graph._h, part._h, None if factors is None else factors.ctypes.data_as(C.c_void_p),
                              float(getattr(self, "max_rank", 1)), self._FORMS, forms.ctypes.data_as(C.c_void_p))
            if status == L.MEASURE_DECLINED:
                return None
            L.check(status)
            out.extend(self._from_forms(graph, [float(v) for v in forms[j]], [float(v) for v in stats[j]]) for j in range(part.b))
        return out

    def _route(self, graph, adjacency, columns):
        """Scores of `columns` (a DeviceMatrix or a list of vectors) on the preprocessed graph."""
        device_graph = getattr(adjacency, "array", adjacency)
        if not _FORCE_PER_COLUMN and isinstance(device_graph, DeviceGraph) and L.measure_entry("pgh_cut_forms") is not None \
                and L.measure_entry("pgh_mat_col_stats") is not None:
            matrix = columns if isinstance(columns, DeviceMatrix) else DeviceMatrix.from_columns(columns)
            out = self._slab(graph, device_graph, matrix)
            if out is not None:
                self.last_route = "slab"
                return out
        self.last_route = "columns"
        vectors = columns.columns() if isinstance(columns, DeviceMatrix) else columns
        for vector in vectors:
            # an unevaluated expression (device.LazyVector) is evaluated first: the scores are the stored f32 values on either route,
            # and a second evaluation of the same signal repeats the first bit for bit
            vector._h                       # noqa: B018
        return [self._one(graph, adjacency, vector) for vector in vectors]

    def evaluate(self, scores):
        graph = self.get_graph(scores)
        if len(graph) == 0:
            return self._empty()
        adjacency, scores = self.to_numpy(scores)
        return self._route(graph, adjacency, [scores])[0]

    def evaluate_many(self, columns):
        """What evaluate returns for every column, as a list of floats: `columns` is a DeviceMatrix over the measure's graph, or a list of
        graph signals / score vectors of one graph.  The columns share the graph's preprocessing and, on the slab route, the passes over
        it; a column that evaluate would refuse raises here too (the first such column, as a loop over evaluate would)."""
        if isinstance(columns, DeviceMatrix):
            if self.graph is None:
                raise Exception("a slab of score columns can only be evaluated by a measure that was given its graph")
            graph = self.graph.graph if isinstance(self.graph, GraphSignal) else self.graph
            count = columns.b
        else:
            signals = [to_signal(self.graph, column) for column in columns]
            if not signals:
                return []
            graph = signals[0].graph
            if any(signal.graph is not graph for signal in signals):
                raise Exception("the score columns belong to different graphs")
            columns, count = [signal.np for signal in signals], len(signals)
        if len(graph) == 0:
            return [self._empty() for _ in range(count)]
        if isinstance(columns, DeviceMatrix) and columns.n != len(graph):
            raise Exception(f"a slab of {columns.n} rows cannot hold scores of {len(graph)} nodes")
        return self._route(graph, self.preprocessor(graph), columns)


class Conductance(Unsupervised):
    """unsupervised.py:52-111: E[outgoing edges] / E[internal edges] of the fuzzy subgraph the scores describe; infinite when either is
    zero.  max_rank bounds the scores: a larger score raises, or with autofix the scores are scaled by max_rank / their maximum."""

    def __init__(self, graph=None, max_rank=1, autofix=False, cut_ratio_only=False, **kwargs):
        self.max_rank = max_rank
        self.autofix = autofix
        self.cut_ratio_only = cut_ratio_only
        super().__init__(graph, **kwargs)

    def _empty(self):
        return float("inf")

    def _refuse(self):
        raise Exception("Normalize scores to be <= " + str(self.max_rank) + " for non-negative conductance")

    def _plan(self, stats):
        import numpy as np
        factors = np.ones(len(stats), dtype=np.float64)
        for j, column in enumerate(stats):
            if column[2] > self.max_rank:
                if not self.autofix:
                    self._refuse()
                factors[j] = self.max_rank / column[2]
        return factors

    def _ratio(self, graph, neighbors_scores, neighbors_rest, rest_scores, rest_rest):
        """unsupervised.py:102-111 from the four forms <N, s>, <N, c>, <C, s>, <C, c> (the last two as callables: taken when needed)."""
        internal_edges = neighbors_scores
        if not self.cut_ratio_only:
            internal_edges = min(internal_edges, rest_rest())
        external_edges = neighbors_rest
        if not graph.is_directed():
            external_edges += rest_scores()
            internal_edges *= 2
        if external_edges == 0:
            return float("inf")
        return backend.safe_div(external_edges, internal_edges, default=float("inf"))

    def _from_forms(self, graph, forms, stats):
        return self._ratio(graph, forms[0], forms[1], lambda: forms[2], lambda: forms[3])

    def _one(self, graph, adjacency, scores):
        largest = backend.max(scores)
        if largest > self.max_rank:
            if not self.autofix:
                self._refuse()
            scores = scores * (self.max_rank / largest)
        rest = self.max_rank - scores
        neighbors = backend.conv(scores, adjacency)
        return self._ratio(graph, backend.dot(neighbors, scores), backend.dot(neighbors, rest),
                           lambda: backend.dot(scores, backend.conv(rest, adjacency)),
                           lambda: backend.dot(backend.conv(rest, adjacency), rest))


class Density(Unsupervised):
    """unsupervised.py:114-145: E[internal edges] / E[possible edges] of the fuzzy subgraph the scores describe (no self-loops)."""
    _FORMS = L.CUT_INTERNAL

    def __init__(self, graph=None, **kwargs):
        super().__init__(graph, **kwargs)

    def _empty(self):
        return 0

    def _from_forms(self, graph, forms, stats):
        return backend.safe_div(forms[0], stats[0] ** 2 - stats[1])

    def _one(self, graph, adjacency, scores):
        internal_edges = backend.dot(backend.conv(scores, adjacency), scores)
        expected_edges = backend.sum(scores) ** 2 - backend.sum(scores ** 2)
        return backend.safe_div(internal_edges, expected_edges)


def split(groups, training_samples=0.8, seed=0):
    """measures/utils.py:48-92: (training, test) of a graph signal (its non-zero nodes are dealt to the two sides, the others are
    zero on both), of an iterable (two lists) or of a mapping of such (two mappings).  training_samples: below 1 a fraction, above 1
    a count, negative = all but that many, exactly 1 = no split (both sides are the input).  The order is the reference's:
    ``sorted`` (unless seed is None), then ``random.Random(seed).shuffle``.  The non-zero nodes of a signal are read from its host
    mirror (one download) instead of one dictionary read per node of the graph."""
    if training_samples == 1:
        return groups, groups
    if isinstance(groups, collections.abc.Mapping) and not isinstance(groups, GraphSignal):
        training, testing = {}, {}
        for group_id, group in groups.items():
            training[group_id], testing[group_id] = split(group, training_samples, seed)
        return training, testing
    values = None
    if isinstance(groups, GraphSignal):
        values, node2id = groups._mirror(), groups.node2id
        if hasattr(node2id, "n"):                            # nodes are positions (signals._IdentityMap): ascending = iteration order
            group = [int(i) for i in values.nonzero()[0]]
        else:
            group = [node for node in groups if values[node2id[node]] != 0]
    else:
        group = list(groups)
    if seed is not None:
        group = sorted(group)
    random.Random(seed).shuffle(group)
    count = len(group)
    cut = int(training_samples) if training_samples > 1 else \
        (int(count * training_samples) if training_samples >= 0 else count + int(training_samples))
    if values is None:
        return group[:cut], group[cut:]
    return tuple(to_signal(groups, {node: float(values[groups.node2id[node]]) for node in side}) for side in (group[:cut], group[cut:]))
