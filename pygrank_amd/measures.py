"""Residual measures used as convergence criteria -- Mabs (default), L1, MaxDifference -- and the residual-style supervised
measures on vectors already in HBM (RMabs, MSQ, MSQRT, L2, Euclidean, Cos, Dot; supervised.py:109-154,208-222).

Restates pygrank/measures/supervised.py:18-47 (Supervised.to_numpy), :93-98 (MaxDifference), :101-106 (Mabs),
:133-138 (L1).  When both operands are HBM vectors the residual is ONE fused HIP reduction
(pgh_residual: |a - b| folded into an f64 sum / max) instead of the reference's three passes
(subtract, abs, sum).  AUC (supervised.py:255-263) is one device sort (pgh_auc).

The other closed-form supervised measures of the reference are here too: Accuracy, TPR, TNR, PPV (supervised.py:225-271), pRule and
L2Disparity (:290-333), BinaryCrossEntropy, CrossEntropy, KLDivergence, MKLDivergence (:157-205), PearsonCorrelation (:282-287) and
MannWhitneyParity (:336-350).  Every supervised measure has ``evaluate_many(columns)`` for the columns of a batch.  All but the
sort-based ones are functions of a handful of per-column sums over (score, known) pairs, and one streaming kernel takes every such sum
for 64 columns while it reads each row of the slab once (include/pgh_supervised.h: pgh_pair_forms).  On a
library without that entry -- the host test double -- the same classes take the reference's route one backend primitive at a time.
AUC and MannWhitneyParity score a slab through the tuner's pgh_probe_auc (include/pgh_tune.h) with an identity coefficient matrix.
NDCG (supervised.py:68-90) and SpearmanCorrelation (:274-279) score a slab through include/pgh_rank.h: the DCG
of 64 columns in one streaming pass, Spearman's rho with one device sort per column, both through a plan shared by every call.  The
combinations of measures/combination.py (AM, GM, Disparity, Parity) live in pygrank_amd/combination.py and are re-exported here.
measures/multigroup.py lives in pygrank_amd/multigroup.py; Mistreatment stays out of scope.

The unsupervised measures Conductance and Density (pygrank/measures/unsupervised.py:8-145) score a ranking without ground truth.  They are
the reference's only measures that run `conv` themselves: two passes over the adjacency per score column.  Here the columns of a batch
travel as one slab (include/pgh_measure.h: pgh_mat_col_stats + pgh_cut_forms): 64 columns cost two passes.
Modularity (unsupervised.py:148-201) is a closed form over the same entries in place of the reference's loop over has_edge.
"""
import collections.abc
import ctypes as C
import itertools
import numbers
import random

from pygrank_amd import _lib as L
from pygrank_amd import backend
from pygrank_amd.device import DeviceGraph, DeviceMatrix, DeviceVector, EnginePlan, lazy_residual
from pygrank_amd.preprocessing import AdjacencyWrapper, preprocessor as default_preprocessor
from pygrank_amd.signals import GraphSignal, to_signal

# private: True sends Conductance / Density and the supervised measures' evaluate_many down the per-column route (one backend primitive
# at a time) even where the library has the slab entries -- a GPU test compares the two routes with it
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

    # ---- the columns of a batch -------------------------------------------------------------------------------------------------
    _GROUP = L.PAIR_MOMENTS       # the slots of pgh_pair_forms the measure is derived from
    _NORMALIZE = False            # KLDivergence, MKLDivergence: to_numpy(scores, normalization=True)
    _from_slots = None            # (slots [20], eps) -> value on the slab route; None: no slab route through pgh_pair_forms
    last_route = None             # "slab" or "columns": the route the last evaluate_many took

    def _one(self, scores):
        """What the columns route returns for one column."""
        return self.evaluate(scores)

    @staticmethod
    def _dense(anchor, obj):
        """The unfiltered backend vector of scores, known scores or exclude values."""
        if anchor is not None:
            return to_signal(anchor, obj).np
        return backend.to_array([obj] if isinstance(obj, numbers.Number) else obj)

    def _slab_available(self):
        return self._from_slots is not None and L.entry("pgh_pair_forms") is not None

    def _operand(self, anchor, side, rows, name):
        """(vector, matrix) of the known scores or the exclude values for a slab of `rows` rows; one of them is None (both for None)."""
        if side is None:
            return None, None
        if isinstance(side, DeviceMatrix):
            if side.n != rows:
                raise Exception(f"{name} of {side.n} rows cannot go with score columns of {rows} rows")
            return None, side
        vector = self._dense(anchor, side)
        vector._h                           # noqa: B018 -- an unevaluated expression (device.LazyVector) is evaluated first
        if len(vector) != rows:
            raise Exception(f"a slab of {rows} rows cannot be scored against {name} of {len(vector)} nodes")
        return vector, None

    def _matrix(self, anchor, columns):
        if isinstance(columns, DeviceMatrix):
            return columns
        return DeviceMatrix.from_columns([self._dense(anchor, column) for column in columns])

    def _slab(self, anchor, columns, count):
        """The slab route: one pgh_pair_forms call per 64 columns, the values derived on the host from its slots.  None when the engine
        declines."""
        import numpy as np
        entry = L.entry("pgh_pair_forms")
        matrix = self._matrix(anchor, columns)
        known_vec, known_mat = self._operand(anchor, self.known_scores, matrix.n, "known scores")
        exclude_vec, exclude_mat = self._operand(anchor, self.exclude, matrix.n, "exclude values")
        eps = backend.epsilon()
        factors = None
        if self._NORMALIZE:
            # supervised.py:182: the scores are normalised BEFORE the excluded nodes leave -- the L1 norm is taken over all rows
            sums = matrix.col_abssum()
            factors = np.where(sums != 0, 1.0 / np.where(sums != 0, sums, 1.0), 1.0)
        out = []

        # a side given per column is cut in step with the scores; evaluate_many has checked that it holds as many columns as they do
        # (zip would stop at the shorter one without a word)
        def cut(side):
            return itertools.repeat((0, None)) if side is None else side.chunks()
        for (first, part), (_, kmat), (_, emat) in zip(matrix.chunks(), cut(known_mat), cut(exclude_mat)):
            width = part.b
            chunk = None if factors is None else np.ascontiguousarray(factors[first:first + width])
            slots = np.empty((width, L.PAIR_SLOTS), dtype=np.float64)
            status = entry(part._h, None if known_vec is None else known_vec._h, None if kmat is None else kmat._h,
                           None if exclude_vec is None else exclude_vec._h, None if emat is None else emat._h,
                           None if chunk is None else chunk.ctypes.data_as(C.c_void_p), eps, self._GROUP,
                           slots.ctypes.data_as(C.c_void_p))
            if not L.accepted(status):
                return None
            out.extend(self._from_slots([float(v) for v in slots[j]], eps) for j in range(width))
        return out

    def _per_column(self, anchor, columns):
        """The columns route: what a loop over evaluate returns."""
        import copy
        known, exclude = self.known_scores, self.exclude
        vectors = columns.columns() if isinstance(columns, DeviceMatrix) else columns
        out = []
        for j, column in enumerate(vectors):
            measure = self
            if isinstance(known, DeviceMatrix) or isinstance(exclude, DeviceMatrix):
                measure = copy.copy(self)
                measure.known_scores = known.column(j) if isinstance(known, DeviceMatrix) else known
                measure.exclude = exclude.column(j) if isinstance(exclude, DeviceMatrix) else exclude
            if anchor is not None and not isinstance(column, GraphSignal):
                column = to_signal(anchor, column)
            out.append(measure._one(column))
        return out

    def evaluate_many(self, columns):
        """What evaluate returns for every column, as a list of floats.  `columns` is a DeviceMatrix, or a list of graph signals or score
        vectors of one graph.  known_scores and exclude are each one signal or vector shared by the columns, or a DeviceMatrix with one
        column per score column.  On the slab route the columns share one pass (pgh_pair_forms, 64 columns at a time; AUC: pgh_probe_auc);
        a column that evaluate would refuse raises here too (the first such column, as a loop over evaluate would)."""
        known, exclude = self.known_scores, self.exclude
        if isinstance(columns, DeviceMatrix):
            count = columns.b
            anchor = known if isinstance(known, GraphSignal) else None
        else:
            columns = list(columns)
            count = len(columns)
            if count == 0:
                return []
            anchor = next((column for column in columns if isinstance(column, GraphSignal)), None)
            if anchor is None and isinstance(known, GraphSignal):
                anchor = known
            if anchor is not None and any(isinstance(column, GraphSignal) and column.graph is not anchor.graph for column in columns):
                raise Exception("the score columns belong to different graphs")
        for name, side in (("known_scores", known), ("exclude", exclude)):
            if isinstance(side, DeviceMatrix) and side.b != count:
                raise Exception(f"{name} holds {side.b} columns for {count} score columns")
        if anchor is None and exclude is not None:
            raise Exception("Needs to parse graph signal scores or known_scores to be able to exclude specific nodes")
        if isinstance(columns, DeviceMatrix) and anchor is None and not isinstance(known, (DeviceMatrix, numbers.Number)) \
                and len(known) != columns.n:
            # said here once, for both routes, and not by whichever primitive meets the two lengths first
            raise Exception(f"a slab of {columns.n} rows cannot be scored against known scores of {len(known)} nodes")
        if not _FORCE_PER_COLUMN and self._slab_available():
            out = self._slab(anchor, columns, count)
            if out is not None:
                self.last_route = "slab"
                return out
        self.last_route = "columns"
        return self._per_column(anchor, columns)

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


def _ieee_div(a, b):
    """a / b as IEEE arithmetic has it (nan for 0 / 0, an infinity for x / 0): what numpy returns where Python raises."""
    if b != 0:
        return a / b
    return float("nan") if a == 0 or a != a else (float("inf") if a > 0 else float("-inf"))


def _ieee_sqrt(a):
    return a ** 0.5 if a >= 0 else float("nan")


# The slots of pgh_pair_forms (include/pgh_supervised.h) per column, over the kept rows:
#   0 count   1 sum s   2 sum s^2   3 sum k   4 sum k^2   5 sum k s   6 sum |k - s|   7 sum (k - s)^2   8 max |k - s|   9 max s   10 max k
#   11 sum |k|   12 sum k log(s + eps)   13 sum (1 - k) log(1 - s + eps)   14 sum (s + eps) log(s + eps)   15 sum (s + eps) log(k + eps)
#   16 sum s log(k)
class MaxDifference(Supervised):                             # supervised.py:93-98
    _KIND = L.ERR_LINF

    def _from_slots(self, s, eps):
        return s[8]


class Mabs(Supervised):                                      # supervised.py:101-106
    _KIND = L.ERR_MABS

    def _from_slots(self, s, eps):
        return _ieee_div(s[6], s[0])


class L1(Supervised):                                        # supervised.py:133-138
    _KIND = L.ERR_L1

    def _from_slots(self, s, eps):
        return s[6]


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

    def _from_slots(self, s, eps):
        return _ieee_div(s[6], s[11])


class MSQ(_Pairwise):                                        # supervised.py:117-122
    def evaluate(self, scores):
        total, n = self._squared_distance(scores)
        return total / n

    def _from_slots(self, s, eps):
        return _ieee_div(s[7], s[0])


class MSQRT(_Pairwise):                                      # supervised.py:125-130
    def evaluate(self, scores):
        total, n = self._squared_distance(scores)
        return (total / n) ** 0.5

    def _from_slots(self, s, eps):
        return _ieee_sqrt(_ieee_div(s[7], s[0]))


class L2(_Pairwise):                                         # supervised.py:141-146 (the squared distance, as the reference)
    def evaluate(self, scores):
        return self._squared_distance(scores)[0]

    def _from_slots(self, s, eps):
        return s[7]


class Euclidean(_Pairwise):                                  # supervised.py:149-154
    def evaluate(self, scores):
        return self._squared_distance(scores)[0] ** 0.5

    def _from_slots(self, s, eps):
        return _ieee_sqrt(s[7])


class Cos(_Pairwise):                                        # supervised.py:208-214
    def evaluate(self, scores):
        known, scores = self._pair(scores)
        return backend.safe_div(known.dot(scores), (known.dot(known) * scores.dot(scores)) ** 0.5)

    def _from_slots(self, s, eps):
        return backend.safe_div(s[5], _ieee_sqrt(s[4] * s[2]))


class _ProbePlan(EnginePlan):
    """The node classes of one (known scores, exclude) pair on the device (pgh_probe_plan_create, include/pgh_tune.h)."""
    _DESTROY = "pgh_probe_plan_destroy"

    def __init__(self, known, exclude):
        self._h = L.c_plan()
        L.check(L.entry("pgh_probe_plan_create")(known._h, None if exclude is None else exclude._h, C.byref(self._h)))
        positive, negative = C.c_int64(), C.c_int64()
        L.check(L.entry("pgh_probe_plan_info")(self._h, C.byref(positive), C.byref(negative)))
        self.num_positive, self.num_negative = positive.value, negative.value


class AUC(_Pairwise):                                        # supervised.py:255-263 (sklearn roc_curve + auc in the reference)
    """Area under the ROC curve of the scores against binary known scores, ties at their mid-rank, with ONE device sort
    (pgh_auc) instead of a trip through sklearn on the host.  The columns of a slab that share their known scores and exclude values
    are scored by pgh_probe_auc (include/pgh_tune.h) with an identity coefficient matrix (terms = probes = columns): the entry then
    returns the AUC of each stored column, the value pgh_auc returns for it."""
    _SAME_CLASS = "Cannot evaluate AUC when all labels are the same"
    _MANY_IS_EXACT = True         # evaluate_many equals a loop over evaluate to the bit (pair counts are integers): see combination.py

    def _auc(self, scores):
        known, scores = self._pair(scores)
        out, positives = C.c_double(), C.c_int64()
        L.check(L.lib().pgh_auc(known._h, scores._h, C.byref(out), C.byref(positives)))
        if positives.value == 0 or positives.value == len(scores):
            raise Exception(self._SAME_CLASS)
        return out.value

    def _of_auc(self, auc):
        return auc

    def evaluate(self, scores):
        return self._of_auc(self._auc(scores))

    def _slab_available(self):
        return all(L.entry(name) is not None for name in L.TUNE_SIGNATURES)

    def _slab(self, anchor, columns, count):
        import numpy as np
        if isinstance(self.known_scores, DeviceMatrix) or isinstance(self.exclude, DeviceMatrix):
            return None                                      # known scores per column: one plan per column, no shared pass
        matrix = self._matrix(anchor, columns)
        known, _ = self._operand(anchor, self.known_scores, matrix.n, "known scores")
        exclude, _ = self._operand(anchor, self.exclude, matrix.n, "exclude values")
        plan = _ProbePlan(known, exclude)
        if plan.num_positive == 0 or plan.num_negative == 0:
            raise Exception(self._SAME_CLASS)
        out = []
        for _, part in matrix.chunks():
            width = part.b
            identity = np.ascontiguousarray(np.eye(width, dtype=np.float64))
            aucs = (C.c_double * width)()
            status = L.entry("pgh_probe_auc")(part._h, identity.ctypes.data_as(C.c_void_p), width, width, plan._h, aucs)
            if not L.accepted(status):
                return None
            out.extend(self._of_auc(float(v)) for v in aucs)
        return out


class Dot(_Pairwise):                                        # supervised.py:217-222
    def evaluate(self, scores):
        known, scores = self._pair(scores)
        return known.dot(scores)

    def _from_slots(self, s, eps):
        return s[5]


class _ClosedForm(_Pairwise):
    """The measures below: ``evaluate`` is the one-column case of ``evaluate_many``.  ``_value`` is the reference's formula over the
    filtered vectors, one backend primitive at a time (the columns route); ``_from_slots`` derives the same value from the slots of
    pgh_pair_forms (the slab route).  On the slab route every ``evaluate`` packs its scores into a one-column DeviceMatrix first: one
    copy of the vector per call, which a caller that scores many vectors in a loop (a fairness postprocessor's loss) avoids by
    handing them to ``evaluate_many`` together."""

    def _value(self, known, scores):
        raise NotImplementedError

    def _one(self, scores):
        known, scores = self.to_numpy(scores, normalization=self._NORMALIZE)
        if not (isinstance(known, DeviceVector) and isinstance(scores, DeviceVector)):
            raise Exception("supervised measures expect backend vectors")
        return self._value(known, scores)

    def evaluate(self, scores):
        return self.evaluate_many([scores])[0]


class Accuracy(_ClosedForm):                                 # supervised.py:266-271
    """1 - the mean absolute difference of the scores and the known scores."""

    def _value(self, known, scores):
        return 1 - backend.sum(backend.abs(known - scores)) / backend.length(scores)

    def _from_slots(self, s, eps):
        return 1 - _ieee_div(s[6], s[0])


class _Rates(_ClosedForm):
    """TPR, TNR, PPV (supervised.py:225-252): both sides are divided by their maximum (a zero maximum leaves the scalar 0, as
    backend.safe_div does), then A = sum k s, K = sum k, S = sum s of the divided sides."""

    @staticmethod
    def _scaled(known, scores):
        return backend.safe_div(known, backend.max(known)), backend.safe_div(scores, backend.max(scores))

    @staticmethod
    def _aks(s):
        return backend.safe_div(s[5], s[10] * s[9]), backend.safe_div(s[3], s[10]), backend.safe_div(s[1], s[9])


class TPR(_Rates):                                           # supervised.py:225-232
    """True positive rate (recall)."""

    def _value(self, known, scores):
        known, scores = self._scaled(known, scores)
        return backend.safe_div(backend.sum(known * scores), backend.sum(known))

    def _from_slots(self, s, eps):
        a, k, _ = self._aks(s)
        return backend.safe_div(a, k)


class TNR(_Rates):                                           # supervised.py:235-242
    """True negative rate."""

    def _value(self, known, scores):
        known, scores = self._scaled(known, scores)
        return backend.safe_div(backend.sum((1 - known) * (1 - scores)), backend.sum(1 - known))

    def _from_slots(self, s, eps):
        # sum (1 - k)(1 - s) = n - K - S + A over the divided sides: a difference of sums, well conditioned while the negatives
        # are not a vanishing share of the rows
        a, k, t = self._aks(s)
        return backend.safe_div(s[0] - k - t + a, s[0] - k)


class PPV(_Rates):                                           # supervised.py:245-252
    """Positive predictive value (precision)."""

    def _value(self, known, scores):
        known, scores = self._scaled(known, scores)
        return backend.safe_div(backend.sum(known * scores), backend.sum(scores))

    def _from_slots(self, s, eps):
        a, _, t = self._aks(s)
        return backend.safe_div(a, t)


class pRule(_ClosedForm):                                    # supervised.py:290-311
    """The ratio of the mean score of the sensitive nodes (the known scores, binary) and of the others, the smaller over the larger: 1
    is statistical parity, usually above 0.8 counts as fair."""

    @staticmethod
    def _ratio(p1, p2, sensitive, n):
        if p1 == 0 or p2 == 0:
            return 0
        p1 = abs(backend.safe_div(p1, sensitive))
        p2 = abs(backend.safe_div(p2, n - sensitive))
        if p1 <= p2:
            return p1 / p2
        return p2 / p1

    def _value(self, sensitive, scores):
        return self._ratio(backend.dot(scores, sensitive), backend.dot(scores, 1 - sensitive), backend.sum(sensitive),
                           backend.length(sensitive))

    def _from_slots(self, s, eps):
        return self._ratio(s[5], s[1] - s[5], s[3], s[0])


class L2Disparity(_ClosedForm):                              # supervised.py:314-333
    def __init__(self, *args, target_pRule=0.8, **kwargs):
        super().__init__(*args, **kwargs)
        self.target_pRule = target_pRule

    @staticmethod
    def _gap(p1, p2, sensitive, n):
        p1 = backend.safe_div(p1, sensitive / float(n))
        p2 = backend.safe_div(p2, 1. - sensitive / float(n))
        return abs(p1 - p2) ** 2

    def _value(self, sensitive, scores):
        return self._gap(backend.dot(scores, sensitive), backend.dot(scores, 1 - sensitive), backend.sum(sensitive),
                         backend.length(sensitive))

    def _from_slots(self, s, eps):
        return self._gap(s[5], s[1] - s[5], s[3], s[0])


class BinaryCrossEntropy(_ClosedForm):                       # supervised.py:157-166
    _GROUP = L.PAIR_LOGS

    def _value(self, known, scores):
        eps = backend.epsilon()
        return -backend.dot(known, backend.log(scores + eps)) - backend.dot(1 - known, backend.log(1 - scores + eps))

    def _from_slots(self, s, eps):
        return -s[12] - s[13]


class CrossEntropy(_ClosedForm):                             # supervised.py:169-175
    _GROUP = L.PAIR_LOGS

    def _value(self, known, scores):
        return -backend.sum(scores * backend.log(known))

    def _from_slots(self, s, eps):
        return -s[16]


class KLDivergence(_ClosedForm):                             # supervised.py:178-190
    """The KL divergence of the scores from the known scores, both shifted by epsilon and divided by their sums.  On the slab route,
    with S = sum (s + eps) and K = sum (k + eps):  sum ((s + eps) / S) log(((s + eps) / S) / ((k + eps) / K))
    = (sum (s + eps) log(s + eps) - sum (s + eps) log(k + eps)) / S - log S + log K."""
    _GROUP = L.PAIR_LOGS
    _NORMALIZE = True

    def _value(self, known, scores):
        eps = backend.epsilon()
        known = known + eps
        known = backend.safe_div(known, backend.sum(known))
        scores = scores + eps
        scores = backend.safe_div(scores, backend.sum(scores))
        return backend.sum(scores * backend.log(scores / known))

    @staticmethod
    def _kl(s, eps):
        import math
        total_s, total_k = s[1] + eps * s[0], s[3] + eps * s[0]
        if not (total_s > 0 and total_k > 0):
            return float("nan")
        return (s[14] - s[15]) / total_s - math.log(total_s) + math.log(total_k)

    def _from_slots(self, s, eps):
        return self._kl(s, eps)


class MKLDivergence(KLDivergence):                           # supervised.py:193-205
    """Minus the KL divergence over the number of evaluated nodes."""

    def _value(self, known, scores):
        eps = backend.epsilon()
        known = known + eps
        known = known / backend.sum(known)
        scores = scores + eps
        scores = scores / backend.sum(scores)
        return -backend.sum(scores * backend.log(scores / known)) / backend.length(scores)

    def _from_slots(self, s, eps):
        return _ieee_div(-self._kl(s, eps), s[0])


class PearsonCorrelation(_ClosedForm):                       # supervised.py:282-287 (scipy.stats.pearsonr in the reference)
    """The columns route is the centred two-pass form: the means first, then dots of the centred vectors.  Constant scores or known
    scores give nan, as scipy does."""

    def _value(self, known, scores):
        n = backend.length(scores)
        known = known - backend.sum(known) / n
        scores = scores - backend.sum(scores) / n
        return _ieee_div(backend.dot(known, scores), _ieee_sqrt(backend.dot(known, known) * backend.dot(scores, scores)))

    def _from_slots(self, s, eps):
        # the one-pass form n sum ks - sum k sum s over sqrt((n sum s^2 - (sum s)^2)(n sum k^2 - (sum k)^2)): each bracket is a difference
        # of two f64 numbers of the size of n sum s^2, so it loses digits when a column's variance is far below its squared mean (about
        # log10(mean^2 / variance) of the 16 an f64 sum holds); the columns route's centred form does not
        n = s[0]
        return _ieee_div(n * s[5] - s[1] * s[3], _ieee_sqrt((n * s[2] - s[1] * s[1]) * (n * s[4] - s[3] * s[3])))


class MannWhitneyParity(AUC):                                # supervised.py:336-350 (scipy.stats.mannwhitneyu in the reference)
    """1 - 2 |AUC - 0.5| with the sensitive nodes (known scores != 0) as the positives: 1 when a sensitive node is as likely to score
    above another node as below it, 0 when it always scores above or always below.  The reference's
    mannwhitneyu(x0, x1).statistic / (n0 n1) is 1 - AUC with ties at half, and the expression is the same for AUC and 1 - AUC.
    Raises when either class is empty, as AUC does."""
    _SAME_CLASS = "Cannot evaluate MannWhitneyParity when all nodes are in the same class"

    def _of_auc(self, auc):
        return 1 - 2 * abs(auc - 0.5)


class _RankPlan(EnginePlan):
    """What the columns of every NDCG / SpearmanCorrelation call share on the device (pgh_rank_plan_create, include/pgh_rank.h)."""
    _DESTROY = "pgh_rank_plan_destroy"

    def __init__(self, known, exclude):
        self._h = L.c_rank_plan()
        L.check(L.entry("pgh_rank_plan_create")(known._h, None if exclude is None else exclude._h, C.byref(self._h)))
        kept, relevant, negative = C.c_int64(), C.c_int64(), C.c_int32()
        L.check(L.entry("pgh_rank_plan_info")(self._h, C.byref(kept), C.byref(relevant), C.byref(negative)))
        self.num_kept, self.num_relevant, self.has_negative = kept.value, relevant.value, bool(negative.value)


class _Ranked(_Pairwise):
    """NDCG and SpearmanCorrelation: measures of a column's ORDER.  With the entries of include/pgh_rank.h ``evaluate`` scores a vector
    as the b = 1 case on its own storage and ``evaluate_many`` scores a slab 64 columns at a time, both through one plan per (known
    scores, exclude) pair: the plan is kept on the measure while ``known_scores`` and ``exclude`` are the same objects (and the graph
    and the number of rows are the same).  On a library without the entries -- or when the entry declines, or with known scores or
    exclude values per column -- every column takes ``_columns_value``: backend primitives over the filtered vectors."""
    _ENTRIES = ()
    _plan_cache = None
    _MANY_IS_EXACT = True         # evaluate is the one-column case of the same entry, whose per-column result does not depend on the width

    def _slab_available(self):
        return all(L.entry(name) is not None for name in ("pgh_rank_plan_create", "pgh_rank_plan_info", "pgh_rank_plan_destroy")
                   + self._ENTRIES)

    def _plan_for(self, anchor, rows):
        graph = None if anchor is None else anchor.graph
        cached = self._plan_cache
        if cached is not None and cached[0] is self.known_scores and cached[1] is self.exclude and cached[2] is graph and cached[3] == rows:
            return cached[4]
        known, _ = self._operand(anchor, self.known_scores, rows, "known scores")
        exclude, _ = self._operand(anchor, self.exclude, rows, "exclude values")
        plan = _RankPlan(known, exclude)
        self._plan_cache = (self.known_scores, self.exclude, graph, rows, plan)
        return plan

    def _of_entry(self, handle, plan, width, vector):
        """The values of `width` columns behind `handle` (a slab, or with `vector` a vector's own storage); None when declined."""
        raise NotImplementedError

    def _columns_value(self, known, scores):
        raise NotImplementedError

    def _slab(self, anchor, columns, count):
        if isinstance(self.known_scores, DeviceMatrix) or isinstance(self.exclude, DeviceMatrix):
            return None                                      # known scores per column: one plan per column, no shared pass
        matrix = self._matrix(anchor, columns)
        plan = self._plan_for(anchor, matrix.n)
        out = []
        for _, part in matrix.chunks():
            values = self._of_entry(part._h, plan, part.b, False)
            if values is None:
                return None
            out.extend(values)
        return out

    def evaluate(self, scores):
        if _FORCE_PER_COLUMN or not self._slab_available() or isinstance(self.known_scores, DeviceMatrix) \
                or isinstance(self.exclude, DeviceMatrix):
            return self._columns_value(*self._pair(scores))
        known = self.known_scores
        if all(isinstance(value, numbers.Number) for value in (scores, known)):
            anchor, vector = None, backend.to_array([scores])
        else:
            anchor = next((value for value in (scores, known) if isinstance(value, GraphSignal)), None)
            if anchor is None and self.exclude is not None:
                raise Exception("Needs to parse graph signal scores or known_scores to be able to exclude specific nodes")
            vector = self._dense(anchor, scores)
        vector._h                           # noqa: B018 -- an unevaluated expression (device.LazyVector) is evaluated first
        values = self._of_entry(vector._h, self._plan_for(anchor, len(vector)), 1, True)
        if values is None:
            return self._columns_value(*self._pair(scores))
        return values[0]


class NDCG(_Ranked):                                         # supervised.py:68-90
    """NDCG@k of the scores against the known scores: the known scores of the first k nodes in descending order of score (ties in node
    order, as Python's stable sort leaves them), each divided by log2(position + 1), over the same sum in descending order of the
    known scores.  k is the number of known scores when None, is not reduced by the exclusion, and a k above that number raises.
    The quotient is the reference's: nan for 0 / 0 (no relevant node among the evaluated ones), and ZeroDivisionError when no node is
    evaluated at all (both sums are then Python's integer 0).

    With include/pgh_rank.h the DCG of up to 64 columns is one streaming pass over the slab.  The columns route
    is filter_out, DeviceVector.ordinals() and one masked sum in f32."""
    _ENTRIES = ("pgh_ndcg", "pgh_ndcg_vec")

    def __init__(self, known_scores, exclude=None, k=None):
        super().__init__(known_scores, exclude=exclude)
        if k is not None and k > len(known_scores):
            raise Exception("NDCG@k cannot be computed for k greater than the number of known scores")
        self.k = len(known_scores) if k is None else k

    def best_direction(self):
        return 1

    @staticmethod
    def _quotient(dcg, idcg, evaluated, k):
        if evaluated == 0 or k < 1:
            raise ZeroDivisionError("division by zero")      # the reference divides the integer 0 by the integer 0 here
        return _ieee_div(dcg, idcg)

    def _of_entry(self, handle, plan, width, vector):
        k = int(self.k)
        if plan.num_kept == 0 or k < 1:
            self._quotient(0, 0, 0, k)
        dcg, idcg = (C.c_double * width)(), C.c_double()
        status = L.entry("pgh_ndcg_vec" if vector else "pgh_ndcg")(handle, plan._h, k, L.RANK_AUTO, dcg, C.byref(idcg))
        if not L.accepted(status):
            return None
        return [self._quotient(float(v), idcg.value, plan.num_kept, k) for v in dcg]

    def _columns_value(self, known, scores):
        import math
        k = int(self.k)

        def gain(order_of):
            ordinals = order_of.ordinals()
            return backend.sum(known * (ordinals <= k) / (backend.log(ordinals + 1) / math.log(2)))
        if len(scores) == 0 or k < 1:
            self._quotient(0, 0, 0, k)
        return self._quotient(gain(scores), gain(known), len(scores), k)


class SpearmanCorrelation(_Ranked):                          # supervised.py:274-279 (scipy.stats.spearmanr in the reference)
    """Spearman's rho of the scores and the known scores over the evaluated nodes: Pearson's correlation of their mid-ranks, in the
    centred form (sum of products of 2 rank - (n + 1), exact integers).  Constant scores or known scores give nan, as scipy does.

    With include/pgh_rank.h a column costs one device radix sort.  The columns route is the fallback of a
    library WITHOUT that entry: the two filtered vectors are downloaded and ranked on the host with numpy."""
    _ENTRIES = ("pgh_spearman", "pgh_spearman_vec")

    def best_direction(self):
        return 1

    def _of_entry(self, handle, plan, width, vector):
        rho = (C.c_double * width)()
        status = L.entry("pgh_spearman_vec" if vector else "pgh_spearman")(handle, plan._h, rho)
        if not L.accepted(status):
            return None
        return [float(v) for v in rho]

    @staticmethod
    def _centred_ranks(values):
        """2 midrank - (n + 1) of every entry, exact integers held in f64."""
        import numpy as np
        _, inverse, counts = np.unique(values, return_inverse=True, return_counts=True)
        upto = np.cumsum(counts)
        return ((2 * upto - counts)[inverse.reshape(-1)] - len(values)).astype(np.float64)

    def _columns_value(self, known, scores):
        import numpy as np
        known, scores = np.asarray(known, dtype=np.float64), np.asarray(scores, dtype=np.float64)
        if np.isnan(scores).any() or np.isnan(known).any():
            return float("nan")
        dk, ds = self._centred_ranks(known), self._centred_ranks(scores)
        return _ieee_div(float(np.dot(ds, dk)), _ieee_sqrt(float(np.dot(ds, ds)) * float(np.dot(dk, dk))))


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
        stats_fn, forms_fn = L.entry("pgh_mat_col_stats"), L.entry("pgh_cut_forms")
        import numpy as np
        out = []
        for _, part in matrix.chunks():
            stats = np.empty((part.b, 4), dtype=np.float64)
            L.check(stats_fn(part._h, stats.ctypes.data_as(C.c_void_p)))
            factors = self._plan(stats)
            forms = np.empty((part.b, 4), dtype=np.float64)
            status = forms_fn(device_graph._h, part._h, None if factors is None else factors.ctypes.data_as(C.c_void_p),
                              float(getattr(self, "max_rank", 1)), self._FORMS, forms.ctypes.data_as(C.c_void_p))
            if not L.accepted(status):
                return None
            out.extend(self._from_forms(graph, [float(v) for v in forms[j]], [float(v) for v in stats[j]]) for j in range(part.b))
        return out

    def _route(self, graph, adjacency, columns):
        """Scores of `columns` (a DeviceMatrix or a list of vectors) on the preprocessed graph."""
        device_graph = getattr(adjacency, "array", adjacency)
        if not _FORCE_PER_COLUMN and isinstance(device_graph, DeviceGraph) and L.entry("pgh_cut_forms") is not None \
                and L.entry("pgh_mat_col_stats") is not None:
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


class Modularity(Unsupervised):
    """unsupervised.py:148-201: modularity of the fuzzy subgraph the scores describe, over a sample of the nodes.  With c_v the
    multiplicity of v in the sample (all ones while the graph has at most max_positive_samples nodes; else the sample is
    ``RandomState(seed).choice(n, max_positive_samples)``, a private generator where the reference reseeds numpy's global one) and
    w = c * scores / max_rank,

        Q = (w^T P w - (sum_v w_v d_v)^2 / 2m) / 2m

    P the 0/1 pattern of the adjacency (``has_edge``), d = ``graph.degree`` and m = ``number_of_edges()`` with networkx's conventions
    (in + out degree on a directed graph; on an undirected one a self-loop counts twice in the degree and once in m); m = 0 gives 0.
    This closed form REPLACES the reference's O(samples^2) loop over ``has_edge``: the same sum, regrouped.  w^T P w is pgh_cut_forms
    (PGH_CUT_INTERNAL) on the graph diag(c) P diag(c), sum w d the <known, scores> slot of pgh_pair_forms against c * d: up to 64
    columns share both passes (``evaluate_many``).  fused=False, a library without the entries or a decline evaluates the same closed
    form column by column with backend primitives (conv and dot)."""

    def __init__(self, graph=None, max_rank=1, max_positive_samples=2000, seed=0, progress=lambda x: x, fused=True):
        self.graph = graph
        self.max_positive_samples = max_positive_samples
        self.max_rank = max_rank
        self.seed = seed
        self.progress = progress                             # kept for the reference's signature: there is no loop to wrap
        self.fused = fused
        self.last_route = None
        self._prepared = None

    def _prepare(self, graph):
        """Per graph: 2m, the device graph diag(c) P diag(c) and the vector c * d."""
        import numpy as np
        import scipy.sparse as sp
        from pygrank_amd import multigroup
        cached = self._prepared
        if cached is not None and cached["of"] is graph and self.seed is not None:
            return cached
        taken, P = multigroup.pattern(graph)
        n = P.shape[0]
        out_degree = np.diff(P.indptr).astype(np.int64)
        if taken.is_directed():
            degree = out_degree + np.bincount(P.indices, minlength=n).astype(np.int64)
            edges = int(P.nnz)
        else:
            loops = P.diagonal().astype(np.int64)
            degree = out_degree + loops
            edges = (int(P.nnz) + int(loops.sum())) // 2
        prepared = dict(of=graph, edges=edges, graph=None, weighted_degree=None)
        if edges != 0:
            candidates, _ = multigroup.sample(n, self.max_positive_samples, self.seed)
            counts = np.bincount(candidates, minlength=n).astype(np.float64)
            scale = sp.dia_array((counts[None, :], [0]), shape=(n, n))
            M = sp.csr_array(scale @ P.astype(np.float64) @ scale)
            M.eliminate_zeros()
            prepared["graph"] = backend.scipy_sparse_to_backend(M)
            prepared["weighted_degree"] = backend.to_array(counts * degree)
        self._prepared = prepared
        return prepared

    def _value(self, prepared, internal, weighted):
        m = prepared["edges"]
        return (internal - weighted * weighted / 2 / m) / 2 / m

    def _slab(self, prepared, matrix):
        import numpy as np
        forms_fn, pair_fn = L.entry("pgh_cut_forms"), L.entry("pgh_pair_forms")
        out = []
        for _, part in matrix.chunks():
            factors = np.full(part.b, 1.0 / self.max_rank, dtype=np.float64)
            forms = np.empty((part.b, 4), dtype=np.float64)
            status = forms_fn(prepared["graph"]._h, part._h, factors.ctypes.data_as(C.c_void_p), 1.0, L.CUT_INTERNAL,
                              forms.ctypes.data_as(C.c_void_p))
            if not L.accepted(status):
                return None
            slots = np.empty((part.b, L.PAIR_SLOTS), dtype=np.float64)
            status = pair_fn(part._h, prepared["weighted_degree"]._h, None, None, None, None, backend.epsilon(), L.PAIR_MOMENTS,
                             slots.ctypes.data_as(C.c_void_p))
            if not L.accepted(status):
                return None
            out.extend(self._value(prepared, float(forms[j][0]), float(slots[j][5]) / self.max_rank) for j in range(part.b))
        return out

    def _one(self, prepared, scores):
        w = scores / self.max_rank if self.max_rank != 1 else scores
        return self._value(prepared, backend.dot(backend.conv(w, prepared["graph"]), w), backend.dot(w, prepared["weighted_degree"]))

    def _route(self, graph, columns):
        prepared = self._prepare(graph)
        count = columns.b if isinstance(columns, DeviceMatrix) else len(columns)
        if prepared["edges"] == 0:
            return [0] * count
        if self.fused and not _FORCE_PER_COLUMN and isinstance(prepared["graph"], DeviceGraph) \
                and L.entry("pgh_cut_forms") is not None and L.entry("pgh_pair_forms") is not None:
            matrix = columns if isinstance(columns, DeviceMatrix) else DeviceMatrix.from_columns(columns)
            out = self._slab(prepared, matrix)
            if out is not None:
                self.last_route = "slab"
                return out
        self.last_route = "columns"
        vectors = columns.columns() if isinstance(columns, DeviceMatrix) else columns
        for vector in vectors:
            vector._h                       # noqa: B018 -- an unevaluated expression (device.LazyVector) is evaluated first
        return [self._one(prepared, vector) for vector in vectors]

    def evaluate(self, scores):
        scores = to_signal(self.graph, scores)
        return self._route(scores.graph, [scores.np])[0]

    def evaluate_many(self, columns):
        """What evaluate returns for every column, as a list: `columns` is a DeviceMatrix over the measure's graph, or a list of graph
        signals / score vectors of one graph.  On the slab route up to 64 columns share the two passes."""
        if isinstance(columns, DeviceMatrix):
            if self.graph is None:
                raise Exception("a slab of score columns can only be evaluated by a measure that was given its graph")
            graph = self.graph.graph if isinstance(self.graph, GraphSignal) else self.graph
            if columns.n != len(graph):
                raise Exception(f"a slab of {columns.n} rows cannot hold scores of {len(graph)} nodes")
            return self._route(graph, columns)
        signals = [to_signal(self.graph, column) for column in columns]
        if not signals:
            return []
        graph = signals[0].graph
        if any(signal.graph is not graph for signal in signals):
            raise Exception("the score columns belong to different graphs")
        return self._route(graph, [signal.np for signal in signals])


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


from pygrank_amd.combination import AM, GM, Disparity, MeasureCombination, Parity  # noqa: E402,F401 -- re-exported; it imports Measure from here
