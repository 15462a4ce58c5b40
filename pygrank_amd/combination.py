"""Combinations of measures: restates pygrank/measures/combination.py:7-137 (MeasureCombination, AM, GM, Disparity, Parity).

A combination bounds every member's value by that member's thresholds and folds the bounded values with the members' weights.  All of
it is scalar f64 arithmetic on the host, what the reference's numpy backend computes; members of weight 0 are not evaluated at all.

Beyond the reference every combination has ``evaluate_many(columns)``.  It equals ``[evaluate(c) for c in columns]`` TO THE BIT: the
members' values are folded per column by the very code ``evaluate`` runs on one column, and a member's own ``evaluate_many`` is called
-- once, for all columns -- only where that member declares it bit-equal to its ``evaluate`` (``_MANY_IS_EXACT``: AUC,
MannWhitneyParity, NDCG, SpearmanCorrelation, whose slab passes count integers, and combinations themselves).  The closed-form measures
do not: on the engine ``pgh_pair_forms`` sums a column's rows in an order that depends on the slab's width (and ``Cos.evaluate`` is
three ``pgh_dot`` reductions), so their two entry points agree to a tolerance, not to the bit; such members are
evaluated column by column.  ``evaluate_many(columns, exact=False)`` gives that up: EVERY member's ``evaluate_many`` is called once --
a combination of AUC and pRule over 64 columns then costs the members' slab passes, not 128 evaluations -- and a value may differ from
``evaluate`` in the last bits, as the members' do.  ``last_batched`` lists the positions of the members the last call scored in one pass.
"""
import math

import numpy as np

from pygrank_amd import backend
from pygrank_amd.measures import Measure


def _differentiable_hinge(x, gamma=30):
    """combination.py:7-11 (doi:10.1088/1742-6596/1743/1/012025, p. 4), in f64 with numpy's overflow rules (exp may return inf)."""
    with np.errstate(all="ignore"):
        x = np.float64(x)
        return float(x + np.log(1 + np.exp(-x * gamma)) / gamma)


class MeasureCombination(Measure):
    """combination.py:14-81.  Measures given to the constructor are bounded to (0, 1) unless thresholds are given; measures that are
    added with ``add`` are unbounded unless min_val / max_val are given."""

    def __init__(self, measures=None, weights=None, thresholds=None, differentiable=False):
        self.measures = list() if measures is None else measures
        self.weights = [1. for _ in self.measures] if weights is None else weights
        self.thresholds = [(0., 1.) for _ in self.measures] if thresholds is None else thresholds
        self.differentiable = differentiable

    def add(self, measure, weight=1., min_val=-float('inf'), max_val=float('inf')):
        self.measures.append(measure)
        self.weights.append(weight)
        self.thresholds.append((min_val, max_val))
        return self

    def _total_weight(self):
        return float(sum(abs(float(weight)) for weight in self.weights))

    def max(self, x, constant):
        if self.differentiable and not math.isinf(constant):
            return _differentiable_hinge(x - constant) + constant
        return max(x, constant)

    def min(self, x, constant):
        if self.differentiable and not math.isinf(constant):
            return constant - _differentiable_hinge(constant - x)
        return min(x, constant)

    # ---- one column and many
    def _active(self):
        """Positions of the members that are evaluated: those of non-zero weight."""
        return [i for i in range(len(self.measures)) if self.weights[i] != 0]

    def _bounded(self, i, value):
        return self.min(self.max(value, self.thresholds[i][0]), self.thresholds[i][1])

    def _fold(self, values):
        """The combination of one column from {member position: its value} over the active members."""
        raise Exception("Non-abstract subclasses of MeasureCombination should implement a _fold method")

    def evaluate(self, scores):
        return self._fold({i: self.measures[i].evaluate(scores) for i in self._active()})

    _MANY_IS_EXACT = True         # evaluate_many(columns) equals a loop over evaluate to the bit (with exact=True, the default)
    last_batched = None           # positions of the members whose evaluate_many the last evaluate_many called

    def evaluate_many(self, columns, exact=True):
        """What evaluate returns for every column, as a list: `columns` is what the members' evaluate_many take (a DeviceMatrix, or a list
        of graph signals or score vectors of one graph).  exact=True (default): to the bit -- a member is scored in one pass over all
        columns when it declares that pass bit-equal to its evaluate, else column by column.  exact=False: every member that has an
        evaluate_many is scored in one pass; the values are then as close to evaluate's as the members' two entry points are."""
        from pygrank_amd.device import DeviceMatrix
        if not isinstance(columns, DeviceMatrix):
            columns = list(columns)
            if not columns:
                return []
        count = columns.b if isinstance(columns, DeviceMatrix) else len(columns)
        vectors = None
        values = {}
        self.last_batched = []
        for i in self._active():
            member = self.measures[i]
            many = getattr(member, "evaluate_many", None)
            if many is not None and (not exact or getattr(member, "_MANY_IS_EXACT", False)):
                values[i] = many(columns, exact=exact) if isinstance(member, MeasureCombination) else many(columns)
                self.last_batched.append(i)
            else:
                if vectors is None:
                    vectors = columns.columns() if isinstance(columns, DeviceMatrix) else columns
                values[i] = [member.evaluate(vector) for vector in vectors]
        return [self._fold({i: values[i][j] for i in values}) for j in range(count)]


class AM(MeasureCombination):                                # combination.py:84-94
    """The weighted arithmetic mean of the bounded values."""

    def _fold(self, values):
        result = 0
        for i, value in values.items():
            result += self.weights[i] * self._bounded(i, value)
        total = self._total_weight()
        if total == 0:
            return float("nan") if result == 0 or result != result else math.copysign(float("inf"), result)
        return result / total


class _Alternating(MeasureCombination):
    def _signed_sum(self, values):
        result = 0
        for i, value in values.items():
            result += (self.weights[i] * (1 if i % 2 == 0 else -1)) * self._bounded(i, value)
        return result if result > 0 else -result


class Disparity(_Alternating):                               # combination.py:97-109
    """abs(M1 - M2 + M3 - M4 ...) of the weighted bounded values; the sign alternates with the member's position, whether or not a
    member of weight 0 is skipped."""

    def _fold(self, values):
        return self._signed_sum(values)


class Parity(_Alternating):                                  # combination.py:112-124
    """1 - abs(M1 - M2 + M3 - M4 ...) of the weighted bounded values."""

    def _fold(self, values):
        return 1 - self._signed_sum(values)


class GM(MeasureCombination):                                # combination.py:127-137
    """The weighted geometric mean of the bounded values, none taken below epsilon."""

    def _fold(self, values):
        result = 0
        with np.errstate(all="ignore"):
            for i, value in values.items():
                result += self.weights[i] * float(np.log(np.float64(self.max(backend.epsilon(), self._bounded(i, value)))))
            return float(np.exp(np.float64(result) / np.float64(self._total_weight())))
