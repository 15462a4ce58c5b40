"""Fairness-aware postprocessors: FairPersonalizer [krasanakis2020prioredit] and AdHocFairness [tsioutsiouliklis2020fairness].

Restates pygrank/algorithms/postprocess/fairness.py:10-141 (``FairPersonalizer``) and :147-217 (``AdHocFairness``).

FairPersonalizer searches a prior-editing model of 4 * buckets + 1 parameters with ``optimize``; every candidate costs one run of the
base ranker at a fixed iteration count and two supervised measures.  A coordinate step's candidates share graph, ranker and iteration
count, so the loss handed to ``optimize`` has a ``many``: one kernel writes every candidate's edited prior into one [n, probes] slab
(include/pgh_fair.h: pgh_prior_edit), ``propagate`` runs the slab through the ranker's multi-seed loop where it has
one, and ``evaluate_many`` scores the columns in one pass each.  On a library without the entry -- the host test double -- the columns
are built one candidate at a time from backend operations and still ranked and scored together.

``FairWalk`` and AdHocFairness's method "O" stay out of scope.
"""
import ctypes as C

import numpy as np

from pygrank_amd import _lib as L
from pygrank_amd import backend
from pygrank_amd.autotune import optimize
from pygrank_amd.convergence import ConvergenceManager
from pygrank_amd.device import DeviceMatrix
from pygrank_amd.measures import Mabs, MannWhitneyParity, pRule
from pygrank_amd.postprocess import Postprocessor, Tautology
from pygrank_amd.signals import to_signal

_NEEDS_MISTREATMENT = ("TPR", "TNR", "mistreatment")


class _EditLoss:
    """FairPersonalizer's loss (fairness.py:123-132) with the ranker's convergence manager swapped for a fixed iteration count while it
    is open; ``close`` puts the original manager back.

    ``loss(params)`` is the reference's pipeline one candidate at a time: the edited prior composed from backend operations, one
    ``ranker.rank`` and the two measures.  ``loss.many(candidates)`` does the same for a coordinate step's candidates together, 64 at a
    time: pgh_prior_edit writes their edited priors into a slab (or, where the library lacks the entry or the entry declines, the
    columns are composed one by one), ``ranker.propagate`` ranks the slab and ``evaluate_many`` scores its columns."""

    def __init__(self, owner, graph, training, sensitive, fairness_measure, original_ranks, args, kwargs):
        self.owner, self.graph, self.training, self.sensitive = owner, graph, training, sensitive
        self.fairness_measure, self.original_ranks, self.args, self.kwargs = fairness_measure, original_ranks, args, kwargs
        # fixed while the loss is open: the error measure against the original scores and the scores' maximum (one reduction)
        self.error = owner.error_type(original_ranks, exclude=None if owner.fix_personalization else training)
        self.rank_max = backend.max(original_ranks.np)
        ranker = owner.ranker
        self._previous = ranker.convergence
        ranker.convergence = ConvergenceManager(error_type="iters", max_iters=self._previous.iteration)
        self._open = True
        if owner.batch:
            self.many = self._many

    def close(self):
        if self._open:
            self.owner.ranker.convergence = self._previous
            self._open = False

    def _combine(self, error, direction, fairness):
        owner = self.owner
        return - owner.retain_rank_weight * error * direction - owner.pRule_weight * min(owner.target_pRule, fairness)

    def edit(self, params):
        """fairness.py:78-93 term for term on backend vectors."""
        owner = self.owner
        personalization, sensitive = self.training.np, self.sensitive.np
        ranks = self.original_ranks.np / self.rank_max
        res = ranks if owner.parameter_buckets == 0 else 0
        for i in range(owner.parameter_buckets):
            a = sensitive * (params[0 + 4 * i] - params[1 + 4 * i]) + params[1 + 4 * i]
            b = sensitive * (params[2 + 4 * i] - params[3 + 4 * i]) + params[3 + 4 * i]
            d = ranks - personalization
            if not owner.error_skewing:
                d = backend.abs(d)
            res = res + (1 - a) * backend.exp(b * d) + a * backend.exp(-b * d)
        return (1.0 - params[-1]) * res + personalization * params[-1]

    def __call__(self, params):
        self.owner.last_fit["single_steps"] += 1
        fair_ranks = self.owner.ranker.rank(self.graph, self.edit(params), *self.args, **self.kwargs)
        fairness = self.fairness_measure(fair_ranks)
        return self._combine(self.error(fair_ranks), self.error.best_direction(), fairness)

    def _slab(self, chunk):
        """The chunk's edited priors through pgh_prior_edit, or None when the library lacks the entry or the entry declines."""
        entry = L.entry("pgh_prior_edit")
        if entry is None:
            return None
        owner = self.owner
        buckets, probes = int(owner.parameter_buckets), len(chunk)
        flat = np.ascontiguousarray(chunk, dtype=np.float64)
        if flat.shape != (probes, 4 * buckets + 1):
            return None
        personalization, sensitive, ranks = self.training.np, self.sensitive.np, self.original_ranks.np
        out = DeviceMatrix.empty(len(personalization), probes)
        status = entry(personalization._h, sensitive._h, ranks._h, float(self.rank_max), flat.ctypes.data_as(C.c_void_p), buckets, probes,
                       1 if owner.error_skewing else 0, out._h)
        if not L.accepted(status):
            return None
        return out

    def _many(self, candidates):
        candidates = [list(params) for params in candidates]
        owner, stats = self.owner, self.owner.last_fit
        losses = []
        for start in range(0, len(candidates), 64):
            chunk = candidates[start:start + 64]
            slab = self._slab(chunk)
            if slab is not None:
                stats["edit_kernel_steps"] += 1
            else:
                slab = DeviceMatrix.from_columns([backend.to_array(self.edit(params)) for params in chunk])
            stats["batched_steps"] += 1
            ranks = owner.ranker.propagate(self.graph, slab, *self.args, **self.kwargs)
            fairness = self.fairness_measure.evaluate_many(ranks)
            direction = self.error.best_direction()
            losses.extend(self._combine(e, direction, f) for e, f in zip(self.error.evaluate_many(ranks), fairness))
        return losses


class FairPersonalizer(Postprocessor):
    """fairness.py:10-141: edits the personalization so that the base ranker's outcome trades
    ``retain_rank_weight * error_type(original scores, edited scores)`` against ``pRule_weight * min(fairness, target_pRule)``.

    ranker: the base ranking algorithm (its ``convergence`` is replaced by a fixed iteration count while the search runs and is the
        original object again afterwards, also when the search raises).
    target_pRule: fairness above this value is not rewarded further.
    retain_rank_weight, pRule_weight: the two weights of the loss (pRule_weight=10 puts most of the emphasis on fairness).
    error_type: known scores, exclude -> supervised measure of the deviation from the original scores (default Mabs).
    parameter_buckets: sets of four parameters of the editing model (the engine's edit kernel serves up to 4).
    max_residual: upper limit of the share of the original personalization that is kept.
    error_skewing: edit by the signed difference between original scores and personalization instead of its absolute value.
    parity_type: "impact" (pRule) or "U" (MannWhitneyParity).  "TPR", "TNR" and "mistreatment" raise NotImplementedError: they are
        built on ``Mistreatment``, which is not yet in this package -- and which the reference constructs on ``validation = None``
        (fairness.py:101,107-113), so they cannot run there either.  Any other string raises the reference's exception.
    fix_personalization: False excludes the personalization's nodes from the error measure (fairness.py:129; the fairness measure is
        built before the reference assigns its `training`, so it never excludes any node).
    batch: False keeps ``many`` off the loss: every candidate takes the reference's route, one at a time.
    verbose: ``optimize`` reports its progress (the reference's default).

    After a run ``last_params`` holds the optimal edit and ``last_fit`` how the candidates were evaluated: ``batched_steps`` slabs went
    through ``propagate``, ``edit_kernel_steps`` of them were written by pgh_prior_edit, ``single_steps`` candidates went one by one."""

    def __init__(self, ranker, target_pRule=1, retain_rank_weight=1, pRule_weight=1, error_type=Mabs, parameter_buckets=1,
                 max_residual=0, error_skewing=False, parity_type="impact", fix_personalization=True, batch=True, verbose=True):
        super().__init__(ranker)
        self.target_pRule = target_pRule
        self.retain_rank_weight = retain_rank_weight
        self.pRule_weight = pRule_weight
        self.error_type = error_type
        self.parameter_buckets = parameter_buckets
        self.max_residual = max_residual
        self.error_skewing = error_skewing
        self.parity_type = parity_type
        self.fix_personalization = fix_personalization
        self.batch = batch
        self.verbose = verbose
        self.last_params = None
        self.last_fit = dict(batched_steps=0, single_steps=0, edit_kernel_steps=0)

    def _fairness_measure(self, sensitive):
        if self.parity_type == "impact":
            return pRule(sensitive, exclude=None)
        if self.parity_type == "U":
            return MannWhitneyParity(sensitive, exclude=None)
        if self.parity_type in _NEEDS_MISTREATMENT:
            raise NotImplementedError("parity_type " + self.parity_type + " is built on Mistreatment, which is not yet in this package")
        raise Exception("Invalid parity type " + str(self.parity_type) + ": expected impact, TPR, TNR or mistreatment")

    def _open(self, graph, personalization, sensitive, args, kwargs):
        """The loss of one (graph, personalization, sensitive) triple: runs the base ranker once for the original scores and swaps its
        convergence manager; the caller closes the loss."""
        personalization = to_signal(graph, personalization)
        sensitive = to_signal(personalization, sensitive)
        fairness_measure = self._fairness_measure(sensitive)
        graph = personalization.graph
        original_ranks = self.ranker.rank(graph, personalization, *args, **kwargs)
        return _EditLoss(self, graph, personalization, sensitive, fairness_measure, original_ranks, args, kwargs)

    def rank(self, graph, personalization, sensitive, *args, **kwargs):
        self.last_fit = dict(batched_steps=0, single_steps=0, edit_kernel_steps=0)
        loss = self._open(graph, personalization, sensitive, args, kwargs)
        try:
            buckets = self.parameter_buckets
            self.last_params = optimize(loss, max_vals=[1, 1, 5, 5] * buckets + [self.max_residual],
                                        min_vals=[0, 0, -5, -5] * buckets + [0], deviation_tol=1.E-6, divide_range=2, partitions=10,
                                        verbose=self.verbose)
            return self.ranker.rank(loss.graph, loss.edit(self.last_params), *args, **kwargs)
        finally:
            loss.close()

    def _reference(self):
        return "fair prior editing \\cite{krasanakis2020prioredit} for disparate " + self.parity_type + " mitigation"


class AdHocFairness(Postprocessor):
    """fairness.py:147-217: rescales the scores of the sensitive and of the other nodes so that each group's share of the total
    becomes its share of the nodes (method "B" or "mult" [tsioutsiouliklis2020fairness]): device vectors, two reductions and
    ``safe_div``.  ``AdHocFairness("B", ranker)`` and ``AdHocFairness(ranker, "B")`` are the same thing (fairness.py:168-171).

    Methods "O" / "LFPRO" raise NotImplementedError: the reference's redistribution is a sequential water-filling over Python
    dictionaries, whose faithful device form is a sort-based kernel of its own.  Any other method raises the reference's exception.
    ``eps`` is the reference's stopping threshold of that redistribution; it is kept for the signature and unused by "B" / "mult"."""

    def __init__(self, ranker=None, method="B", eps=1.E-12):
        if ranker is not None and not callable(getattr(ranker, "rank", None)):
            ranker, method = method, ranker
            if not callable(getattr(ranker, "rank", None)):
                ranker = None
        super().__init__(Tautology() if ranker is None else ranker)
        self.method = method
        self.eps = eps

    def _transform(self, ranks, sensitive):
        sensitive = to_signal(ranks, sensitive)
        if self.method in ("O", "LFPRO"):
            raise NotImplementedError("AdHocFairness method " + self.method + " (LFPRO water-filling) is not in this package")
        if self.method not in ("B", "mult"):
            raise Exception("Invalid fairness postprocessing method " + str(self.method))
        phi = backend.sum(sensitive.np) / backend.length(sensitive.np)
        sum_r = backend.sum((ranks * sensitive).np)
        sum_b = backend.sum((ranks * (1 - sensitive)).np)
        sum_total = sum_r + sum_b
        sum_r = backend.safe_div(sum_r, sum_total)
        sum_b = backend.safe_div(sum_b, sum_total)
        return ranks * sensitive * backend.safe_div(phi, sum_r) + ranks * (1 - sensitive) * backend.safe_div(1 - phi, sum_b)

    def _reference(self):
        return "LFPRO fairness \\cite{tsioutsiouliklis2020fairness}" if self.method in ("O", "LFPRO") \
            else "multiplicative fairness \\cite{tsioutsiouliklis2020fairness}"
