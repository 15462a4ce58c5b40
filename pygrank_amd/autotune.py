"""Parameter tuning: the coordinate descent of [krasanakis2022autogf], the tuner built on it and the selection among ready filters.

Restates pygrank/algorithms/autotune/optimization.py:9-25,64-212 (``optimize``), autotune/tuning.py:5-23 (``Tuner``),
autotune/parameterized.py:9-177 (``default_tuning_optimization``, ``SelfClearDict``, ``ParameterTuner``),
autotune/selection.py:10-91 (``AlgorithmSelection``) and autotune/hop_tuner.py:14-184 (``HopTuner``).

One addition to the reference.  A coordinate step of ``optimize`` scores ``partitions`` candidates that differ in ONE weight.  When
the loss object has a callable attribute ``many`` the step hands it the whole candidate list in one call.  ``ParameterTuner`` builds
such a loss for its default setting (GenericGraphFilter over stored powers, measure AUC): the candidates of a step share the power
slab of the training personalization (filters._PowerSlab), and ``pgh_probe_auc`` (include/pgh_tune.h) scores all of them in one
streaming pass over it -- no [n, P] ranks, no normalisation, no compaction and no sort of n pairs per candidate.
"""
import ctypes as C
import sys
from collections.abc import Iterable
from math import log
from random import random

import numpy as np

from pygrank_amd import _lib as L
from pygrank_amd.measures import AUC, Cos, _ProbePlan, split
from pygrank_amd.preprocessing import preprocessor
from pygrank_amd.signals import NodeRanking, to_signal
from pygrank_amd.utils import ensure_used_args, remove_used_args


def _log(text=""):
    """pygrank/core/utils/__init__.py log(): progress on one console line."""
    sys.stdout.write("\r" + text)
    sys.stdout.flush()


def _add(weights, index, increment, max_val, min_val, coarse=0):
    """optimization.py:9-25: a copy of `weights` with `increment` added at `index`, clipped to [min_val, max_val] and (coarse != 0)
    snapped to multiples of `coarse`."""
    weights = [weight for weight in weights]
    weights[index] = min(max_val, max(min_val, weights[index] + increment))
    if coarse != 0:
        weights[index] = round(weights[index] / coarse) * coarse
    return weights


def optimize(loss, max_vals=[1 for _ in range(1)], min_vals=None, deviation_tol=1.E-9, divide_range=1.01, partitions=5,
             parameter_tol=float('inf'), depth=1, coarse=0, shrink_strategy="divide", partition_strategy="split", randomize=False,
             weights=None, verbose=True, validation_loss=None):
    """optimization.py:64-212: coordinate descent over the box [min_vals, max_vals].  Every step shrinks the search range of the
    current variable ("divide": by divide_range; "shrinking": (max - min) / ((iter + 1)^divide_range log(iter + 2))), scores the
    candidates of that variable ("split": `partitions` points across the range; "step": multiples of `partitions` inside it), moves to
    the FIRST candidate of least loss and goes to the next variable (a random one with `randomize`), until the loss moved by at
    most deviation_tol over a whole round and every range is at most parameter_tol.  `validation_loss` picks the returned weights among
    the visited ones; `depth` > 1 restarts from the result with fresh ranges; `weights` is the starting point (default: the centre).

    `loss.many(candidate_weights) -> [losses]`, when the loss object has it, is called once per step instead of `loss` once per
    candidate; it must return what ``[loss(w) for w in candidate_weights]`` would."""
    if min_vals is None:
        min_vals = [0 for _ in max_vals]
    for min_val, max_val in zip(min_vals, max_vals):
        if min_val > max_val:
            raise Exception("Empty parameter range [" + str(min_val) + "," + str(max_val) + "]")
    if str(divide_range) != "shrinking" and divide_range <= 1:
        raise Exception("divide_range should be greater than 1, otherwise the search space never shrinks.")
    if weights is None:
        weights = [(min_val + max_val) / 2 for min_val, max_val in zip(min_vals, max_vals)]
    range_search = [(max_val - min_val) / 2 for min_val, max_val in zip(min_vals, max_vals)]
    many = getattr(loss, "many", None)
    if not callable(many):
        many = None
    curr_variable = 0
    iteration = 0
    range_deviations = [float('inf')] * len(max_vals)
    best_weights = weights
    best_loss = float('inf')
    evals = 0
    while True:
        if randomize:
            curr_variable = int(random() * len(weights))
        if max(range_search) == 0:
            break
        if shrink_strategy == "shrinking":
            range_search[curr_variable] = (max_vals[curr_variable] - min_vals[curr_variable]) \
                / ((iteration + 1) ** divide_range * log(iteration + 2))
        elif shrink_strategy == "divide":
            range_search[curr_variable] /= divide_range
        else:
            raise Exception("Invalid shrink strategy: either shrinking or divide expected")
        if range_search[curr_variable] == 0:
            range_deviations[curr_variable] = 0
            curr_variable += 1
            if curr_variable >= len(max_vals):
                curr_variable -= len(max_vals)
            continue
        if partition_strategy == "split":
            increments = [range_search[curr_variable] * (part * 2. / (partitions - 1) - 1) for part in range(partitions)]
        elif partition_strategy == "step":
            reach = int(range_search[curr_variable] / partitions)
            increments = [part * partitions for part in range(-reach, 1 + reach)]
        else:
            raise Exception("Invalid partition strategy: either split or step expected")
        candidate_weights = [_add(weights, curr_variable, increment, max_vals[curr_variable], min_vals[curr_variable], coarse=coarse)
                             for increment in increments]
        losses = list(many(candidate_weights)) if many is not None else [loss(w) for w in candidate_weights]
        if len(losses) != len(candidate_weights):
            raise Exception("loss.many must return one loss per candidate")
        loss_pairs = list(zip(candidate_weights, losses))
        evals += len(loss_pairs)
        weights, weights_loss = min(loss_pairs, key=lambda pair: pair[1])
        prev_best_loss = best_loss
        if validation_loss is not None:
            weights_loss = validation_loss(weights)
            if weights_loss < best_loss:
                best_loss = weights_loss
                best_weights = weights
        else:
            best_loss = weights_loss
            best_weights = weights
        range_deviations[curr_variable] = abs(prev_best_loss - best_loss)
        if verbose:
            _log(f"Tuning evaluations {evals} loss {best_loss:.8f} +- {max(range_deviations):.8f}")
        if max(range_deviations) <= deviation_tol and max(range_search) <= parameter_tol:
            break
        iteration += 1
        curr_variable += 1
        if curr_variable >= len(max_vals):
            curr_variable -= len(max_vals)
    weights = best_weights
    if verbose:
        _log()
    if depth > 1:
        return optimize(loss, max_vals, min_vals, deviation_tol, divide_range, partitions, parameter_tol, depth - 1, coarse,
                        shrink_strategy, partition_strategy, randomize, weights, verbose, validation_loss)
    return weights


default_tuning_optimization = {                             # parameterized.py:9-21
    "max_vals": [1] + [1] * 40,
    "min_vals": [1] + [0] * 40,
    "deviation_tol": 1.E-6,
    "parameter_tol": 1,
    "verbose": True,
    "divide_range": 1.01,
    "partitions": 5,
    "depth": 1,
    "coarse": 0,
    "shrink_strategy": "divide",
    "partition_strategy": "split"
}


class SelfClearDict(dict):
    """parameterized.py:24-35: a dictionary that holds one entry at a time (it clears itself before every assignment).  As the
    `optimization_dict` of a closed-form filter it keeps the stored powers of the LAST personalization only: back-to-back calls on
    one personalization (a tuner's probes) reuse them, and a new personalization releases the old slab."""

    def __setitem__(self, key, value):
        self.clear()
        super().__setitem__(key, value)


class Tuner(NodeRanking):
    """tuning.py:5-23: a ranker that first finds the ranker to run."""

    def tune(self, graph=None, personalization=None, *args, **kwargs):
        return self._tune(graph, personalization, *args, **kwargs)[0]

    def rank(self, graph=None, personalization=None, *args, **kwargs):
        ranker, personalization = self._tune(graph, personalization, *args, **kwargs)
        return ranker.rank(graph, personalization, *args, **kwargs)

    def _tune(self, graph=None, personalization=None, *args, **kwargs):
        raise Exception("Tuners should implement a _tune method")


class _ProbeLoss:
    """The tuner's loss for its default setting: ``loss(params)`` is the reference's one-probe evaluation
    (parameterized.py:135-145), ``loss.many(candidates)`` scores a coordinate step's candidates together.

    ``many``, per validation split: the candidates become GenericGraphFilter variants that share the tuner's optimisation dict, so
    the split's power slab is found (or built) there and a later rank() on the same personalization finds it too; every variant's
    coefficients are cut where its own stopping rule ends it (ClosedFormGraphFilter.probe_coefficients).  Then
      * fused: ``pgh_probe_auc`` -- one pass over the slab for all candidates -- when the library exports it and does not decline;
      * unfused: ``rank_many``'s [n, P] product and one ``measures.AUC`` per column with the split's `exclude`.
    Neither route applies the generator's ``Normalize("max")``: the AUC does not change under division by a positive maximum (a
    zero maximum means all-zero scores, AUC 0.5 either way), while an f32 division can round two neighbouring scores onto one
    value and so turn a strict order into a tie -- which is why the unfused route leaves it out as well when it stands in for the
    fused one (the two then agree to the last bit).  ``loss(params)`` keeps the reference's pipeline, Normalize included.
    Losses are -best_direction * AUC averaged over the splits."""

    def __init__(self, tuner, splits, filter_kwargs, args, kwargs):
        self.tuner, self.splits, self.filter_kwargs, self.args, self.kwargs = tuner, splits, filter_kwargs, args, kwargs
        self._plans = {}

    def __call__(self, params):
        return self.tuner._evaluate(self.splits, params, self.args, self.kwargs)

    def _plan(self, index, validation, exclude):
        plan = self._plans.get(index)
        if plan is None:
            plan = self._plans[index] = _ProbePlan(validation.np, None if exclude is None else to_signal(validation, exclude).np)
        return plan

    def _fused(self, index, validation, exclude, slab, coefficients):
        """[AUC of every column of `coefficients`] through pgh_probe_auc, or None when the entry is missing or declines."""
        entry = L.entry("pgh_probe_auc")
        if entry is None or slab.chebyshev or len(slab.slabs) < 1:     # (more than one slab of terms: the entry declines)
            return None
        plan = self._plan(index, validation, exclude)
        terms, probes = coefficients.shape
        flat = np.ascontiguousarray(coefficients, dtype=np.float64)
        out = (C.c_double * probes)()
        status = entry(slab.slabs[0]._h, flat.ctypes.data_as(C.c_void_p), terms, probes, plan._h, out)
        if status == L.DECLINED:
            if plan.num_positive == 0 or plan.num_negative == 0:
                raise Exception("Cannot evaluate AUC when all labels are the same")
            return None
        L.check(status)
        return list(out)

    def many(self, candidates):
        from pygrank_amd.filters import GenericGraphFilter
        candidates = list(candidates)
        totals = [0.0] * len(candidates)
        stats = self.tuner.last_tune
        for start in range(0, len(candidates), 64):
            chunk = candidates[start:start + 64]
            variants = [GenericGraphFilter(params, **self.filter_kwargs) for params in chunk]
            for index, (training, validation, exclude) in enumerate(self.splits):
                direction = AUC(validation, exclude).best_direction()
                plan = variants[0].probe_coefficients(training, None, variants)
                aucs = None if plan is None or self.tuner.fuse is False else \
                    self._fused(index, validation, exclude, plan[0], plan[1])
                if aucs is not None:
                    stats["fused_steps"] += 1
                else:
                    stats["unfused_steps"] += 1
                    ranks = plan[0].combine_many(plan[1]) if plan is not None else variants[0].rank_many(training, None, variants)[0]
                    measure = AUC(validation, exclude)
                    aucs = [measure.evaluate(to_signal(training, ranks.column(q))) for q in range(len(chunk))]
                for q, auc in enumerate(aucs):
                    totals[start + q] -= direction * auc
        return [total / len(self.splits) for total in totals]


class ParameterTuner(Tuner):
    """parameterized.py:38-177: tunes the parameters of a ranker family under a supervised measure on a training / validation
    split of the personalization [krasanakis2022autogf].

    ranker_generator: parameters -> ranker.  None (default): ``Normalize(GenericGraphFilter(params, ...))`` with an immutable-graph
        preprocessor and a ``SelfClearDict`` optimisation dict unless the keywords say otherwise; the filter's keywords are taken
        from kwargs (those ``optimize`` has no parameter for).
    measure: known scores, exclude -> supervised measure (default AUC).
    fraction_of_training: one ``split`` argument, or an iterable of them (one split each, seeds 0, 1, ...; losses are averaged).
    cross_validate: number of tuning runs (split seeds shifted by the run's number) whose parameters are averaged.
    combined_prediction: rank() applies the tuned ranker to the whole personalization (default) or to the training part.
    tuning_backend: None or "hip" (this package has one engine).
    optimizer: ``optimize`` or any callable(loss, **optimize arguments) -> parameters.
    kwargs: the arguments of ``optimize`` (defaults: ``default_tuning_optimization``) and of the generated filter.

    After a run ``last_params`` holds the tuned parameters and ``last_tune`` how many candidate batches took the fused
    (``fused_steps``) and the unfused (``unfused_steps``) route of the default setting; ``fuse=False`` keeps ``many`` off the
    fused entry (the unfused route then serves every step)."""

    def __init__(self, ranker_generator=None, measure=AUC, fraction_of_training=0.9, cross_validate=1, combined_prediction=True,
                 tuning_backend=None, optimizer=optimize, **kwargs):
        if tuning_backend not in (None, "hip"):
            raise Exception("tuning_backend is None or 'hip': this package drives one engine")
        self.fuse = kwargs.pop("fuse", True)
        self._filter_kwargs = None
        if ranker_generator is None:
            from pygrank_amd.filters import GenericGraphFilter
            from pygrank_amd.postprocess import Normalize
            if 'preprocessor' not in kwargs and 'assume_immutability' not in kwargs and 'normalization' not in kwargs:
                kwargs['preprocessor'] = preprocessor(assume_immutability=True)
            if "optimization_dict" not in kwargs:
                kwargs["optimization_dict"] = SelfClearDict()
            filter_kwargs = self._filter_kwargs = remove_used_args(optimize, kwargs)

            def ranker_generator(params):
                return Normalize(GenericGraphFilter(params, **filter_kwargs))
        self.ranker_generator = ranker_generator
        self.measure = measure
        self.fraction_of_training = fraction_of_training
        self.optimize_args = {kwarg: kwargs.get(kwarg, val) for kwarg, val in default_tuning_optimization.items()}
        self.combined_prediction = combined_prediction
        self.tuning_backend = tuning_backend
        self.cross_validate = cross_validate
        self.optimizer = optimizer
        self.last_tune = dict(fused_steps=0, unfused_steps=0)

    def _run(self, personalization, params, *args, **kwargs):
        return self.ranker_generator(params).rank(personalization, *args, **kwargs)

    def _evaluate(self, splits, params, args, kwargs):
        """parameterized.py:135-145: the loss of one parameter vector, one rank() and one measure per split."""
        val = 0
        for training, validation, exclude in splits:
            measure = self.measure(validation, exclude)
            val = val - measure.best_direction() * measure.evaluate(self._run(training, params, *args, **kwargs))
        return val / len(splits)

    def _splits(self, personalization, seed0):
        """[(training, validation, exclude)] of one tuning run (parameterized.py:125-133,143: the training part is excluded from the
        measure unless it IS the validation part)."""
        fractions = self.fraction_of_training if isinstance(self.fraction_of_training, Iterable) else [self.fraction_of_training]
        splits = []
        for seed, fraction in enumerate(fractions):
            training, validation = split(personalization, fraction, seed0 + seed)
            same = training is validation or np.array_equal(training._mirror(), validation._mirror())
            splits.append((training, validation, None if same else training))
        return splits

    def _loss(self, splits, args, kwargs):
        """The loss handed to the optimiser: with a ``many`` only for the default generator under AUC and no extra rank()
        arguments; anything else is the reference's one-probe-at-a-time loss."""
        if self._filter_kwargs is not None and self.measure is AUC and not args and not kwargs \
                and self._filter_kwargs.get("optimization_dict") is not None \
                and self._filter_kwargs.get("coefficient_type", "taylor").lower() in ("taylor", "chebyshev") \
                and self._filter_kwargs.get("krylov_dims") is None:
            return _ProbeLoss(self, splits, self._filter_kwargs, args, kwargs)
        return lambda params: self._evaluate(splits, params, args, kwargs)

    def _tune(self, graph=None, personalization=None, *args, **kwargs):
        personalization = to_signal(graph, personalization)
        self.last_tune = dict(fused_steps=0, unfused_steps=0)
        total_params = []
        training = personalization
        for seed0 in range(self.cross_validate):
            splits = self._splits(personalization, seed0)
            training = splits[-1][0]
            total_params.append(self.optimizer(self._loss(splits, args, kwargs), **self.optimize_args))
        best_params = [0 for _ in total_params[0]]
        for params in total_params:                          # parameterized.py:153-161: the mean over the runs
            for i in range(len(best_params)):
                best_params[i] += params[i] / self.cross_validate
        self.last_params = best_params
        return self.ranker_generator(best_params), personalization if self.combined_prediction else training

    def references(self):
        withheld = self.fraction_of_training
        withheld = f"{1 - withheld:.3f}" if not isinstance(withheld, Iterable) else \
            "/".join(f"{1 - fraction:.3f}" for fraction in withheld)
        name = getattr(self.measure, "__name__", type(self.measure).__name__)
        desc = "parameters tuned \\cite{krasanakis2022autogf} to optimize " + name \
               + f" while withholding {withheld} of nodes for validation"
        ret = list(self.ranker_generator([-42]).references())      # an invalid parameter value marks where the parameters are named
        for i in range(len(ret)):
            if "-42" in ret[i]:
                ret[i] = desc
                return ret
        return ret + [desc]


def hop_parameters(measure_values, num_parameters, autoregression=0):
    """hop_tuner.py:106-143 on the host in f64: the K x H hop values (K = num_parameters + autoregression hops, H held-out halves) ->
    the num_parameters hop weights before the offset search and the final normalisation.  The values are mean-centred per half; with
    autoregression > 0 an Adam loop fits a window that predicts every hop from the `autoregression` hops behind it and the
    predictions replace the values; the halves are averaged and the mean of the means is added back."""
    measure_values = np.array(measure_values, dtype=np.float64)
    mean_value = np.mean(measure_values, axis=0)
    measure_values = measure_values - mean_value
    best_parameters = measure_values
    measure_weights = [1] * measure_values.shape[1]
    if autoregression != 0:
        window = np.repeat(1. / autoregression, autoregression)
        beta1 = 0.9
        beta2 = 0.999
        beta1t = 1
        beta2t = 1
        rms = window * 0
        momentum = window * 0
        error = float('inf')
        while True:
            beta1t *= beta1
            beta2t *= beta2
            prev_error = error
            parameters = np.copy(measure_values)
            for i in range(len(measure_values) - len(window) - 2, -1, -1):
                parameters[i, :] = np.dot(window, measure_values[(i + 1):(i + len(window) + 1), :])
            errors = (parameters - measure_values) * measure_weights / np.sum(measure_weights)
            for j in range(len(window)):
                gradient = 0
                for i in range(len(measure_values) - len(window) - 1):
                    gradient += np.dot(measure_values[i + j + 1, :], errors[i, :])
                momentum[j] = beta1 * momentum[j] + (1 - beta1) * gradient
                rms[j] = beta2 * rms[j] + (1 - beta2) * gradient * gradient
                window[j] -= 0.01 * momentum[j] / (1 - beta1t) / ((rms[j] / (1 - beta2t)) ** 0.5 + 1.E-8)
            error = np.mean(np.abs(errors))
            if error == 0 or abs(error - prev_error) / error < 1.E-6:
                best_parameters = parameters
                break
    return np.mean(best_parameters[:num_parameters, :] * np.asarray(measure_weights, dtype=np.float64), axis=1) + np.mean(mean_value)


class _HopOffsetLoss:
    """The loss of HopTuner's offset search (hop_tuner.py:150-155): ``loss([offset])`` is the reference's one-probe evaluation,
    -best_direction * measure(_run(training, parameters + offset)).  ``many`` exists where a step's candidates share one slab pass:
      * "krylov" basis, the default generator and AUC: the candidates are GenericGraphFilter variants over the power slab of
        `training` in the tuner's optimisation dict, scored by ParameterTuner's _ProbeLoss (pgh_probe_auc);
      * "arnoldi" basis: one pgh_mat_gemm over the basis of the first half turns the candidates into an [n, P] slab that the
        measure's evaluate_many scores."""

    def __init__(self, tuner, measure, training, validation, parameters, base, args, kwargs):
        self.tuner, self.measure, self.training, self.parameters, self.base = tuner, measure, training, parameters, base
        self.args, self.kwargs = args, kwargs
        self._probe = None
        if not tuner.fused or args or kwargs:
            return
        filter_kwargs = tuner._filter_kwargs
        if base is not None:
            from pygrank_amd.device import DeviceMatrix
            if isinstance(base, DeviceMatrix) and base.b <= 64 and callable(getattr(measure, "evaluate_many", None)):
                self.many = self._many_arnoldi
        elif filter_kwargs is not None and tuner.tunable_offset is AUC and filter_kwargs.get("optimization_dict") is not None \
                and filter_kwargs.get("coefficient_type", "taylor").lower() in ("taylor", "chebyshev") \
                and filter_kwargs.get("krylov_dims") is None:
            self._probe = _ProbeLoss(tuner, [(training, validation, training)], filter_kwargs, args, kwargs)
            self.many = self._many_krylov

    def _weights(self, params):
        """hop_tuner.py:153 and _run's normalisation (hop_tuner.py:172-175)."""
        weights = np.array([self.parameters[i] + params[0] for i in range(len(self.parameters))], dtype=np.float64)
        div = np.sum(np.abs(weights))
        return weights / div if div != 0 else weights

    def __call__(self, params):
        weights = [self.parameters[i] + params[0] for i in range(len(self.parameters))]
        return -self.measure.best_direction() * self.measure(self.tuner._run(self.training, weights, self.base, *self.args, **self.kwargs))

    def _many_krylov(self, candidates):
        return self._probe.many([[float(w) for w in self._weights(params)] for params in candidates])

    def _many_arnoldi(self, candidates):
        candidates = list(candidates)
        losses = []
        for start in range(0, len(candidates), 64):
            coefficients = np.stack([self._weights(params) for params in candidates[start:start + 64]], axis=1)
            ranks = self.base.gemm(coefficients)
            self.tuner.last_tune["slab_passes"] += 2
            self.tuner.last_tune["fused_steps"] += 1
            losses.extend(-self.measure.best_direction() * value for value in self.measure.evaluate_many(ranks))
        return losses


class HopTuner(Tuner):
    """hop_tuner.py:14-184: tunes a GenericGraphFilter WITHOUT a search.  The training seeds are split in two halves, both are
    propagated hop by hop, every hop is scored against the held-out validation seeds (the half itself excluded) and the scores become
    the filter's hop weights.  (The reference marks the approach as experimental.)

    ranker_generator: parameters -> ranker.  None (default): ``GenericGraphFilter(params, **kwargs)`` with a ``SelfClearDict``
        optimisation dict unless the keywords say otherwise (no Normalize, no immutable preprocessor: the reference adds neither).
    measure: known scores, exclude -> supervised measure that scores a hop (default Cos).  With Cos the hop-0 score is 0 -- a half and
        the validation seeds are disjoint --, the filter's first weight is then 0 and the filter ends after 2 iterations with all-zero
        ranks, as in the reference.
    basis: "krylov" (the plain powers of the halves) or "arnoldi" (the columns of ``arnoldi_iteration`` of each half; the tuner then
        returns a Tautology and the combined basis as the personalization: no ranking algorithm comes out of it).
    tuning_backend: None or "hip" (this package has one engine).
    autoregression: hops a fitted window predicts every hop from (0: the scores are taken as they are); ``hop_parameters``.
    num_parameters: hop weights of the filter.
    tunable_offset: None, or a measure generator: an offset in [0, 1] added to every weight is searched with ``optimize`` on the
        training seeds against the validation seeds.
    pre_diffuse: accepted and unused, as in the reference.
    fused: True (default; an extension) runs the sweep on slabs: the powers of a half are the columns of an
        [n, K] slab, the K scores of a half come from one slab pass of the measure's ``evaluate_many`` (pgh_pair_forms with the half as
        `exclude`; pgh_probe_auc for AUC), the "arnoldi" basis comes from the two-pass Arnoldi step (include/pgh_arnoldi.h) and a step
        of the offset search scores its candidates together.  False -- and more than 64 hops, a graph that is not the engine's, a
        library without the entries -- is the reference's route, one backend primitive at a time.

    After a run ``last_params`` holds the weights, ``last_values`` the K x 2 hop values (``last_pre_offset`` and ``last_offset`` what
    the offset search started from and found) and ``last_tune`` the ``route`` ("fused" or
    "primitive"), the ``sweep`` ("steps", "arnoldi:fused", "arnoldi:primitive" or "primitive"), the ``scoring`` route of each
    half ("slab" or "columns"), the ``products`` with the adjacency, the ``slab_passes`` of the scoring,
    the Arnoldi steps and the offset search, and that search's ``fused_steps`` / ``unfused_steps``."""

    def __init__(self, ranker_generator=None, measure=Cos, basis="Krylov", tuning_backend=None, autoregression=0, num_parameters=20,
                 tunable_offset=None, pre_diffuse=None, fused=True, **kwargs):
        if tuning_backend not in (None, "hip"):
            raise Exception("tuning_backend is None or 'hip': this package drives one engine")
        self._filter_kwargs = None
        if ranker_generator is None:
            if "optimization_dict" not in kwargs:
                kwargs["optimization_dict"] = SelfClearDict()
            from pygrank_amd.filters import GenericGraphFilter
            filter_kwargs = self._filter_kwargs = kwargs

            def ranker_generator(params):
                return GenericGraphFilter(params, **filter_kwargs)
        else:
            ensure_used_args(kwargs, [])
        self.ranker_generator = ranker_generator
        self.measure = measure
        self.tuning_backend = tuning_backend
        self.autoregression = autoregression
        self.num_parameters = num_parameters
        self.tunable_offset = tunable_offset
        self.pre_diffuse = pre_diffuse
        self.basis = basis.lower()
        self.fused = fused
        self.last_tune = self._fresh_stats()
        self.last_params = self.last_values = None

    fuse = property(lambda self: self.fused)          # what _ProbeLoss asks its tuner

    @staticmethod
    def _fresh_stats():
        return dict(route="primitive", sweep="primitive", scoring=[], products=0, slab_passes=0, fused_steps=0, unfused_steps=0)

    def _evaluate(self, splits, params, args, kwargs):
        """One probe of the offset search as _ProbeLoss calls it: hop_tuner.py:152-154 for weights that are already normalised."""
        val = 0
        for training, validation, exclude in splits:
            measure = self.tunable_offset(validation, exclude)
            val = val - measure.best_direction() * measure(self._run(training, params, None, *args, **kwargs))
        return val / len(splits)

    # ---- the hop sweep ---------------------------------------------------------------------------------------------------------------
    def _score(self, measure, slab, stats):
        """The score of every column of `slab` under `measure`: one slab pass where the measure has one."""
        many = getattr(measure, "evaluate_many", None)
        if callable(many):
            values = [float(v) for v in many(slab)]
            route = getattr(measure, "last_route", None) or "columns"
        else:
            values, route = [float(measure(slab.column(i))) for i in range(slab.b)], "columns"
        stats["scoring"].append(route)
        stats["slab_passes"] += 1 if route == "slab" else slab.b
        return values

    def _sweep_powers(self, g, halves, hops, stats):
        """The [n, hops] slabs of the powers (M^T)^i p of both halves, or None where the slab route does not apply.
        A hop is one single-vector step per half.  Measured on an MI355X (tools/hop_bench.py, profiles/hop/; symmetrised RMAT, 20 hops,
        medians of 9, the routes alternating): that sweep takes 4.1-4.2 ms at scale 20 and 26.9-27.8 ms at scale 23, while one 2-wide
        pgh_spmm per hop for both halves takes 7.5-7.7 and 65.0-65.5 ms (disjoint spreads everywhere) -- a multi-seed pass of two
        columns costs more than two resident steps, so that route was measured and not kept."""
        from pygrank_amd.device import DeviceMatrix, DeviceVector
        if g is None or g.shape[0] != g.shape[1] or hops < 1 or hops > 64 \
                or any(not isinstance(p, DeviceVector) or len(p) != g.shape[0] for p in halves) \
                or L.entry("pgh_pair_forms") is None or L.entry("pgh_probe_auc") is None:
            return None                                      # (a library without the slab measures: nothing to score the slabs with)
        slabs = [DeviceMatrix.empty(len(p), hops) for p in halves]
        for slab, p in zip(slabs, halves):
            slab.set_column(0, p)
        current = list(halves)
        for i in range(1, hops):
            current = [g.conv(p) for p in current]
            stats["products"] += len(current)
            for slab, p in zip(slabs, current):
                slab.set_column(i, p)
        stats["sweep"] = "steps"
        return slabs

    def _hop_values(self, M, propagated, measures, hops, stats):
        """hop_tuner.py:94-101 -> (the hops x 2 list of values, the Arnoldi bases or None)."""
        from pygrank_amd import backend, krylov
        from pygrank_amd.device import DeviceMatrix
        g = krylov._device_graph(M)
        if self.basis == "krylov":
            slabs = self._sweep_powers(g, propagated, hops, stats) if self.fused else None
            if slabs is not None:
                stats["route"] = "fused"
                columns = [self._score(measure, slab, stats) for slab, measure in zip(slabs, measures)]
                return [[column[i] for column in columns] for i in range(hops)], None
            values = [None] * hops
            for i in range(hops):
                values[i] = [float(measure(p)) for p, measure in zip(propagated, measures)]
                propagated = [backend.conv(p, g if g is not None else M) for p in propagated]
                stats["products"] += len(propagated)
            stats["scoring"] = ["columns"] * len(measures)
            return values, None
        runs = [krylov.arnoldi_run(M, p, hops, self.fused) for p in propagated]
        basis = [run[0] for run in runs]
        routes = set(run[2] for run in runs)
        stats["route"] = "fused" if routes == {"fused"} else "primitive"
        stats["sweep"] = "arnoldi:" + stats["route"]
        stats["products"] += len(runs) * max(hops - 1, 0)
        for run in runs:
            stats["slab_passes"] += 2 * max(hops - 1, 0) if run[2] == "fused" else hops * (hops - 1)
        if stats["route"] == "fused" and all(isinstance(base, DeviceMatrix) and base.b <= 64 for base in basis):
            columns = [self._score(measure, base, stats) for base, measure in zip(basis, measures)]
            return [[column[i] for column in columns] for i in range(hops)], basis
        stats["scoring"] = ["columns"] * len(measures)
        return [[float(measure(base.column(i))) for base, measure in zip(basis, measures)] for i in range(hops)], basis

    def _tune(self, graph=None, personalization=None, *args, **kwargs):
        from pygrank_amd import backend
        from pygrank_amd.postprocess import Tautology
        stats = self.last_tune = self._fresh_stats()
        personalization = to_signal(graph, personalization)
        graph = personalization.graph
        backend_personalization = to_signal(personalization, backend.to_array(personalization.np))
        hops = self.num_parameters + self.autoregression
        M = self.ranker_generator([None] * hops).preprocessor(graph)
        training, validation = split(backend_personalization, 0.8)
        training1, training2 = split(training, 0.5)
        propagated = [training1.np, training2.np]
        measures = [self.measure(validation, training1), self.measure(validation, training2)]
        measure_values, basis = self._hop_values(M, propagated, measures, hops, stats)
        self.last_values = np.array(measure_values, dtype=np.float64)
        best_parameters = hop_parameters(self.last_values, self.num_parameters, self.autoregression)
        if self.tunable_offset is not None:
            div = np.max(best_parameters)
            if div != 0:
                best_parameters = best_parameters / div
            measure = self.tunable_offset(validation, training)
            base = basis[0] if self.basis != "krylov" else None
            self.last_pre_offset = np.array(best_parameters, dtype=np.float64)
            loss = _HopOffsetLoss(self, measure, training, validation, best_parameters, base, args, kwargs)
            best_offset = optimize(loss, max_vals=[1], min_vals=[0], deviation_tol=0.005, parameter_tol=1, partitions=5, divide_range=1.1)
            self.last_offset = float(best_offset[0])
            best_parameters = np.array([best_parameters[i] + best_offset[0] for i in range(len(best_parameters))], dtype=np.float64)
        if np.sum(np.abs(best_parameters)) != 0:
            best_parameters = best_parameters / np.mean(np.abs(best_parameters))
        best_parameters = [float(param) for param in best_parameters]
        self.last_params = best_parameters
        if self.basis != "krylov":
            return Tautology(), self._run(personalization, best_parameters, None, *args, **kwargs)
        return self.ranker_generator(best_parameters), personalization

    def _run(self, personalization, params, base=None, *args, **kwargs):
        """hop_tuner.py:171-184: the filter of the normalised weights ("krylov"), or the weighted sum of the Arnoldi basis of the
        personalization (of `base` where one is given): one pgh_mat_gemv."""
        from pygrank_amd import krylov
        from pygrank_amd.device import DeviceMatrix
        params = np.array(params, dtype=np.float64)
        div = np.sum(np.abs(params))
        if div != 0:
            params = params / div
        if self.basis != "krylov":
            if base is None:
                M = self.ranker_generator(params).preprocessor(personalization.graph)
                base, _, route = krylov.arnoldi_run(M, personalization.np, len(params), self.fused)
                self.last_tune["products"] += max(len(params) - 1, 0)
                self.last_tune["slab_passes"] += 2 * max(len(params) - 1, 0) if route == "fused" else len(params) * (len(params) - 1)
            if isinstance(base, DeviceMatrix):
                return to_signal(personalization, base.gemv(params))
            ret = 0
            for i in range(len(params)):
                ret = ret + params[i] * base[:, i]
            return to_signal(personalization, ret)
        return self.ranker_generator([float(param) for param in params]).rank(personalization, *args, **kwargs)


def _convergence_key(ranker):
    """What two filters must share to be columns of one device loop: the stopping rule the engine evaluates."""
    cm = ranker.convergence
    return (cm.device_error_kind(), float(cm.effective_tolerance()), int(cm.max_iters), int(cm.end_modulo))


class AlgorithmSelection(Tuner):
    """selection.py:10-91: the best of a list of rankers, found by holding part of the personalization back and scoring how well every
    ranker recovers it from the rest.

    rankers: the candidates, visited in order (default: ``create_demo_filters().values()``).  Filters that share a preprocessor share
        the uploaded graph.
    measure: known scores, exclude -> supervised measure (default AUC); the training part is always excluded.
    fraction_of_training: one ``split`` argument, or an iterable of them (one split each, seeds 0, 1, ...).  A ranker's value is the
        LEAST of ``best_direction * measure`` over the splits; the first ranker of the greatest value is selected.
    combined_prediction: rank() applies the selected ranker to the whole personalization (default) or to the last training part.
    tuning_backend: None or "hip" (this package drives one engine).
    batch: True (default) runs the candidates that are plain filters as mixed batches (include/pgh_mixed.h), columns = (ranker, split)
        pairs, 64 at a time.  Bare ``PageRank`` instances that share the preprocessor, ``use_quotient`` and the stopping rule form one
        group (pgh_ppr_run_batch_mixed: an alpha per column); bare taylor-form ``HeatKernel`` / ``PageRankClosed`` /
        ``GenericGraphFilter`` instances that share the preprocessor and the stopping rule form another (pgh_poly_run_batch_mixed: a
        coefficient schedule per column).  Everything else -- a ranker inside a postprocessor, a filter that runs in f64 (``tol`` below
        fp32 eps), AbsorbingWalks, the chebyshev form, a group of one ranker or of fewer than ``min_batch_width`` columns, a library
        without the entries, a graph the entries decline -- is ranked exactly as ``batch=False`` ranks everything: one ``rank()`` per
        ranker and split.  The columns of one split are scored together by the measure's ``evaluate_many`` where it has one.
    min_batch_width: the least number of columns (rankers x splits) a group is batched at; None (default): ``MIN_BATCH_WIDTH``.
    retire: False (default), True or a list of levels, as ``PageRank(retire=)``: the mixed PageRank group retires its converged columns
        inside the loop (pgh_ppr_run_batch_mixed_retire, include/pgh_retire.h; its columns stop at different steps, one alpha each) and
        the call's record in ``mixed_calls`` carries the run's report under "stages".  The plain entry where the library lacks that one or
        it declines.

    After a run ``last_selection`` holds ``rankers`` (per ranker: ``values`` per split and the ``route`` taken: "mixed_ppr",
    "mixed_poly" or "single"), ``mixed_calls`` (per engine call: ``kind``, ``width``, the per-column ``iterations`` and the loop's
    ``loop_ms``) and
    ``selected`` (the index of the chosen ranker)."""

    # Measured on an MI355X at RMAT scale 23 under the L1 rule (tools/select_bench.py, profiles/selection/): a selection whose groups are
    # 4 columns wide takes 1.23 times as long batched as one by one (disjoint spreads); at 8, 12 and 16 columns 0.98, 0.96 and 0.90 (inside
    # the spreads).  Widths 5 to 7 are not measured.
    MIN_BATCH_WIDTH = 8

    def __init__(self, rankers=None, measure=AUC, fraction_of_training=0.9, combined_prediction=True, tuning_backend=None, batch=True,
                 min_batch_width=None, retire=False):
        if tuning_backend not in (None, "hip"):
            raise Exception("tuning_backend is None or 'hip': this package drives one engine")
        if rankers is None:
            from pygrank_amd.comparables import create_demo_filters
            rankers = create_demo_filters().values()
        self.rankers = rankers
        self.measure = measure
        self.fraction_of_training = fraction_of_training
        self.combined_prediction = combined_prediction
        self.tuning_backend = tuning_backend
        self.batch = batch
        self.min_batch_width = min_batch_width
        self.retire = retire
        self.last_selection = None

    # ---- the batch route -----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _group_key(ranker):
        """(kind, what the group shares) of a ranker a mixed batch can hold, or None."""
        from pygrank_amd.convergence import ConvergenceManager
        from pygrank_amd.filters import GenericGraphFilter, GraphFilter, HeatKernel, PageRank, PageRankClosed
        from pygrank_amd.postprocess import Tautology
        if type(ranker) is PageRank:
            if not ranker._plain_quotient():
                return None
            kind, extra = "mixed_ppr", (bool(ranker.use_quotient),)
        elif type(ranker) in (HeatKernel, PageRankClosed, GenericGraphFilter):
            if ranker.coefficient_type != "taylor" or ranker.optimization_dict is not None or ranker.krylov_dims is not None:
                return None
            kind, extra = "mixed_poly", ()
        else:
            return None
        if type(ranker.convergence) is not ConvergenceManager or ranker._loop_cfg() is None or ranker._f64_wanted():
            return None
        # every member's own rank() must be the plain f32 loop on the raw personalization (the test of GraphFilter._batch_graph): a
        # personalization transform or a graph hook of ANY member keeps that member out, not only the group's first
        transform = ranker.personalization_transform
        if not (isinstance(transform, Tautology) and transform.ranker is None) or type(ranker)._prepare_graph is not GraphFilter._prepare_graph:
            return None
        return (kind, id(ranker.preprocessor)) + extra + _convergence_key(ranker)

    def _run_group(self, kind, members, rankers, splits, columns_of, calls):
        """Ranks the (ranker, split) pairs of one group as mixed batches.  columns_of[split] gains (ranker index, ranks vector) pairs;
        returns False (nothing gained) when the entry is missing or declines."""
        from pygrank_amd.device import DeviceMatrix
        from pygrank_amd.filters import _batch_call
        entry = L.entry("pgh_ppr_run_batch_mixed" if kind == "mixed_ppr" else "pgh_poly_run_batch_mixed")
        if entry is None:
            return False
        first = rankers[members[0]]
        g = first._batch_graph(splits[0][0].graph, (), {})
        if g is None:
            return False
        pairs = [(r, s) for r in members for s in range(len(splits))]
        gained = []
        for start in range(0, len(pairs), 64):
            chunk = pairs[start:start + 64]
            slab = DeviceMatrix.from_columns([splits[s][0].np for _, s in chunk])
            norms = slab.col_abssum()
            P = slab.div_cols(norms)                            # abstract_filters.py:52-55 per column; zero columns stay zero
            R = DeviceMatrix.empty(slab.n, slab.b)
            results = (L.LoopResult * slab.b)()
            scales = (C.c_double * slab.b)(*[(float(nrm) if rankers[r].preserve_norm else 1.0) for (r, _), nrm in zip(chunk, norms)])
            if kind == "mixed_ppr":
                cfg = first._loop_cfg(0.0, bool(first.use_quotient), 1.0)
                cfg.start_from_p = 1
                alphas = (C.c_double * slab.b)(*[float(rankers[r].alpha) for r, _ in chunk])
                status, stages = _batch_call(self, entry, "pgh_ppr_run_batch_mixed_retire",
                                             (g._h, P._h, R._h, C.byref(cfg), alphas, scales, results))
            else:
                stages = None
                cfg = first._loop_cfg(0.0, False, 1.0)
                cfg.start_from_p = 1
                terms = max(int(first.convergence.max_iters) - 1, 0)
                schedule = {r: rankers[r]._coefficient_schedule(terms) for r in members}
                coeffs = np.ascontiguousarray(np.array([schedule[r] for r, _ in chunk], dtype=np.float64).T.reshape(terms, slab.b))
                status = entry(g._h, P._h, coeffs.ctypes.data_as(C.c_void_p), terms, R._h, C.byref(cfg), scales, results)
            if status == L.DECLINED and not gained:
                return False
            L.check(status)
            calls.append(dict(kind=kind, width=slab.b, iterations=[res.iterations for res in results], loop_ms=results[0].loop_ms,
                              **({} if stages is None else dict(stages=stages))))
            for j, ((r, s), res, nrm) in enumerate(zip(chunk, results, norms)):
                if nrm != 0:
                    rankers[r].convergence.start()
                    rankers[r].convergence.finish_device_loop(res.iterations, res.converged)   # raises like the ranker's own rank()
                gained.append((s, r, R.column(j)))
        for s, r, column in gained:
            columns_of[s].append((r, column))
        return True

    def _batch_values(self, rankers, splits, values, routes, calls):
        """Fills values[ranker][split] (best_direction * measure) and routes[ranker] for every ranker a mixed batch served."""
        groups = {}
        for index, ranker in enumerate(rankers):
            key = self._group_key(ranker)
            if key is not None:
                groups.setdefault(key, []).append(index)
        columns_of = [[] for _ in splits]
        least = self.MIN_BATCH_WIDTH if self.min_batch_width is None else self.min_batch_width
        for key, members in groups.items():
            if len(members) >= 2 and len(members) * len(splits) >= least \
                    and self._run_group(key[0], members, rankers, splits, columns_of, calls):
                for r in members:
                    routes[r] = key[0]
        for s, (training, validation) in enumerate(splits):
            if not columns_of[s]:
                continue
            measure = self.measure(validation, training)
            signals = [to_signal(training, column) for _, column in columns_of[s]]
            many = getattr(measure, "evaluate_many", None)
            scores = many(signals) if callable(many) else [measure.evaluate(signal) for signal in signals]
            for (r, _), score in zip(columns_of[s], scores):
                values[r][s] = measure.best_direction() * score

    def _tune(self, graph=None, personalization=None, *args, **kwargs):
        personalization = to_signal(graph, personalization)
        tuning_kwargs = dict(kwargs, graph_dropout=0)            # selection.py:64-65: no dropout while the candidates are compared
        fractions = self.fraction_of_training if isinstance(self.fraction_of_training, Iterable) else [self.fraction_of_training]
        splits = [split(personalization, fraction, seed=seed) for seed, fraction in enumerate(fractions)]
        rankers = list(self.rankers)
        values = [[None] * len(splits) for _ in rankers]
        routes = ["single"] * len(rankers)
        calls = []
        if self.batch and not args and set(kwargs) <= {"graph_dropout"}:
            self._batch_values(rankers, splits, values, routes, calls)
        best_value, best_ranker, selected = -float('inf'), None, None
        for index, ranker in enumerate(rankers):
            for s, (training, validation) in enumerate(splits):
                if values[index][s] is None:
                    measure = self.measure(validation, training)
                    values[index][s] = measure.best_direction() * measure.evaluate(ranker.rank(training, *args, **tuning_kwargs))
            value = min(values[index])
            if value > best_value:                               # strict: the first of equally good rankers is kept
                best_value, best_ranker, selected = value, ranker, index
        self.last_selection = dict(rankers=[dict(values=list(v), route=route) for v, route in zip(values, routes)],
                                   mixed_calls=calls, selected=selected)
        training = splits[-1][0] if splits else personalization
        return best_ranker, personalization if self.combined_prediction else training

    def references(self):
        withheld = self.fraction_of_training
        withheld = f"{1 - withheld:.3f}" if not isinstance(withheld, Iterable) else \
            "/".join(f"{1 - fraction:.3f}" for fraction in withheld)
        name = getattr(self.measure, "__name__", type(self.measure).__name__)
        desc = "selected the best among the following algorithms \\cite{krasanakis2022autogf} that optimizes " + name \
               + f" while withholding {withheld} of nodes for validation: \\\\\n"
        for ranker in self.rankers:
            desc += "  - " + ranker.cite() + " \\\\\n"
        return [desc]
