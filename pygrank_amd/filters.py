"""Graph filters of the propagation path on the MI355X engine.

Same classes, constructor arguments, operators and error behaviour as the reference:
  GraphFilter / RecursiveGraphFilter / ClosedFormGraphFilter  pygrank/algorithms/filters/abstract_filters.py:11-270
  PageRank, PageRankClosed, HeatKernel, AbsorbingWalks         pygrank/algorithms/filters/adhoc.py:9-174
  GenericGraphFilter, ImpulseGraphFilter, LowPassRecursive...  pygrank/algorithms/filters/low_pass.py:5-91

Two execution routes, both on the GPU:
  * generic route -- the reference's ``_start / while not has_converged: _step / _end`` structure
    (abstract_filters.py:58-62) expressed with backend primitives; used whenever an option needs per-step
    Python (callable quotient, custom error measure, optimisation dict, graph dropout ...).
  * fused route -- the whole loop runs inside the engine (pgh_ppr_run / pgh_absorb_run / pgh_poly_run,
    include/pgh.h): one merge-path SpMV kernel per iteration with the filter's vector algebra in its
    epilogue, the residual as a separate wavefront-reduced kernel, and ConvergenceManager's stopping rule
    evaluated on the device so that the host does not synchronise every iteration.  Results and
    ``convergence.iteration`` are those of the generic route.
"""
import ctypes as C

import numpy as np

from pygrank_amd import _lib as L
from pygrank_amd import backend
from pygrank_amd.convergence import ConvergenceManager
from pygrank_amd.device import DeviceGraph, DeviceVector, LazyVector
from pygrank_amd.postprocess import Postprocessor, Tautology
from pygrank_amd.preprocessing import obj2id, preprocessor as default_preprocessor
from pygrank_amd.signals import GraphSignal, NodeRanking, to_signal
from pygrank_amd.utils import call, ensure_used_args


def _device_graph(M):
    array = getattr(M, "array", M)
    return array if isinstance(array, DeviceGraph) else None


def _f64_image_usable(g):
    """The engine's f64 image serves square graphs that carry the blocked layout (csrc/pgh_bsf64.hip bsf64_usable)."""
    return g is not None and g.shape[0] == g.shape[1] and g.shape[0] > 0 and g.nnz > 0 and "row-major" not in g.format()


def _batch_call(ranker, plain, retiring, args):
    """One multi-seed call of propagate: through `plain(*args)`, or -- when ``ranker.retire`` asks for it -- through the entry
    `retiring` of include/pgh_retire.h, which takes the same arguments with the levels and a report behind them and retires converged
    columns inside the loop.  A library without that entry takes the plain call, and so does a call the entry DECLINED.  Returns
    (status, the report as ``_lib.retire_stages`` gives it, or None after a plain call)."""
    entry = L.entry(retiring) if L.retire_on(getattr(ranker, "retire", False)) else None
    if entry is not None:
        levels, count = L.retire_levels(ranker.retire)
        report = L.RetireReport()
        status = entry(*args, levels, count, C.byref(report))
        if status != L.DECLINED:
            return status, (L.retire_stages(report) if status == 0 else None)
    return plain(*args), None


def _batch_info(results, stages):
    """The per-column records of one chunk in ``last_batches``; a run of include/pgh_retire.h adds its report under "stages"."""
    extra = {} if stages is None else dict(stages=stages)
    return [dict(iterations=r.iterations, converged=bool(r.converged), spmv=r.spmv_count, loop_ms=r.loop_ms, flags=r.flags, **extra)
            for r in results]


def _propagate_in_batches(ranker, features, cfg, run):
    """signals.py:225-226 (one rank() per feature column) as multi-seed device loops of up to 64 columns with the prologue of
    PageRank.propagate: per-column L1 norms (abstract_filters.py:52-55; zero columns stay zero), preserve_norm factors, the loop
    started from p (:56), ConvergenceManager's verdict per non-zero column.  run(P, R, cfg_ref, scales, results) -> what _batch_call
    returns for one include/pgh_batch.h call.  Returns the [n, B] ranks, or None when the engine declined the first chunk (nothing was run)."""
    from pygrank_amd.device import DeviceMatrix
    F = features if isinstance(features, DeviceMatrix) else backend.to_primitive(features)
    if not isinstance(F, DeviceMatrix):
        F = DeviceMatrix.from_columns([F])
    cfg.start_from_p = 1
    batches = []
    out = DeviceMatrix.empty(F.n, F.b) if F.b > 64 else None
    for start, chunk in F.chunks():
        norms = chunk.col_abssum()
        P = chunk.div_cols(norms)
        R = DeviceMatrix.empty(chunk.n, chunk.b)
        results = (L.LoopResult * chunk.b)()
        scales = (C.c_double * chunk.b)(*[(float(nrm) if ranker.preserve_norm else 1.0) for nrm in norms])
        ranker.convergence.start()
        status, stages = run(P, R, C.byref(cfg), scales, results)
        if status == L.DECLINED and not batches:
            return None
        L.check(status)
        batches.append(_batch_info(results, stages))
        ranker.last_batches = batches
        for r, nrm in zip(results, norms):
            if nrm != 0:
                ranker.convergence.finish_device_loop(r.iterations, r.converged)   # raises like the per-column run would
        if out is None:
            return R
        out.set_cols(start, R)
    return out


def _propagate_in_batches64(ranker, features, cfg, run, raw):
    """_propagate_in_batches through an entry of include/pgh_batch64.h (``GraphFilter(f64_batch=True)``): the loop keeps its iterates,
    sums, quotients and residuals in f64 and the tolerance is clamped at fp64 eps (_f64_cfg).  raw: the chunk goes in UN-normalised
    with its column norms beside it, as _f64_operands hands a single vector to the f64 route (the recursive filters); otherwise
    L1-normalised in f32, as the closed-form filters' single rank() does.  run(P, R, cfg_ref, scales, results, norms) -> status.
    Every record of ``last_batches`` carries "f64": True.  Returns the [n, B] ranks, or None when the engine declined the first chunk
    (nothing was run)."""
    from pygrank_amd.device import DeviceMatrix
    F = features if isinstance(features, DeviceMatrix) else backend.to_primitive(features)
    if not isinstance(F, DeviceMatrix):
        F = DeviceMatrix.from_columns([F])
    cfg = ranker._f64_cfg(cfg)
    cfg.start_from_p = 1
    batches = []
    out = DeviceMatrix.empty(F.n, F.b) if F.b > 64 else None
    for start, chunk in F.chunks():
        norms = chunk.col_abssum()
        P = chunk
        if not raw:
            # p * f32(1 / |p|), the bits a single rank() hands its loop (device.py _scalar_factor: a division by a scalar is a
            # multiplication); a library without the slab form divides (a last bit of p may then differ from the single run's)
            P = chunk.col_scale([1.0 / nrm if nrm != 0 else 1.0 for nrm in norms])
            if P is None:
                P = chunk.div_cols(norms)
        R = DeviceMatrix.empty(chunk.n, chunk.b)
        results = (L.LoopResult * chunk.b)()
        scales = (C.c_double * chunk.b)(*[(float(nrm) if ranker.preserve_norm else 1.0) for nrm in norms])
        in_norms = (C.c_double * chunk.b)(*[float(nrm) for nrm in norms])
        ranker.convergence.start()
        status = run(P, R, C.byref(cfg), scales, results, in_norms)
        if status == L.DECLINED and not batches:
            return None
        L.check(status)
        batches.append([dict(record, f64=True) for record in _batch_info(results, None)])
        ranker.last_batches = batches
        for r, nrm in zip(results, norms):
            if nrm != 0:
                ranker.convergence.finish_device_loop(r.iterations, r.converged)   # raises like the per-column run would
        if out is None:
            return R
        out.set_cols(start, R)
    return out


class GraphFilter(NodeRanking):
    """abstract_filters.py:11-106."""

    # collaborators a filter builds for itself from its keyword arguments when none is handed in: attribute -> factory
    _BUILT_FROM_KWARGS = (("preprocessor", default_preprocessor), ("convergence", ConvergenceManager))

    def __init__(self, preprocessor=None, convergence=None, personalization_transform=None, preserve_norm=True,
                 dtype=None, f64_batch=False, **kwargs):
        """dtype (an extension of this backend; the reference's numpy engine is fp64 throughout, pygrank/core/backend/numpy.py:84-86):
        None -- the engine's f32 loop, and f64 iterates / sums / quotient / residual on the engine's f64 image whenever the tolerance lies
        below fp32 eps (where an f32 loop, clamped at fp32 eps by convergence.py:101, stops early: the reference's AbsorbingWalks default
        alpha = 1 - 1e-6 with tol = 1e-9 takes 21 iterations, an f32 loop 12); "float32" -- always the f32 loop; "float64" -- always f64.
        f64_batch (an extension; also an attribute; off by default): where a run wants f64 iterates and ``propagate`` would otherwise
        take its f32 multi-seed route, PageRank, AbsorbingWalks, SymmetricAbsorbingRandomWalks and the taylor form of the closed-form
        filters run chunks of up to 64 columns through the f64 multi-seed loops of include/pgh_batch64.h instead of one f64 loop per
        column; ``last_batches`` records carry "f64": True.  A column may differ from the column loop's in its last bits (the row sums
        are grouped differently).  Not served -- today's route: graph_dropout, the "chebyshev" form, warm starts, AlgorithmSelection's
        mixed groups, LFPR; ``retire=`` is ignored by the f64 batch (a later piece of work)."""
        if dtype not in (None, "float32", "float64"):
            raise Exception("dtype is None (f32, f64 below fp32 eps), 'float32' or 'float64'")
        self.dtype = dtype
        self.f64_batch = f64_batch
        given = dict(preprocessor=preprocessor, convergence=convergence)
        for attribute, factory in self._BUILT_FROM_KWARGS:
            setattr(self, attribute, given[attribute] if given[attribute] is not None else call(factory, kwargs))
        ensure_used_args(kwargs, [factory for _, factory in self._BUILT_FROM_KWARGS])   # a keyword nobody declares is a typo
        self.personalization_transform = personalization_transform or Tautology()
        self.preserve_norm = preserve_norm

    def _prepare(self, personalization):
        pass

    def rank(self, graph=None, personalization=None, warm_start=None, graph_dropout=0, *args, **kwargs):
        """abstract_filters.py:44-65.  personalization -> signal -> (transform) -> L1-normalised seed vector; the iterate starts
        as a copy of it (or of warm_start); the preprocessor turns the graph into the operator; the loop runs until the
        convergence manager says stop; preserve_norm gives the input's L1 norm back.  Whenever the configuration allows it the
        whole loop is ONE engine call (_fused_rank / _fused_loop); the hook protocol below serves everything else."""
        seed_signal = to_signal(graph, personalization)
        self._prepare(seed_signal)
        signal = self.personalization_transform(seed_signal)
        if warm_start is None:
            # norm, normalisation and start vector folded into the engine's first pass over the operands (pgh_loop_cfg.in_norm < 0,
            # start_from_p): no reduction and no host round trip in front of the first step.  A zero norm comes back as the signal.
            # graph_dropout > 0: the same loop with a fresh mask per step inside the step's kernels (pgh_ppr_run_dropout).
            fused = self._fused_rank(signal, *args, **kwargs) if graph_dropout == 0 else \
                self._fused_rank(signal, *args, dropout=graph_dropout, **kwargs)
            if fused is not None:
                return fused
        raw = signal.np
        norm = raw.abssum() if isinstance(raw, DeviceVector) else backend.sum(backend.abs(raw))
        if norm == 0:
            return signal                       # nothing to spread: the reference hands the (all-zero) signal back
        # (the f64 routes of the walks normalise the personalization themselves, in f64: an f32 quotient p / |p| sums to 1 only within
        # 6e-8, which a run at tol = 1e-9 sees -- it would start beside the fixed point the reference starts ON)
        self._raw_input = (raw, float(norm)) if warm_start is None and isinstance(raw, DeviceVector) else None
        signal = to_signal(signal, signal.np / norm)
        # the reference never writes into the caller's warm_start (every step builds a fresh array); the device loops update
        # their iterate in place, so the start vector is always a copy
        ranks = to_signal(signal, backend.copy(signal.np if warm_start is None else to_signal(signal, warm_start).np))
        M = self.preprocessor(self._prepare_graph(signal.graph, signal, *args, **kwargs))
        self.convergence.start()
        try:
            fused = graph_dropout == 0 and self._fused_loop(M, signal, ranks, norm if self.preserve_norm else 1.0, *args, **kwargs)
        finally:
            self._raw_input = None             # (only the f64 routes of _fused_loop look at it; nothing keeps the caller's vector alive)
        if fused:
            return ranks
        self._host_driven_loop(M, signal, ranks, graph_dropout, args, kwargs)
        if self.preserve_norm:
            ranks.np = ranks.np * norm
        return ranks

    def _host_driven_loop(self, M, signal, ranks, dropout_rate, args, kwargs):
        """The hook protocol of abstract_filters.py:57-62 for filters and configurations without a device loop: _start, then
        _step until the convergence manager stops the loop, then _end -- each hook sees an operator whose entries were dropped
        afresh (backend.graph_dropout draws a new mask per call; rate 0 returns the operator itself)."""
        def operator():
            return backend.graph_dropout(M, dropout_rate)
        self._start(operator(), signal, ranks, *args, **kwargs)
        keep_going = lambda: not self.convergence.has_converged(ranks.np)      # noqa: E731
        while keep_going():
            self._step(operator(), signal, ranks, *args, **kwargs)
        self._end(operator(), signal, ranks, *args, **kwargs)

    # ---- hooks
    def _fused_rank(self, personalization, *args, dropout=0, **kwargs):
        """Whole rank() inside the engine, norm included, starting from the UN-normalised personalization; returns the ranks
        signal (the personalization itself when its norm is zero) or None when this filter / configuration has no such route.
        dropout: graph_dropout of every step."""
        return None

    def _fused_loop(self, M, personalization, ranks, out_scale, *args, **kwargs):
        """Runs the whole loop inside the engine when the configuration allows it; returns True when it did."""
        return False

    def _f64_wanted(self):
        """f64 iterates for this run (see __init__): asked for, or chosen because the tolerance lies below fp32 eps."""
        if self.dtype == "float64":
            return True
        cm = self.convergence
        if self.dtype == "float32" or type(cm) is not ConvergenceManager or cm.device_error_kind() in (None, L.ERR_ITERS):
            return False
        return cm.tol is None or float(cm.tol) < backend.epsilon()

    def _f64_cfg(self, cfg):
        """the loop configuration of an f64 route: the tolerance never below fp64 eps (convergence.py:101 with numpy's epsilon())"""
        tol = self.convergence.tol
        cfg.tol = 0.0 if tol is None else max(float(tol), float(np.finfo(np.float64).eps))
        return cfg

    def _f64_operands(self, cfg, p):
        """(cfg, personalization) of an f64 recursive route: the UN-normalised personalization with its norm beside it whenever rank()
        kept them (no warm start) -- the engine then forms p / |p| and the start vector in f64 (pgh_loop_cfg.in_norm, start_from_p)"""
        cfg = self._f64_cfg(cfg)
        raw = getattr(self, "_raw_input", None)
        if raw is not None and len(raw[0]) == len(p) and raw[1] > 0:
            cfg.in_norm, cfg.start_from_p = raw[1], 1
            return cfg, raw[0]
        return cfg, p

    def _loop_cfg(self, alpha=0.0, use_quotient=False, out_scale=1.0):
        cm = self.convergence
        if type(cm) is not ConvergenceManager:
            return None
        kind = cm.device_error_kind()
        if kind is None:
            return None
        return L.LoopCfg(alpha=float(alpha), use_quotient=1 if use_quotient else 0, err_kind=kind,
                         tol=float(cm.effective_tolerance()), max_iters=int(cm.max_iters),
                         end_modulo=int(cm.end_modulo), out_scale=float(out_scale))

    def _prepare_graph(self, graph, *args, **kwargs):
        return graph

    def _batch_graph(self, graph, args, kwargs, allowed=(), f64=False):
        """The device graph of a multi-seed loop (include/pgh_batch.h) for propagate(graph, ..., *args, **kwargs), or None where a single
        rank() would not run the f32 fused loop: extra arguments, graph_dropout, f64 iterates (dtype or a tolerance below fp32 eps), a
        personalization transform, a stopping rule the engine cannot evaluate, a non-square / row-major / empty or non-device graph.
        f64: the same question for the f64 multi-seed loops (include/pgh_batch64.h) -- the run must WANT f64 iterates and the filter
        must have been built with f64_batch=True; everything else is judged alike."""
        if args or any(k not in allowed and not (k == "graph_dropout" and not kwargs[k]) for k in kwargs):
            return None
        if self._loop_cfg() is None or self._f64_wanted() != f64 or (f64 and not getattr(self, "f64_batch", False)):
            return None
        transform = self.personalization_transform
        if not (isinstance(transform, Tautology) and transform.ranker is None) or type(self)._prepare_graph is not GraphFilter._prepare_graph:
            return None
        g = _device_graph(self.preprocessor(graph))
        if g is None or g.shape[0] != g.shape[1] or g.shape[0] == 0 or g.nnz == 0 or "row-major" in g.format():
            return None
        return g

    def _start(self, M, personalization, ranks, *args, **kwargs):
        pass

    def _end(self, M, personalization, ranks, *args, **kwargs):
        pass

    def _step(self, M, personalization, ranks, *args, **kwargs):
        raise Exception("Use a derived class of GraphFilter that implements the _step method")

    def _slot_for(self, part):
        """Which attribute `filter + part` replaces (abstract_filters.py:86-95): a convergence manager, a preprocessor
        (recognised by the name preprocessor() gives its outcome) or a postprocessor that takes the quotient's place."""
        if isinstance(part, ConvergenceManager):
            return "convergence"
        if getattr(part, "__name__", None) == "preprocess":
            return "preprocessor"
        if isinstance(part, Postprocessor):
            return "use_quotient"
        return None

    def __add__(self, part):
        slot = self._slot_for(part)
        if slot is None:
            raise Exception("a graph filter takes convergence managers, preprocessors and quotient postprocessors, not "
                            + type(part).__name__)
        setattr(self, slot, part)
        return self

    def __lshift__(self, ranker):
        """`ranker >> filter`: the ranker's outcome becomes this filter's personalization (abstract_filters.py:97-101)."""
        if isinstance(ranker, NodeRanking):
            self.personalization_transform = ranker
            return ranker
        raise Exception("only node ranking algorithms can be chained into a graph filter")

    def _reference(self):
        return "graph filter"

    def cite(self):                                                               # abstract_filters.py:82-86
        own = super().cite()
        upstream = self.personalization_transform
        if isinstance(upstream, Tautology) and upstream.ranker is None:
            return own
        return upstream.cite() + "\n  passed to " + own


# =====================================================================================================
# recursive filters
# =====================================================================================================
class RecursiveGraphFilter(GraphFilter):
    """abstract_filters.py:104-149: ranks = formula(G, ranks), optional L1 quotient per step."""

    def __init__(self, use_quotient=True, converge_to_eigenvectors=False, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.use_quotient, self.converge_to_eigenvectors = use_quotient, converge_to_eigenvectors

    def _quotient(self, ranks):
        """What follows the formula in every step (abstract_filters.py:130-134): a postprocessor in the quotient's place,
        the plain division by the sum, or nothing."""
        rule = self.use_quotient
        if isinstance(rule, Postprocessor):
            return rule(ranks)
        return backend.safe_div(ranks, backend.sum(ranks)) if rule else ranks.np

    def _step(self, M, personalization, ranks, *args, **kwargs):
        outcome = self._formula(M, personalization, ranks, *args, **kwargs)
        ranks.np = outcome.np if isinstance(outcome, GraphSignal) else outcome
        ranks.np = self._quotient(ranks)
        if self.converge_to_eigenvectors:                   # the personalization follows the iterate (abstract_filters.py:135-136)
            personalization.np = ranks.np

    def references(self):
        extra = ["unbiased convergence to the eigenvector"] if self.converge_to_eigenvectors else []
        return super().references() + extra

    def _formula(self, M, personalization, ranks, *args, **kwargs):
        raise Exception("Use a derived class of RecursiveGraphFilter that implements the _formula method")

    def _plain_quotient(self):
        return (self.use_quotient is None or isinstance(self.use_quotient, (bool, int))) \
            and not self.converge_to_eigenvectors

    def _walk_batch_graph(self, cls, graph, args, kwargs, allowed=(), f64=False):
        """_batch_graph for the walks of class `cls`: also the plain quotient and the class's own formula, step and start."""
        if not self._plain_quotient() or type(self)._formula is not cls._formula or type(self)._step is not RecursiveGraphFilter._step \
                or type(self)._start is not cls._start:
            return None
        return self._batch_graph(graph, args, kwargs, allowed, f64)

    def _run_recursive(self, entry, g, cfg, ranks, *vectors):
        if cfg is None or g is None or g.shape[0] != g.shape[1]:
            return False
        x = ranks.np
        if not isinstance(x, DeviceVector):
            return False
        if isinstance(x, LazyVector):
            x = x._writable()              # the engine updates the iterate in place: an expression becomes memory of its own first
        x._before_write()
        res = L.LoopResult()
        L.check(entry(g._h, *[v._h for v in vectors], x._h, C.byref(cfg), C.byref(res)))
        if cfg.in_norm < 0 and res.in_norm == 0:
            return "zero"                  # an all-zero personalization: nothing was run, nothing is counted
        ranks.np = x                       # updated in place by the engine; drops the host mirror
        self.last_loop = dict(iterations=res.iterations, converged=bool(res.converged), spmv=res.spmv_count,
                              last_error=res.last_error, loop_ms=res.loop_ms, flags=res.flags)
        self.convergence.finish_device_loop(res.iterations, res.converged)
        return True


class PageRank(RecursiveGraphFilter):
    """adhoc.py:9-46: r <- alpha * M^T r + (1 - alpha) * p."""

    def __init__(self, alpha=0.85, *args, dtype=None, retire=False, **kwargs):
        """retire (an extension of this backend; also an attribute): True, or a list of strictly descending live-column counts below 64
        (True: 32, 16, 8, 4) -- propagate's multi-seed runs retire their converged columns inside the loop (include/pgh_retire.h) and
        ``last_batches`` carries the run's report under "stages".  A column of such a run may differ from the plain batch's in its last
        bits.  graph_dropout takes the plain loop.
        dtype="float64" (an extension of this backend): the loop keeps its iterates, sums, quotient and residual in f64 on the engine's
        f64 image (pgh_ppr_run_f64) and the tolerance is clamped at fp64 eps like the reference's numpy backend
        (pygrank/core/backend/numpy.py:84-86) instead of fp32 eps -- e.g. tol=1e-9 as in the reference's tests/test_filters.py:189,194.
        An exactness mode (one host look per step); personalization and ranks stay f32 vectors."""
        self.alpha = alpha
        self.retire = retire
        super().__init__(*args, dtype=dtype, **kwargs)

    def _reference(self):
        return f"personalized PageRank (restart probability {1 - self.alpha:.3g})"

    def _formula(self, M, personalization, ranks, *args, **kwargs):               # adhoc.py:34-36
        return backend.conv(ranks, M) * self.alpha + personalization * (1 - self.alpha)

    def _fused_loop(self, M, personalization, ranks, out_scale, *args, **kwargs):
        if args or kwargs or not self._plain_quotient() or type(self)._formula is not PageRank._formula \
                or type(self)._step is not RecursiveGraphFilter._step:
            return False
        cfg = self._loop_cfg(self.alpha, bool(self.use_quotient), out_scale)
        p = personalization.np
        if not isinstance(p, DeviceVector):
            return False
        if self.dtype == "float64" and cfg is None:
            raise Exception("PageRank(dtype='float64') needs a stopping rule the engine evaluates (Mabs / L1 / MaxDifference / 'iters')")
        g = _device_graph(M)
        if cfg is not None and self._f64_wanted() and _f64_image_usable(g):
            return self._run_recursive(L.lib().pgh_ppr_run_f64, g, self._f64_cfg(cfg), ranks, p)
        return self._run_recursive(L.lib().pgh_ppr_run, g, cfg, ranks, p)

    fused_dropout = True          # False (on an instance): rank(..., graph_dropout=) takes the hook protocol, one engine call per primitive

    def _fused_rank(self, personalization, *args, dropout=0, **kwargs):
        if args or kwargs or not self._plain_quotient() or type(self)._formula is not PageRank._formula \
                or type(self)._step is not RecursiveGraphFilter._step or type(self)._prepare_graph is not GraphFilter._prepare_graph:
            return None
        if dropout and not (self.fused_dropout and 0 < dropout < 1):
            return None
        if self.dtype == "float64" and dropout:
            raise Exception("PageRank(dtype='float64') has no graph_dropout route")
        p = personalization.np
        cfg = self._loop_cfg(self.alpha, bool(self.use_quotient), -1.0 if self.preserve_norm else 1.0)     # -1: times the norm
        if cfg is None or not isinstance(p, DeviceVector):
            return None
        M = self.preprocessor(personalization.graph)
        g = _device_graph(M)
        if g is None or g.shape[0] != g.shape[1] or g.shape[0] != len(p):
            return None
        cfg.in_norm, cfg.start_from_p = -1.0, 1            # the engine sums |p| itself
        before = dict(vars(self.convergence))
        self.convergence.start()
        ranks = to_signal(personalization, DeviceVector.empty(len(p)))
        entry = L.lib().pgh_ppr_run
        if self._f64_wanted() and not dropout and _f64_image_usable(g):
            entry, cfg = L.lib().pgh_ppr_run_f64, self._f64_cfg(cfg)
        if dropout:
            # the masks the hook protocol would draw (abstract_filters.py:57-62): one for _start, one per step, one for _end -- step k
            # runs on the (k + 1)-th of them, so both routes compute the same thing from the same seed
            from pygrank_amd.backend import hip as _hip
            first = _hip.peek_dropout_seed()
            lib, rate, seed0 = L.lib(), float(dropout), int(first) + 1

            def entry(gh, ph, xh, cfg_ref, res_ref):
                return lib.pgh_ppr_run_dropout(gh, ph, xh, cfg_ref, rate, seed0, res_ref)
        outcome = self._run_recursive(entry, g, cfg, ranks, p)
        if outcome == "zero":                              # abstract_filters.py:53-54: returned before the manager is started
            vars(self.convergence).update(before)
            return personalization
        if dropout and outcome:
            # ... and leaves the seed counter where the hook protocol would: it draws iterations + 1 masks (_start, iterations - 1
            # steps, _end), however early the tolerance stopped the run; a run that fell back (outcome False) has drawn none
            _hip.take_dropout_seeds(int(self.convergence.iteration) + 1)
        return ranks if outcome else None

    def propagate(self, graph, features, *args, **kwargs):
        """signals.py:225-226 semantics (one rank() per feature column), run as multi-seed batches of up to 64 columns
        through pgh_ppr_run_batch: the adjacency is streamed once per iteration for the whole batch and every column
        keeps its own quotient, residual and stopping iteration.  With f64_batch=True a run that wants f64 iterates goes through
        pgh_ppr_run_batch_f64 (include/pgh_batch64.h) the same way; graph_dropout, a library without that entry and a declined call
        take the route below."""
        from pygrank_amd.device import DeviceMatrix
        g64 = self._walk_batch_graph(PageRank, graph, args, kwargs, f64=True)
        entry64 = L.entry("pgh_ppr_run_batch_f64") if g64 is not None else None
        if entry64 is not None:
            out = _propagate_in_batches64(self, features, self._loop_cfg(self.alpha, bool(self.use_quotient), 1.0),
                                          lambda P, R, cfg_ref, scales, res, norms: entry64(g64._h, P._h, R._h, cfg_ref, scales, res, norms),
                                          raw=True)
            if out is not None:
                return out
        cfg = self._loop_cfg(self.alpha, bool(self.use_quotient), 1.0)
        dropout = float(kwargs.get("graph_dropout", 0) or 0)
        only_dropout = not kwargs or (set(kwargs) == {"graph_dropout"} and 0 <= dropout < 1)
        batched = (not args and only_dropout and cfg is not None and self._plain_quotient()
                   and type(self)._formula is PageRank._formula and type(self)._step is RecursiveGraphFilter._step
                   and isinstance(self.personalization_transform, Tautology) and self.personalization_transform.ranker is None)
        if self.dtype == "float64":
            #  the multi-seed loop is an f32 loop: a ranker that promises f64 iterates and an fp64-eps tolerance runs its columns
            # one by one through pgh_ppr_run_f64 (signals.py:225-226 as written) instead of silently changing precision
            batched = False
        M = self.preprocessor(graph) if batched else None
        g = _device_graph(M) if batched else None
        if g is None or g.shape[0] != g.shape[1]:
            return super().propagate(graph, features, *args, **kwargs)
        F = features if isinstance(features, DeviceMatrix) else backend.to_primitive(features)
        if not isinstance(F, DeviceMatrix):
            F = DeviceMatrix.from_columns([F])
        self.last_batches = []
        out = DeviceMatrix.empty(F.n, F.b) if F.b > 64 else None
        for start, chunk in F.chunks():
            norms = chunk.col_abssum()                                            # abstract_filters.py:52-55 per column
            P = chunk.div_cols(norms)                                             # zero columns stay zero (:53-54)
            R = DeviceMatrix.empty(chunk.n, chunk.b)
            results = (L.LoopResult * chunk.b)()
            scales = (C.c_double * chunk.b)(*[(float(nrm) if self.preserve_norm else 1.0) for nrm in norms])
            cfg.start_from_p = 1                                                  # ranks start as a copy of p (:56)
            self.convergence.start()
            stages = None
            if dropout > 0:
                # graph_dropout(M, rate) of every step (abstract_filters.py:59-62) inside the batch kernel: one mask per step,
                # seeds reserved up front (the loop stops on the device)
                from pygrank_amd.backend import hip as _hip
                seed0 = _hip.take_dropout_seeds(max(int(cfg.max_iters), 1))
                L.check(L.lib().pgh_ppr_run_batch_dropout(g._h, P._h, R._h, C.byref(cfg), scales, dropout, seed0, results))
            else:
                status, stages = _batch_call(self, L.lib().pgh_ppr_run_batch, "pgh_ppr_run_batch_retire",
                                             (g._h, P._h, R._h, C.byref(cfg), scales, results))
                L.check(status)
            self.last_batches.append(_batch_info(results, stages))
            for r, nrm in zip(results, norms):
                if nrm != 0:
                    self.convergence.finish_device_loop(r.iterations, r.converged)   # raises like the per-column run would
            if out is None:
                return R
            out.set_cols(start, R)
        return out


class AbsorbingWalks(RecursiveGraphFilter):
    """adhoc.py:125-174: partially absorbing random walks."""

    def __init__(self, alpha=1 - 1.E-6, *args, retire=False, **kwargs):
        """retire: as PageRank's (propagate's multi-seed runs retire their converged columns inside the loop)."""
        super().__init__(*args, **kwargs)
        self.alpha = alpha
        self.retire = retire

    def _reference(self):
        return f"partially absorbing random walks (absorption scale {(1 - self.alpha) / self.alpha:.3g})"

    def _start(self, M, personalization, ranks, absorption=None, **kwargs):       # adhoc.py:157-159
        self.absorption = to_signal(personalization.graph, absorption) * ((1 - self.alpha) / self.alpha)
        self.degrees = backend.degrees(M)

    def _end(self, *args, **kwargs):
        super()._end(*args, **kwargs)
        del self.absorption
        del self.degrees

    def _formula(self, M, personalization, ranks, *args, **kwargs):               # adhoc.py:166-169
        return (backend.conv(ranks, M) * self.degrees + personalization * self.absorption) / \
            (self.absorption + self.degrees)

    def _fused_loop(self, M, personalization, ranks, out_scale, *args, absorption=None, **kwargs):
        if args or kwargs or not self._plain_quotient() or type(self)._formula is not AbsorbingWalks._formula \
                or type(self)._step is not RecursiveGraphFilter._step:
            return False
        cfg = self._loop_cfg(self.alpha, bool(self.use_quotient), out_scale)
        p = personalization.np
        if not isinstance(p, DeviceVector):
            return False
        lam = (to_signal(personalization.graph, absorption) * ((1 - self.alpha) / self.alpha)).np
        g = _device_graph(M)
        if cfg is not None and self._f64_wanted() and _f64_image_usable(g):
            cfg, p = self._f64_operands(cfg, p)
            return self._run_recursive(L.lib().pgh_absorb_run_f64, g, cfg, ranks, p, lam)
        return self._run_recursive(L.lib().pgh_absorb_run, g, cfg, ranks, p, lam)

    def propagate(self, graph, features, *args, **kwargs):
        """signals.py:225-226 (one rank() per feature column, each with the same `absorption=`) as multi-seed batches of up to 64
        columns through pgh_absorb_run_batch (include/pgh_batch.h) wherever a single rank() would run the f32 loop of pgh_absorb_run;
        every column keeps its own quotient, residual and stopping iteration.  With f64_batch=True a run that wants f64 iterates goes
        through pgh_absorb_run_batch_f64 (include/pgh_batch64.h) the same way.  The column loop otherwise."""
        g64 = self._walk_batch_graph(AbsorbingWalks, graph, args, kwargs, allowed=("absorption",), f64=True)
        entry64 = L.entry("pgh_absorb_run_batch_f64") if g64 is not None else None
        if entry64 is not None:
            lam = (to_signal(graph, kwargs.get("absorption")) * ((1 - self.alpha) / self.alpha)).np
            if isinstance(lam, DeviceVector) and len(lam) == g64.shape[0]:
                out = _propagate_in_batches64(self, features, self._loop_cfg(self.alpha, bool(self.use_quotient), 1.0),
                                              lambda P, R, cfg_ref, scales, res, norms: entry64(g64._h, P._h, lam._h, R._h, cfg_ref, scales, res,
                                                                                                norms), raw=True)
                if out is not None:
                    return out
        g = self._walk_batch_graph(AbsorbingWalks, graph, args, kwargs, allowed=("absorption",))
        entry = L.entry("pgh_absorb_run_batch") if g is not None else None
        if entry is not None:
            lam = (to_signal(graph, kwargs.get("absorption")) * ((1 - self.alpha) / self.alpha)).np
            if isinstance(lam, DeviceVector) and len(lam) == g.shape[0]:
                cfg = self._loop_cfg(self.alpha, bool(self.use_quotient), 1.0)
                out = _propagate_in_batches(self, features, cfg, lambda P, R, cfg_ref, scales, res: _batch_call(
                    self, entry, "pgh_absorb_run_batch_retire", (g._h, P._h, lam._h, R._h, cfg_ref, scales, res)))
                if out is not None:
                    return out
        return super().propagate(graph, features, *args, **kwargs)


class LFPR(RecursiveGraphFilter):
    """adhoc.py:196-314: the locally fair PageRank of [tsioutsiouliklis2021fairness].  With outR = conv(sensitive, W) and
    outB = conv(1 - sensitive, W) on the RAW adjacency W, a row scaling d and two residual vectors dR, dB (LFPR.normalization, _start) a
    step is ``(conv(ranks, Q W) + deltaR xR + deltaB xB) alpha + personalization (1 - alpha)`` with Q = diag(d), deltaR = sum(ranks dR),
    deltaB = sum(ranks dB); _end takes ``personalization (1 - alpha)`` off again.

    The reference builds Q @ W on the host and normalises it on every rank(), because Q depends on the sensitive attribute.  Here
    conv(x, Q W) = W^T (d x): the loop runs on the raw-adjacency device graph (normalization="none", the image Conductance uses) and
    scales the iterate by d in front of each product, so the device graph does not depend on `sensitive`.

    preprocessor: by default ``preprocessor(normalization="none", assume_immutability=False)`` as in the reference, which overwrites
    whatever preprocessor it is given.  An extension of this backend: a caller may hand in
    ``preprocessor=pg.preprocessor(normalization="none", assume_immutability=True)`` and reuse the device image over many rank() calls
    with different sensitive groups.  The normalization must stay "none".  (redistributor="original" still builds its col-normalised
    graph per rank(), as adhoc.py:270-274 does.)

    fused=True (the default; an extension): per step ONE pgh_resident_step on the resident iterate, ONE pgh_lfpr_close
    (include/pgh_lfpr.h) and, on images with a gather form, one pgh_resident_gather; two host reads.  fused=False: the reference's
    _formula in backend primitives on the same graph.  The primitives also run where the library lacks the entries, the image has no
    resident form, an entry declines, use_quotient is a postprocessor, converge_to_eigenvectors is set, the convergence manager is
    not a plain ConvergenceManager with Mabs / L1 / MaxDifference / "iters", or graph_dropout / warm_start is given.  Both routes
    share _start.  Iterates are f32 on either route: a tolerance below fp32 eps is clamped there (convergence.py:101).

    Not here: f64 iterates, a batch of sensitive attributes, partitioned graphs."""

    def __init__(self, alpha=0.85, redistributor=None, target_prule=1, fix_personalization=True, *args, fused=True, **kwargs):
        self.alpha = alpha
        if kwargs.get("preprocessor") is None:
            kwargs["preprocessor"] = default_preprocessor(assume_immutability=False, normalization="none")
        self.target_prule = target_prule
        self.redistributor = redistributor
        self.fix_personalization = fix_personalization
        self.fused = fused
        self._warm = False
        super().__init__(*args, **kwargs)

    def rank(self, graph=None, personalization=None, warm_start=None, graph_dropout=0, *args, **kwargs):
        self._warm = warm_start is not None
        try:
            return super().rank(graph, personalization, warm_start, graph_dropout, *args, **kwargs)
        finally:
            self._warm = False

    def _prepare_graph(self, graph, personalization, sensitive, *args, **kwargs):    # adhoc.py:243-254
        personalization = to_signal(graph, personalization)
        sensitive = to_signal(personalization, sensitive)
        self.sensitive = sensitive
        self.phi = backend.sum(sensitive.np) / backend.length(sensitive.np) * self.target_prule
        return graph

    def _original_ranks(self, personalization):                                      # adhoc.py:268-276
        rule = self.redistributor
        if rule is None or (isinstance(rule, str) and rule == "uniform"):
            return None
        if isinstance(rule, str) and rule == "original":
            cm = self.convergence
            inner = PageRank(alpha=self.alpha, tol=cm.tol, convergence=cm,
                             preprocessor=default_preprocessor(assume_immutability=False, normalization="col"))(personalization).np
            cm.last_ranks = inner            # what the inner loop's last has_converged call leaves behind in the shared manager
            return inner
        if isinstance(rule, NodeRanking):
            return rule(personalization).np
        raise Exception("LFPR redistributor: None, 'uniform', 'original' or a node ranking algorithm, not " + repr(rule))

    def _start(self, M, personalization, ranks, sensitive, *args, **kwargs):         # adhoc.py:227-241, 256-282
        s = to_signal(ranks, sensitive).np
        phi = float(backend.sum(s) / backend.length(s) * self.target_prule)
        out_r, out_b = backend.conv(s, M), backend.conv(1. - s, M)
        original = self._original_ranks(personalization)
        setup = L.entry("pgh_lfpr_setup") if self.fused else None
        if setup is not None and all(isinstance(v, DeviceVector) for v in (s, out_r, out_b)) \
                and (original is None or isinstance(original, DeviceVector)):
            made = [DeviceVector.empty(len(s)) for _ in range(5)]
            sums = (C.c_double * 2)()
            status = setup(s._h, out_r._h, out_b._h, None if original is None else original._h, phi, *[v._h for v in made], sums)
            if L.accepted(status):
                self.d, self.dR, self.dB, self.xR, self.xB = made
                self.sum_xR, self.sum_xB = float(sums[0]), float(sums[1])
                return
        case1 = out_r < (out_r + out_b) * phi
        case2 = (1 - case1) * (out_r != 0)
        case3 = (1 - case1) * (1 - case2)
        inv_r, inv_b = backend.safe_inv(out_r), backend.safe_inv(out_b)
        self.d = case1 * inv_b * (1 - phi) + case2 * inv_r * phi + case3
        self.dR = case1 * (phi - (1 - phi) * inv_b * out_r) + case3 * phi
        self.dB = case2 * ((1 - phi) - phi * inv_r * out_b) + case3 * (1 - phi)
        # (xR, xB stay un-normalised with their sums beside them: deltaR * xR / sum(xR) is formed per step on either route)
        self.xR = s * 1. if original is None else original * s
        self.xB = 1. - s if original is None else original * (1. - s)
        self.sum_xR, self.sum_xB = float(backend.sum(self.xR)), float(backend.sum(self.xB))

    def _formula(self, M, personalization, ranks, sensitive, *args, **kwargs):       # adhoc.py:284-293
        # (alpha is multiplied into the two coefficients and the rank-two correction is added as ONE vector: every addition of a
        # vector rounds the seeds' large entries to f32 once more, and _end takes most of such an entry off again)
        x = ranks.np
        cR = self.alpha * backend.safe_div(backend.sum(x * self.dR), self.sum_xR)
        cB = self.alpha * backend.safe_div(backend.sum(x * self.dB), self.sum_xB)
        correction = self.xR * cR + self.xB * cB
        return backend.conv(x * self.d, M) * self.alpha + personalization.np * (1 - self.alpha) + correction

    def _end(self, M, personalization, ranks, *args, **kwargs):                      # adhoc.py:295-305
        ranks.np = ranks.np - personalization.np * (1 - self.alpha)
        self._forget()
        super()._end(M, personalization, ranks, *args, **kwargs)

    def _forget(self):
        for name in ("xR", "xB", "dR", "dB", "d", "sum_xR", "sum_xB", "sensitive", "phi"):
            if hasattr(self, name):
                delattr(self, name)

    def references(self):                                                             # adhoc.py:307-314
        refs = super().references()
        refs[0] = "fairness-aware PageRank \\cite{tsioutsiouliklis2021fairness}"
        refs.insert(1, f"diffusion rate {self.alpha:.3f}")
        redistributor = "uniform" if self.redistributor is None else self.redistributor
        redistributor = redistributor if isinstance(redistributor, str) else redistributor.cite()
        refs.insert(2, f"{redistributor} rank redistribution strategy")
        return refs

    def _fused_route(self, M, personalization):
        """(device graph, pgh_lfpr_close) when this run takes the fused route, else None."""
        close = L.entry("pgh_lfpr_close") if self.fused and not self._warm else None
        cm = self.convergence
        g = _device_graph(M)
        if close is None or g is None or g.shape[0] != g.shape[1] or g.shape[0] == 0 or not self._plain_quotient() \
                or type(cm) is not ConvergenceManager or cm.device_error_kind() is None \
                or not isinstance(personalization.np, DeviceVector) or len(personalization.np) != g.shape[0]:
            return None
        if any(getattr(type(self), hook) is not getattr(LFPR, hook) for hook in ("_formula", "_start", "_end")) \
                or type(self)._step is not RecursiveGraphFilter._step:
            return None
        return (g, close) if g._resident_lengths() else None

    def _primitive_loop(self, M, personalization, ranks, out_scale, args, kwargs):
        """The rest of a run whose _start has run, in backend primitives (an entry declined)."""
        while not self.convergence.has_converged(ranks.np):
            self._step(M, personalization, ranks, *args, **kwargs)
        self._end(M, personalization, ranks, *args, **kwargs)
        if out_scale != 1.0:
            ranks.np = ranks.np * out_scale
        return True

    def _fused_loop(self, M, personalization, ranks, out_scale, *args, **kwargs):
        route = self._fused_route(M, personalization)
        if route is None:
            return False
        g, close = route
        self._start(M, personalization, ranks, *args, **kwargs)
        operands = (self.d, self.dR, self.dB, self.xR, self.xB)
        cm = self.convergence
        self.last_loop = None
        if not all(type(v) is DeviceVector for v in operands):          # pgh_lfpr_setup declined
            return self._primitive_loop(M, personalization, ranks, out_scale, args, kwargs)
        if cm.has_converged(ranks.np):
            return self._finish_fused(M, personalization, ranks, out_scale, args, kwargs)
        lib = L.lib()
        n, n_int, n_gather = len(personalization.np), g._n_int, g._n_gather

        def bring(vec):
            out = DeviceVector.empty(n_int)
            L.check(lib.pgh_resident_in(g._h, vec._h, 0.0, out._h, None))
            return out
        p_int, x = bring(personalization.np), bring(ranks.np)
        d, dR, dB, xR, xB = [bring(v) for v in operands]
        u, y = DeviceVector.empty(n_int), DeviceVector.empty(n_int)
        ug = DeviceVector.empty(n_gather) if n_gather else None
        # (on images with a gather form the step entry insists on writing the gather form of ITS outcome y0, which nobody reads here:
        # the next product gathers from u = d * y, whose gather form pgh_resident_gather makes -- one wasted n_gather write per step)
        yg = DeviceVector.empty(n_gather) if n_gather else None
        L.check(lib.pgh_ewise_vv(L.MUL, x._h, d._h, u._h))
        got = C.c_double()
        L.check(lib.pgh_dot(x._h, dR._h, C.byref(got)))
        delta_r = got.value
        L.check(lib.pgh_dot(x._h, dB._h, C.byref(got)))
        delta_b = got.value
        alpha, quotient = float(self.alpha), bool(self.use_quotient)
        kind = cm.device_error_kind()
        counts_only = kind == L.ERR_ITERS
        tol = float(cm.effective_tolerance())
        sums = (C.c_double * 5)()
        x_scale, step_sums, err, steps, converged = 1.0, [], float("nan"), 0, False
        while True:
            if ug is not None:
                L.check(lib.pgh_resident_gather(g._h, u._h, ug._h))
            L.check(lib.pgh_resident_step(g._h, 1, u._h, None if ug is None else ug._h, alpha * x_scale, p_int._h, 1.0 - alpha, None, None,
                                          y._h, None if yg is None else yg._h, C.byref(got)))
            cR = alpha * backend.safe_div(delta_r, self.sum_xR)
            cB = alpha * backend.safe_div(delta_b, self.sum_xB)
            predicted = got.value + cR * self.sum_xR + cB * self.sum_xB
            y_scale = backend.safe_inv(predicted) if quotient else 1.0
            status = close(y._h, x._h, x_scale, xR._h, xB._h, d._h, dR._h, dB._h, cR, cB, y_scale,
                           L.ERR_L1 if counts_only else kind, y._h, u._h, sums)
            if status == L.DECLINED:
                # the iterate before this step goes back to the caller's ids; the step is taken again there
                out = DeviceVector.empty(n)
                L.check(lib.pgh_resident_out(g._h, x._h, x_scale, out._h))
                ranks.np = out
                cm.last_ranks = out
                self._step(M, personalization, ranks, *args, **kwargs)
                return self._primitive_loop(M, personalization, ranks, out_scale, args, kwargs)
            L.check(status)
            steps += 1
            total = sums[0]
            scale = backend.safe_inv(total) if quotient else 1.0
            err = sums[3] if kind == L.ERR_LINF else sums[3] + (scale - y_scale) * sums[4]
            if kind == L.ERR_MABS:
                err /= n
            delta_r, delta_b = scale * sums[1], scale * sums[2]
            step_sums.append(total)
            x, y, x_scale = y, x, scale
            # ConvergenceManager.has_converged (convergence.py:77-101), asked before the next step
            cm.iteration += 1
            cm._stamp()
            if cm.iteration >= cm.max_iters:
                if not counts_only and cm.iter_exception is not None:
                    self.last_loop = dict(iterations=cm.iteration, converged=False, steps=steps, last_error=err, step_sums=step_sums)
                    raise cm.iter_exception(cm._out_of_iterations())
                break
            if not counts_only and cm.iteration % cm.end_modulo == 0 and err <= tol:
                converged = True
                break
        self.last_loop = dict(iterations=cm.iteration, converged=converged, steps=steps, last_error=err, step_sums=step_sums)
        # _end in the id space: x_scale x - (1 - alpha) p = x_scale (x - (1 - alpha) / x_scale p), the bracket by one more close (f64, ONE
        # rounding).  _end takes most of a seed's entry off again, so whatever was done to that entry before shows in what is left: the
        # step's epilogue applied (1 - alpha) as an f32 coefficient, and the same f32 value is taken off here.  x_scale and
        # preserve_norm ride on the way out of the id space, which runs once
        out = DeviceVector.empty(n)
        status = L.DECLINED
        if x_scale != 0.0:
            # the close as an f64 axpy, y <- x + c p:  y0 = x,  xR = p with cR = c,  xB with cB = 0 adds nothing;  the residual operand
            # (x again), d / dR / dB, the five sums and u are by-products nobody reads
            c = -float(np.float32(1.0 - alpha)) / x_scale
            status = close(x._h, x._h, 1.0, p_int._h, p_int._h, d._h, dR._h, dB._h, c, 0.0, 1.0, L.ERR_L1, y._h, u._h, sums)
        if status == L.DECLINED:                           # (a zero quotient, or the entry declined: _end in backend primitives)
            L.check(lib.pgh_resident_out(g._h, x._h, x_scale, out._h))
            ranks.np = out
            return self._finish_fused(M, personalization, ranks, out_scale, args, kwargs)
        L.check(status)
        L.check(lib.pgh_resident_out(g._h, y._h, x_scale * out_scale, out._h))
        ranks.np = out
        self._forget()
        return True

    def _finish_fused(self, M, personalization, ranks, out_scale, args, kwargs):
        self._end(M, personalization, ranks, *args, **kwargs)
        if out_scale != 1.0:
            ranks.np = ranks.np * out_scale
        return True


class SymmetricAbsorbingRandomWalks(RecursiveGraphFilter):
    """adhoc.py:317-369: symmetric partially absorbing random walks.  With d = degrees(M) and the per-node absorption
    a = (1 + sqrt(1 + 4 d)) / 2 a step is ``conv(ranks / a, M) * d / (a + d) + personalization * a / (a + d)``
    (``alpha`` is accepted for signature compatibility and, as in the reference, does not enter the formula)."""

    def __init__(self, alpha=0.5, *args, retire=False, **kwargs):
        """retire: as PageRank's (propagate's multi-seed runs retire their converged columns inside the loop)."""
        super().__init__(*args, **kwargs)
        self.alpha = alpha
        self.retire = retire

    def _reference(self):
        return "symmetric partially absorbing random walks"

    def _start(self, M, personalization, ranks, **kwargs):                        # adhoc.py:348-353
        d = backend.degrees(M)
        a = ((d * 4 + 1) ** 0.5 + 1) / 2
        self._walk = dict(pre=1. / a, post=d / (a + d), skew=a / (a + d))

    def _end(self, *args, **kwargs):
        super()._end(*args, **kwargs)
        self._walk = None

    def _formula(self, M, personalization, ranks, *args, **kwargs):               # adhoc.py:362-364
        w = self._walk
        return backend.conv(ranks * w["pre"], M) * w["post"] + personalization * w["skew"]

    def _fused_loop(self, M, personalization, ranks, out_scale, *args, **kwargs):
        if args or kwargs or not self._plain_quotient() or type(self)._formula is not SymmetricAbsorbingRandomWalks._formula \
                or type(self)._step is not RecursiveGraphFilter._step or type(self)._start is not SymmetricAbsorbingRandomWalks._start:
            return False
        cfg = self._loop_cfg(self.alpha, bool(self.use_quotient), out_scale)
        p = personalization.np
        g = _device_graph(M)
        if not isinstance(p, DeviceVector) or g is None or "row-major" in g.format():     # PGH_FORMAT=csr: generic route
            return False
        if cfg is not None and self._f64_wanted() and _f64_image_usable(g):
            cfg, p = self._f64_operands(cfg, p)
            return self._run_recursive(L.lib().pgh_sarw_run_f64, g, cfg, ranks, p)
        return self._run_recursive(L.lib().pgh_sarw_run, g, cfg, ranks, p)

    def propagate(self, graph, features, *args, **kwargs):
        """signals.py:225-226 as multi-seed batches of up to 64 columns through pgh_sarw_run_batch (include/pgh_batch.h) wherever a
        single rank() would run the f32 loop of pgh_sarw_run; with f64_batch=True a run that wants f64 iterates goes through
        pgh_sarw_run_batch_f64 (include/pgh_batch64.h) the same way; the column loop otherwise."""
        g64 = self._walk_batch_graph(SymmetricAbsorbingRandomWalks, graph, args, kwargs, f64=True)
        entry64 = L.entry("pgh_sarw_run_batch_f64") if g64 is not None else None
        if entry64 is not None:
            out = _propagate_in_batches64(self, features, self._loop_cfg(self.alpha, bool(self.use_quotient), 1.0),
                                          lambda P, R, cfg_ref, scales, res, norms: entry64(g64._h, P._h, R._h, cfg_ref, scales, res, norms),
                                          raw=True)
            if out is not None:
                return out
        g = self._walk_batch_graph(SymmetricAbsorbingRandomWalks, graph, args, kwargs)
        entry = L.entry("pgh_sarw_run_batch") if g is not None else None
        if entry is not None:
            cfg = self._loop_cfg(self.alpha, bool(self.use_quotient), 1.0)
            out = _propagate_in_batches(self, features, cfg, lambda P, R, cfg_ref, scales, res: _batch_call(
                self, entry, "pgh_sarw_run_batch_retire", (g._h, P._h, R._h, cfg_ref, scales, res)))
            if out is not None:
                return out
        return super().propagate(graph, features, *args, **kwargs)


class LowPassRecursiveGraphFilter(GraphFilter):
    """low_pass.py:61-91: recursive low-pass filter with per-iteration parameters."""

    def __init__(self, params=None, *args, **kwargs):
        if params is None:
            params = [0.9] * 10
        super().__init__(*args, **kwargs)
        self.params = params

    def _step(self, M, personalization, ranks, *args, **kwargs):
        if self.convergence.iteration > len(self.params):
            return 0
        param = self.params[self.convergence.iteration - 1]
        if param == 0:
            return ranks
        if param == 1:
            ranks.np = backend.conv(ranks, M).np
            return ranks
        ranks.np = (backend.conv(ranks, M) * param + personalization * (1 - param)).np


class ImpulseGraphFilter(GraphFilter):
    """low_pass.py:29-58: filter defined by its impulse-response parameters."""

    def __init__(self, params=None, *args, **kwargs):
        if params is None:
            params = [0.9] * 10
        super().__init__(*args, **kwargs)
        self.params = params

    def _step(self, M, personalization, ranks, *args, **kwargs):
        if self.convergence.iteration > len(self.params):
            return 0
        param = self.params[self.convergence.iteration - 1]
        if param == 0:
            return ranks
        if param == 1:
            ranks.np = backend.conv(ranks, M).np
            return ranks
        ranks.np = (backend.conv(ranks, M) * param + ranks * (1 - param)).np


# =====================================================================================================
# closed-form (polynomial) filters
# =====================================================================================================
class _PowerSlab:
    """The device form of the optimisation dict (abstract_filters.py:232-246): the powers
    {(M^T)^k p, k = 0, 1, ...} of ONE personalization as the columns of [n, 64] slabs in HBM (as many slabs as the
    longest expansion asked for needs), extended on demand (one conv per new column), with the L1 and L-inf norm of every
    column on the host.  A filter evaluated from it costs one pass over the slabs (pgh_mat_gemv) instead of one SpMV
    per term, and P filters cost one pass as well (pgh_mat_gemm) -- what a tuner that probes hundreds of coefficient
    vectors on the same personalization (autotune/parameterized.py:94-145) needs."""
    WIDTH = 64
    MAX_TERMS = 4096          # 64 slabs; beyond that the step-by-step route takes over

    def __init__(self, graph, p, chebyshev=False):
        self.graph = graph
        self.n = len(p)
        self.slabs = []
        self.count = 0
        self.l1, self.linf = [], []
        self._last = None
        self.chebyshev = bool(chebyshev)
        self._p = p
        if not self.chebyshev:
            self._push(p)

    def _push(self, col):
        from pygrank_amd.device import DeviceMatrix
        slab, at = divmod(self.count, self.WIDTH)
        if slab == len(self.slabs):
            self.slabs.append(DeviceMatrix.empty(self.n, self.WIDTH))
        self.slabs[slab].set_column(at, col)
        self.l1.append(float(col.abssum()))
        self.linf.append(float(backend.max(backend.abs(col))) if len(col) else 0.0)
        self._last = col
        self.count += 1

    def ensure(self, columns):
        """Makes the first `columns` powers available; False when that is more than a slab set may hold."""
        if columns > self.MAX_TERMS:
            return False
        if self.chebyshev:
            return self._ensure_chebyshev(columns)
        while self.count < columns:
            self._push(self.graph.conv(self._last))
        return True

    def _ensure_chebyshev(self, columns):
        """The terms T_k of the reference's "chebyshev" recurrence (abstract_filters.py:216-224) as slab columns: they come out
        of the engine's f64 recurrence (pgh_poly_terms) 32 at a time -- a term rounded to f32 must not feed the next ones, so an
        extension recomputes from T_1."""
        from pygrank_amd.device import DeviceMatrix
        while self.count < columns:
            slab, at = divmod(self.count, self.WIDTH)
            if slab == len(self.slabs):
                self.slabs.append(DeviceMatrix.empty(self.n, self.WIDTH))
            chunk = min(32, self.WIDTH - at)
            rc = L.lib().pgh_poly_terms(self.graph._h, self._p._h, 1, self.count, chunk, self.slabs[slab]._h, at)
            if rc != 0:
                return False                                 # no blocked f64 image for this graph: the step-by-step route
            for j in range(chunk):
                col = self.slabs[slab].column(at + j)
                self.l1.append(float(col.abssum()))
                self.linf.append(float(backend.max(backend.abs(col))) if len(col) else 0.0)
            self.count += chunk
        return True

    def combine(self, coeffs):
        """sum_k coeffs[k] * power_k as a DeviceVector (coeffs: 1-D, at most `count` long)."""
        c = np.asarray(coeffs, dtype=np.float64)
        out = None
        for slab, first in zip(self.slabs, range(0, len(c), self.WIDTH)):
            part = slab.gemv(c[first:first + self.WIDTH])
            out = part if out is None else out + part
        return out if out is not None else backend.repeat(0.0, self.n)

    def combine_many(self, coeff_matrix):
        """[terms, P] coefficients -> [n, P] slab of results (P <= 64): every slab is read once for all P probes."""
        c = np.asarray(coeff_matrix, dtype=np.float64)
        out = None
        for slab, first in zip(self.slabs, range(0, c.shape[0], self.WIDTH)):
            out = slab.gemm(c[first:first + self.WIDTH], out=out, accumulate=out is not None)
        return out


class ClosedFormGraphFilter(GraphFilter):
    """abstract_filters.py:152-270: sum_k c_k (M^T)^k p with Taylor or the reference's "chebyshev" recurrence.

    krylov_dims=k: the filter is evaluated in the k-dimensional Krylov space of the personalization (pygrank_amd/krylov.py; DESIGN.md
    section 17): k products build the Lanczos basis V [n, k] and the k x k matrix H, the expansion then runs on k x k host matrices and
    the ranks are V @ result[:, 0].  As in the reference the outcome is an APPROXIMATION of the filter on the L2-normalised
    personalization, and a basis whose estimated relative error exceeds 0.01 raises.
    fused=True (the default; an extension): the basis comes from the engine's Lanczos step (include/pgh_krylov.h) and, under a plain
    ConvergenceManager with Mabs / L1 / MaxDifference, the residuals of up to 64 iterations come from ONE pgh_krylov_residuals pass
    over the basis and the ranks from ONE pgh_mat_gemv (_krylov_loop).  fused=False, and a library without the entries: the same
    recurrence and the same loop in backend primitives (one gemv and two reductions per iteration).  Any other convergence manager,
    overridden hooks, extra arguments, graph_dropout and a warm start step one iteration at a time through the hooks (one gemv and one
    has_converged each)."""

    def __init__(self, krylov_dims=None, coefficient_type="taylor", optimization_dict=None, *args, fused=True, **kwargs):
        super().__init__(*args, **kwargs)
        self.krylov_dims = krylov_dims
        self.coefficient_type = coefficient_type.lower()
        self.optimization_dict = optimization_dict
        self.fused = fused
        self._active_dict = None

    _FORMS = ("taylor", "chebyshev")

    def _krylov_basis(self, M, personalization):
        """(basis, products it cost this run) for krylov_dims, with the error bound checked (abstract_filters.py:207-210).  With an
        optimisation dict the basis, H and the bound are kept in the active dict, keyed by krylov_dims, while the graph object stays the
        same (as _PowerSlab checks): a second run on the same personalization costs no product."""
        from pygrank_amd import krylov
        k = int(self.krylov_dims)
        g = _device_graph(M)
        store = self._active_dict.setdefault("krylov", {}) if self._active_dict is not None else None
        kept = store.get(k) if store is not None else None
        if kept is not None and g is not None and kept["graph"] is g:
            basis, bound, spmv = kept["basis"], kept["bound"], 0
        else:
            basis = krylov.lanczos(M, personalization.np, k, fused=self.fused)
            bound, spmv = basis.error_bound(), basis.spmv
            if store is not None:
                store[k] = dict(graph=g, basis=basis, bound=bound, powers={})
        self._krylov_powers = store[k]["powers"] if store is not None else None
        if bound > krylov.TOO_ROUGH:
            raise Exception("Krylov approximation with estimated relative error " + str(bound)
                            + " > 0.01 is too rough to be meaningful (try on lager graphs)")
        return basis, spmv

    def _start(self, M, personalization, ranks, *args, **kwargs):
        """abstract_filters.py:196-213: the sum starts empty, the running term is the personalization itself (in the Krylov space:
        the k x k identity; the ranks keep their start value until the first step, as in the reference)."""
        self.coefficient = None
        if self.coefficient_type == "chebyshev":
            self.prev_term = 0
        if self.krylov_dims is not None:
            self.krylov_base, self._krylov_spmv = self._krylov_basis(M, personalization)
            self.krylov_H = self.krylov_base.H
            self.krylov_result = self.krylov_H * 0
            self.Mpower = np.eye(int(self.krylov_dims))
            return
        self.ranks_power = personalization.np
        ranks.np = backend.repeat(0.0, backend.length(ranks.np))

    def _recursion(self, result, next_term, next_coefficient):
        """One term of the expansion (abstract_filters.py:215-230) -> (sum so far, term to propagate next).  "taylor": the
        term as it comes.  "chebyshev", as the reference defines it: from the third iteration on the term is 2 * term -
        previous term, the previous term being whatever was propagated at iteration 2 or later; a zero coefficient skips
        the addition (at iteration 2 and before, the reference adds even then)."""
        form = self.coefficient_type
        if form not in self._FORMS:
            raise Exception("Invalid coefficient type")
        it = self.convergence.iteration
        skip_zero = form == "taylor" or it > 2
        if form == "chebyshev" and it >= 2:
            if it > 2:
                next_term = 2 * next_term - self.prev_term
            self.prev_term = next_term
        if skip_zero and self.coefficient == 0:
            return result, next_term
        return result + next_term * next_coefficient, next_term

    def references(self):
        refs = super().references()
        if self.coefficient_type == "chebyshev":
            refs.append("Chebyshev recurrence of the terms")
        if self.krylov_dims is not None:                                          # abstract_filters.py:190-191, as written
            refs.append("Lanczos acceleration \\cite{susnjara2015accelerated} in the" + str(self.krylov_dims) + "-dimensional Krylov space")
        if self.optimization_dict is not None:
            refs.append("stored powers of the personalization (optimization dictionary)")
        return refs

    def _prepare(self, personalization):                                          # abstract_filters.py:232-239
        if self.optimization_dict is not None:
            pid = obj2id(personalization)
            if pid not in self.optimization_dict:
                self.optimization_dict[pid] = dict()
            self._active_dict = self.optimization_dict[pid]
        else:
            self._active_dict = None

    def _retrieve_power(self, ranks_power, M):                                    # abstract_filters.py:241-246
        if self.krylov_dims is not None:
            # the k x k powers of H, kept per iteration beside the basis they belong to (the reference keys them by the iteration alone)
            powers = getattr(self, "_krylov_powers", None)
            if powers is None:
                return ranks_power @ M
            if self.convergence.iteration not in powers:
                powers[self.convergence.iteration] = ranks_power @ M
            return powers[self.convergence.iteration]
        if self._active_dict is not None:
            if self.convergence.iteration not in self._active_dict:
                self._active_dict[self.convergence.iteration] = backend.conv(ranks_power, M)
            return self._active_dict[self.convergence.iteration]
        return backend.conv(ranks_power, M)

    def _step(self, M, personalization, ranks, *args, **kwargs):
        """abstract_filters.py:248-256: draw the next coefficient, add the running term with it, propagate the term once more."""
        weight = self.coefficient = self._coefficient(self.coefficient)
        if self.krylov_dims is not None:
            self.krylov_result, term = self._recursion(self.krylov_result, self.Mpower, weight)
            ranks.np = self.krylov_base.project(self.krylov_result[:, 0])
            self.Mpower = self._retrieve_power(term, self.krylov_H)
            return
        total, term = self._recursion(ranks.np, self.ranks_power, weight)
        ranks.np = total
        self.ranks_power = self._retrieve_power(term, M)

    _KRYLOV_PER_RUN = ("krylov_base", "krylov_H", "krylov_result", "Mpower", "_krylov_spmv", "_krylov_powers")

    def _end(self, M, personalization, ranks, *args, **kwargs):
        """abstract_filters.py:258-267: the per-run attributes of the expansion go away."""
        if self.krylov_dims is not None:
            cm = self.convergence
            self.last_loop = dict(iterations=cm.iteration, converged=cm.iteration < cm.max_iters, spmv=self._krylov_spmv,
                                  last_error=float("nan"), dims=int(self.krylov_dims), residual_passes=0)
            per_run = list(self._KRYLOV_PER_RUN)
        else:
            per_run = ["ranks_power"]
        per_run += ["coefficient"] + (["prev_term"] if self.coefficient_type == "chebyshev" else [])
        for name in per_run:
            if hasattr(self, name):
                delattr(self, name)
        self._active_dict = None

    def _coefficient(self, previous_coefficient):
        raise Exception("Use a derived class of ClosedFormGraphFilter that implements the _coefficient method")

    def _coefficient_schedule(self, count):
        """c_1 .. c_count exactly as ``_step`` would draw them (``_coefficient`` sees ``convergence.iteration``)."""
        saved = self.convergence.iteration
        coeffs, prev = [], None
        try:
            for it in range(1, count + 1):
                self.convergence.iteration = it
                prev = self._coefficient(prev)
                coeffs.append(float(prev))
        finally:
            self.convergence.iteration = saved
        return coeffs

    def _slab_for(self, M, personalization):
        """The power slab of this personalization inside the active optimisation dict, or None when this configuration
        cannot be served from stored powers."""
        cm = self.convergence
        g = _device_graph(M)
        p = personalization.np
        if type(cm) is not ConvergenceManager or cm.device_error_kind() is None or g is None or g.shape[0] != g.shape[1] \
                or not isinstance(p, DeviceVector) or self.coefficient_type not in self._FORMS or self._active_dict is None:
            return None
        cheb = self.coefficient_type == "chebyshev"
        key = "terms_chebyshev" if cheb else "powers"
        slab = self._active_dict.get(key)
        if not isinstance(slab, _PowerSlab) or slab.graph is not g:
            slab = _PowerSlab(g, p, chebyshev=cheb)
            self._active_dict[key] = slab
        return slab

    def _expansion(self, slab, n):
        """Coefficients of the terms ConvergenceManager (convergence.py:77-101) lets through, decided on the exact change of
        every step, |c_k| * ||term_k|| (the reference compares result_k with result_{k-1} = result_k - c_k term_k).  Returns
        (coeffs, iteration at exit, converged, last change) or None when the slab cannot hold that many powers;
        ``convergence.iteration`` is left as it was."""
        cm = self.convergence
        kind, tol = cm.device_error_kind(), cm.effective_tolerance()
        saved = cm.iteration
        coeffs, prev, it, converged, delta = [], None, 0, False, None
        try:
            while True:
                it += 1
                if it >= cm.max_iters:
                    break
                if delta is not None and kind != L.ERR_ITERS and it % cm.end_modulo == 0 and delta <= tol:
                    converged = True
                    break
                cm.iteration = it                           # _coefficient reads convergence.iteration
                prev = self._coefficient(prev)
                if not slab.ensure(it):
                    return None
                c = float(prev)
                coeffs.append(c)
                norm = slab.linf[it - 1] if kind == L.ERR_LINF else slab.l1[it - 1]
                delta = abs(c) * norm / (n if kind == L.ERR_MABS else 1)
        finally:
            cm.iteration = saved
        return coeffs, it, converged, delta

    def _fused_from_powers(self, M, personalization, ranks, out_scale):
        """optimization_dict route: the filter as ONE pass over the stored powers of this personalization."""
        slab = self._slab_for(M, personalization)
        if slab is None:
            return False
        n = max(len(personalization.np), 1)
        plan = self._expansion(slab, n)
        if plan is None:
            return False                                    # more terms than slabs may hold: the step-by-step route
        coeffs, it, converged, delta = plan
        ranks.np = slab.combine(np.asarray(coeffs, dtype=np.float64) * float(out_scale)) if coeffs \
            else backend.repeat(0.0, len(personalization.np))
        self.last_loop = dict(iterations=it, converged=converged, spmv=0, last_error=delta, loop_ms=0.0, terms=len(coeffs))
        self.convergence.finish_device_loop(it, converged)
        return True

    def rank_many(self, graph, personalization, variants):
        """The ranks of SEVERAL filters of this class on ONE personalization as the columns of an [n, P] device slab
        (P <= 64) -- the probes of an optimiser (autotune/parameterized.py:94-145: every probe differs in the coefficients
        only) or the candidate parameters of a sweep, evaluated in one pass over the stored powers (pgh_mat_gemm).
        `variants`: filters like this one (same graph pipeline, same convergence settings are NOT required: every variant
        stops by its own rule).  Needs an optimisation dict on self (its powers -- or, for the "chebyshev" form, the terms of
        the f64 recurrence -- are shared); returns (DeviceMatrix, [iterations of every variant])."""
        plan = self.probe_coefficients(graph, personalization, variants)
        if plan is None:
            from pygrank_amd.device import DeviceMatrix
            zeros = backend.repeat(0.0, len(to_signal(graph, personalization).np))
            return DeviceMatrix.from_columns([zeros] * len(variants)), [0] * len(variants)
        slab, C_, iterations = plan
        return slab.combine_many(C_), iterations

    def probe_coefficients(self, graph, personalization, variants):
        """What rank_many multiplies: (the power slab of this personalization, the [terms, P] coefficient matrix of the variants --
        every variant cut where its own stopping rule ends it, preserve_norm folded in --, [iterations of every variant]), or None
        for an all-zero personalization (every rank is zero).  A caller that only needs a statistic of the P columns (the tuner's
        AUC, include/pgh_tune.h) takes it from here without the [n, P] product."""
        if self.optimization_dict is None:
            raise Exception("rank_many evaluates stored powers: construct the filter with optimization_dict={}")
        if len(variants) < 1 or len(variants) > 64:
            raise Exception("rank_many takes 1 to 64 variants")
        if self.krylov_dims is not None or any(getattr(v, "krylov_dims", None) is not None for v in variants):
            raise Exception("rank_many evaluates stored powers of the personalization: filters with krylov_dims have none "
                            "(rank them one by one)")
        personalization = to_signal(graph, personalization)
        self._prepare(personalization)
        personalization = self.personalization_transform(personalization)
        raw = personalization.np
        norm = raw.abssum() if isinstance(raw, DeviceVector) else backend.sum(backend.abs(raw))
        if norm == 0:
            return None
        personalization = to_signal(personalization, personalization.np / norm)
        M = self.preprocessor(self._prepare_graph(personalization.graph, personalization))
        slab = self._slab_for(M, personalization)
        if slab is None:
            raise Exception("rank_many needs the engine's graph and a plain ConvergenceManager")
        n = max(len(personalization.np), 1)
        columns, iterations = [], []
        for v in variants:
            if not isinstance(v, ClosedFormGraphFilter) or v.coefficient_type != self.coefficient_type:
                raise Exception("rank_many variants must be closed-form filters of the same coefficient type")
            v.convergence.start()
            plan = v._expansion(slab, n)
            if plan is None:
                raise Exception("a variant needs more powers than the slabs may hold")
            coeffs, it, converged, _ = plan
            v.convergence.finish_device_loop(it, converged)
            scale = norm if v.preserve_norm else 1.0
            columns.append(np.asarray(coeffs, dtype=np.float64) * scale)
            iterations.append(it)
        terms = max((len(c) for c in columns), default=0)
        C_ = np.zeros((max(terms, 1), len(columns)))
        for q, c in enumerate(columns):
            C_[:len(c), q] = c
        return slab, C_, iterations

    def _fused_loop(self, M, personalization, ranks, out_scale, *args, **kwargs):
        if self.krylov_dims is not None:
            return self._krylov_loop(M, personalization, ranks, out_scale, args, kwargs)
        if args or kwargs or type(self)._step is not ClosedFormGraphFilter._step \
                or type(self)._recursion is not ClosedFormGraphFilter._recursion:
            return False
        if self.optimization_dict is not None:
            return type(self)._retrieve_power is ClosedFormGraphFilter._retrieve_power \
                and self._fused_from_powers(M, personalization, ranks, out_scale)
        if self.coefficient_type not in ("taylor", "chebyshev"):
            raise Exception("Invalid coefficient type")
        cfg = self._loop_cfg(0.0, False, out_scale)
        g = _device_graph(M)
        p, x = personalization.np, ranks.np
        if cfg is None or g is None or g.shape[0] != g.shape[1] or not isinstance(p, DeviceVector) \
                or not isinstance(x, DeviceVector):
            return False
        coeffs = np.asarray(self._coefficient_schedule(max(int(self.convergence.max_iters) - 1, 0)), dtype=np.float64)
        if isinstance(x, LazyVector):
            x = x._writable()              # written in place by the engine
        x._before_write()
        res = L.LoopResult()
        form = 1 if self.coefficient_type == "chebyshev" else 0
        if self._f64_wanted() and _f64_image_usable(g):
            form, cfg = (form or 2), self._f64_cfg(cfg)      # 2: the taylor form with f64 terms and accumulator
        L.check(L.lib().pgh_poly_run(g._h, p._h, coeffs.ctypes.data_as(C.c_void_p), len(coeffs), form, x._h, C.byref(cfg),
                                     C.byref(res)))
        ranks.np = x
        self.last_loop = dict(iterations=res.iterations, converged=bool(res.converged), spmv=res.spmv_count,
                              last_error=res.last_error, loop_ms=res.loop_ms)
        self.convergence.finish_device_loop(res.iterations, res.converged)
        return True

    def _krylov_forget(self):
        per_run = self._KRYLOV_PER_RUN + ("coefficient", "prev_term")
        for name in per_run:
            if hasattr(self, name):
                delattr(self, name)
        self._active_dict = None

    def _krylov_loop(self, M, personalization, ranks, out_scale, args, kwargs):
        """The loop of a run with krylov_dims under a plain ConvergenceManager with Mabs / L1 / MaxDifference;
        False where the hooks must run it one iteration at a time with has_converged.
        The k x k recursion runs on the host with the filter's own _coefficient and _recursion.  The change of iteration t is V d_t with
        d_t = (result_t - result_{t-1})[:, 0], so its residual sum_i |V d_t| or max_i |V d_t| is taken from d_t directly and not from
        two rounded f32 iterates: it resolves tolerances below fp32 eps, and the tolerance is clamped at fp64 eps as on the f64 routes
        (_f64_cfg), not at fp32 eps.  fused: the recursion runs AHEAD, up to 64 iterations at a time, and ONE pgh_krylov_residuals pass
        over the basis gives all their residuals; otherwise (fused=False, a library without the entry, a declined pass) every iteration
        costs one pgh_mat_gemv and two reductions.  ConvergenceManager's rule (convergence.py:77-101: the call before step t + 1
        compares the outcome of step t with the one before it, on multiples of end_modulo, and gives up at max_iters) then picks the
        stopping iteration exactly as _expansion does, a second chunk follows if the first does not stop, and the ranks are ONE
        pgh_mat_gemv.  As in the reference the first comparison is against the ranks' start value, the L1-normalised personalization
        -- in the Krylov space |p|_2 e_0."""
        own, cm, k = ClosedFormGraphFilter, self.convergence, int(self.krylov_dims)
        hooks = ("_start", "_step", "_end", "_recursion", "_retrieve_power")
        if args or kwargs or any(getattr(type(self), hook) is not getattr(own, hook) for hook in hooks) \
                or type(cm) is not ConvergenceManager or cm.device_error_kind() not in (L.ERR_MABS, L.ERR_L1, L.ERR_LINF) \
                or self.coefficient_type not in self._FORMS \
                or getattr(self, "_raw_input", None) is None:          # (a warm start: the first comparison is against another vector)
            return False
        kind, n = cm.device_error_kind(), max(len(personalization.np), 1)
        tol = 0.0 if cm.tol is None else max(float(cm.tol), float(np.finfo(np.float64).eps))
        try:
            self._start(M, personalization, ranks)
            basis = self.krylov_base
            ahead = L.KRYLOV_MAX_PROBES if basis.residual_entry(self.fused) is not None else 1
            before = np.zeros(k)
            before[0] = basis.p_norm
            done, passes, err, converged, it, stop_at = 0, 0, float("nan"), False, 1, None
            while stop_at is None:
                steps = range(done + 1, min(done + ahead, int(cm.max_iters) - 1) + 1)
                cols = []
                for s in steps:
                    cm.iteration = s                        # _coefficient and _recursion read convergence.iteration
                    weight = self.coefficient = self._coefficient(self.coefficient)
                    self.krylov_result, term = self._recursion(self.krylov_result, self.Mpower, weight)
                    self.Mpower = self._retrieve_power(term, self.krylov_H)
                    cols.append(np.array(np.asarray(self.krylov_result)[:, 0], dtype=np.float64))
                if not cols:                                # max_iters <= 1: the first has_converged call ends the run
                    it = done + 1
                    break
                deltas = np.stack([now - was for now, was in zip(cols, [before] + cols[:-1])], axis=1)
                sums, tops, fused_pass = basis.residuals(deltas, self.fused)
                passes += fused_pass
                errors = tops if kind == L.ERR_LINF else (sums / n if kind == L.ERR_MABS else sums)
                for index, s in enumerate(steps):
                    it, err = s + 1, float(errors[index])   # the has_converged call that follows step s
                    if it >= cm.max_iters or (it % cm.end_modulo == 0 and err <= tol):
                        converged, stop_at = it < cm.max_iters, cols[index]
                        break
                done, before = steps[-1], cols[-1]
            if stop_at is not None:
                ranks.np = basis.project(stop_at, out_scale)
            elif out_scale != 1.0:
                ranks.np = ranks.np * out_scale
            self.last_loop = dict(iterations=it, converged=converged, spmv=self._krylov_spmv, last_error=err, dims=k,
                                  residual_passes=passes)
        finally:
            self._krylov_forget()
        cm.finish_device_loop(it, converged)
        return True

    def propagate(self, graph, features, *args, **kwargs):
        """signals.py:225-226 (one rank() per feature column) as multi-seed batches of up to 64 columns through pgh_poly_run_batch
        (include/pgh_batch.h) wherever a single rank() would run the f32 taylor loop of pgh_poly_run: the adjacency is streamed once
        per term for the whole batch and every column stops at its own iteration.  The column loop otherwise (the "chebyshev" form,
        an optimisation dict, overridden hooks, f64 iterates ...).  With f64_batch=True a taylor run that wants f64 iterates goes
        through pgh_poly_run_batch_f64 (include/pgh_batch64.h) the same way, its personalizations L1-normalised in f32 as a single
        rank() normalises them."""
        own = ClosedFormGraphFilter
        g = g64 = None
        if self.coefficient_type == "taylor" and self.optimization_dict is None and self.krylov_dims is None and type(self)._step is own._step \
                and type(self)._recursion is own._recursion and type(self)._start is own._start \
                and type(self)._retrieve_power is own._retrieve_power and type(self)._prepare is own._prepare:
            g64 = self._batch_graph(graph, args, kwargs, f64=True)
            g = self._batch_graph(graph, args, kwargs) if g64 is None else None
        entry64 = L.entry("pgh_poly_run_batch_f64") if g64 is not None else None
        if entry64 is not None:
            coeffs = np.asarray(self._coefficient_schedule(max(int(self.convergence.max_iters) - 1, 0)), dtype=np.float64)
            out = _propagate_in_batches64(self, features, self._loop_cfg(0.0, False, 1.0), lambda P, R, cfg_ref, scales, res, norms: entry64(
                g64._h, P._h, coeffs.ctypes.data_as(C.c_void_p), len(coeffs), R._h, cfg_ref, scales, res), raw=False)
            if out is not None:
                return out
        entry = L.entry("pgh_poly_run_batch") if g is not None else None
        if entry is not None:
            cfg = self._loop_cfg(0.0, False, 1.0)
            coeffs = np.asarray(self._coefficient_schedule(max(int(self.convergence.max_iters) - 1, 0)), dtype=np.float64)
            out = _propagate_in_batches(self, features, cfg, lambda P, R, cfg_ref, scales, res: (entry(
                g._h, P._h, coeffs.ctypes.data_as(C.c_void_p), len(coeffs), R._h, cfg_ref, scales, res), None))
            if out is not None:
                return out
        return super().propagate(graph, features, *args, **kwargs)


class GenericGraphFilter(ClosedFormGraphFilter):
    """low_pass.py:5-26: filter defined by its hop weights."""

    def __init__(self, weights=None, **kwargs):
        super().__init__(**kwargs)
        self.weights = weights if weights is not None else [0.9] * 10

    def _coefficient(self, _):
        if self.convergence.iteration > len(self.weights):
            return 0
        return self.weights[self.convergence.iteration - 1]

    def _reference(self):
        return f"graph filter with {len(self.weights)} hop weights"


class HeatKernel(ClosedFormGraphFilter):
    """adhoc.py:93-122."""

    def __init__(self, t=3, *args, **kwargs):
        self.t = t
        super().__init__(*args, **kwargs)

    def _coefficient(self, previous_coefficient):                                 # adhoc.py:113-116
        return 1. if previous_coefficient is None else (previous_coefficient * self.t / (self.convergence.iteration + 1))

    def _reference(self):
        return f"heat kernel (t = {self.t:g})"


class PageRankClosed(ClosedFormGraphFilter):
    """adhoc.py:63-90."""

    def __init__(self, alpha=0.85, *args, **kwargs):
        self.alpha = alpha
        super().__init__(*args, **kwargs)

    def _coefficient(self, previous_coefficient):                                 # adhoc.py:83-84
        return 1. if previous_coefficient is None else (previous_coefficient * self.alpha)

    def _reference(self):
        return f"PageRank as a power series (alpha = {self.alpha:g})"


