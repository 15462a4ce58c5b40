"""Postprocessors that act on rank vectors already resident in HBM.

``Tautology`` is the default ``personalization_transform`` of every filter (abstract_filters.py:37) and ``Normalize`` is
the callable form of ``use_quotient`` (abstract_filters.py:131-132; the reference's filter tests compare outcomes after
``Normalize``, tests/test_filters.py:41-82).  ``Ordinals`` / ``Top`` / ``Threshold`` / ``Transformer`` / ``Sweep`` /
``LinearSweep`` are SURVEY.md 8f-3: elementwise kernels, device reductions and one device radix sort instead of the
reference's per-node Python dictionaries.  Behaviour follows pygrank/algorithms/postprocess/postprocess.py:7-80,106-290,
353-450.  ``propagate`` keeps the inner ranker's batch: the inner ``propagate`` runs once and its [n, b] slab goes through the
passes of include/pgh_post.h (a multi-column radix select for ``Top``, one slab pass each for the others), so a
chain such as ``PageRank() >> Sweep() >> Normalize() >> Top(10)`` stays on the device between the multi-seed loop and the measures'
``evaluate_many``.  ``MabsMaintain`` / ``Sequential`` / ``SeparateNormalization`` follow postprocess.py:83-103,461-503; the first and the
last have slab forms on the passes of include/pgh_select.h.  The fairness postprocessors are in
pygrank_amd/fairness.py, the seed oversampling ones in pygrank_amd/oversampling.py, ``Subgraph`` / ``Supergraph`` in pygrank_amd/subgraph.py."""
from pygrank_amd import _lib as L
from pygrank_amd import backend
from pygrank_amd.device import DeviceMatrix, DeviceVector
from pygrank_amd.signals import GraphSignal, NodeRanking, to_signal
from pygrank_amd.utils import call, ensure_used_args, remove_used_args


CHUNK = L.POST_MAX_COLS        # most columns of one include/pgh_post.h call


def _definer(cls, name):
    for base in cls.__mro__:
        if name in vars(base):
            return base
    return None


def _as_slab(features):
    F = features if isinstance(features, DeviceMatrix) else backend.to_primitive(features)
    return F if isinstance(F, DeviceMatrix) else DeviceMatrix.from_columns([F])


class _Calls(dict):
    """The engine calls of one ``propagate``, by entry name."""

    def add(self, name, times=1):
        self[name] = self.get(name, 0) + times


class Postprocessor(NodeRanking):
    """A ranker wrapped around another ranker: ``rank`` runs the inner one and passes its outcome through ``_transform``.

    ``propagate`` of a class with a slab form (``_slab``: Normalize, Ordinals, Transformer, Top, Threshold, Sweep, LinearSweep) runs the
    inner ranker's ``propagate`` ONCE and transforms its outcome.  Two switches, class attributes an instance may set to False:
    ``batch = False`` is one ``rank()`` per column (NodeRanking.propagate); ``fused = False`` keeps the inner batch but sends its columns
    through ``_apply`` one by one, on backend primitives.  After a call ``last_propagate`` holds the route ("slab": the entries of
    include/pgh_post.h, "columns": the inner batch's columns one by one -- also what a library without the entries or a declined call
    takes --, "ranks": one ``rank()`` per column), the widths of the chunks (at most 64 columns) and the engine calls made for the
    transformation.  A subclass without a slab form, or one that overrides what the slab form stands for, takes "ranks"."""

    batch = True
    fused = True
    _slab = None        # (self, graph, chunk, calls) -> the transformed [n, b <= 64] slab, or None when the engine does not serve it
    _needs = tuple(L.POST_SIGNATURES)      # the optional entries the slab form calls

    def __init__(self, ranker=None):
        self.ranker = ranker

    def _has_slab_form(self):
        cls = type(self)
        owner = _definer(cls, "_slab")
        if owner is None or vars(owner)["_slab"] is None or self.ranker is None:
            return False
        # the slab form restates _values / _transform / _apply of its own class: a subclass that changes one of them is not restated
        return all(issubclass(owner, _definer(cls, name)) for name in ("_values", "_transform", "_apply", "transform", "rank")
                   if _definer(cls, name) is not None)

    def propagate(self, graph, features, *args, **kwargs):
        calls = _Calls()
        self.last_propagate = dict(route="ranks", chunks=[], calls=calls)
        if not self.batch or not self._has_slab_form():
            return super().propagate(graph, features, *args, **kwargs)
        inner = self.ranker.propagate(graph, features, *args, **kwargs)
        leftover = remove_used_args(self.ranker.rank, kwargs)      # keywords the inner ranker did not take, as in rank
        plain = graph.graph if isinstance(graph, GraphSignal) else graph
        # (a keyword that _transform has a parameter for would reach it through _apply: the columns route lets it)
        reaching = len(leftover) - len(remove_used_args(self._transform, leftover))
        served = all(L.entry(name) is not None for name in self._needs)          # (a library has all of a header or none)
        if self.fused and served and isinstance(inner, DeviceMatrix) and inner.n > 0 and not reaching:
            widths = [min(CHUNK, inner.b - first) for first in range(0, inner.b, CHUNK)]
            out = DeviceMatrix.empty(inner.n, inner.b) if inner.b > CHUNK else None
            for first, chunk in inner.chunks(CHUNK):
                done = self._slab(plain, chunk, calls)
                if done is None:
                    break
                if out is None:
                    out = done
                else:
                    out.set_cols(first, done)
            else:
                self.last_propagate.update(route="slab", chunks=widths)
                return out
            calls.clear()
        self.last_propagate.update(route="columns", chunks=[inner.b] if isinstance(inner, DeviceMatrix) else [])
        columns = [self._apply(to_signal(graph, column), leftover)._np for column in backend.separate_cols(inner)]
        return backend.combine_cols(columns)

    def _transform(self, ranks, **kwargs):
        raise Exception("_transform method not implemented for the class " + type(self).__name__)

    def _apply(self, ranks, kwargs):
        return to_signal(ranks, call(self._transform, kwargs, [ranks]))

    def transform(self, ranks, *args, **kwargs):
        return self._apply(ranks, kwargs)

    def rank(self, *args, **kwargs):
        inner = self.ranker.rank(*args, **kwargs)
        return self._apply(inner, remove_used_args(self.ranker.rank, kwargs))      # keywords the inner ranker did not take

    def __lshift__(self, ranker):
        if isinstance(ranker, NodeRanking):
            self.ranker = ranker
            return ranker
        raise Exception("only a ranker can be shifted into a postprocessor, got " + type(ranker).__name__)

    # self-description: the wrapped algorithm's parts, then this step (postprocess.py: references() of every postprocessor
    # extends the inner ranker's list)
    def _reference(self):
        return type(self).__name__.lower() + " postprocessing"

    def references(self):
        inner = list(self.ranker.references()) if self.ranker is not None else []
        return inner + [self._reference()]

    # a wrapped filter's collaborators show through, so that ``postprocessor.convergence`` works like the filter's
    preprocessor = property(lambda self: self.ranker.preprocessor)
    convergence = property(lambda self: self.ranker.convergence,
                           lambda self, value: setattr(self.ranker, "convergence", value))


class Tautology(Postprocessor):
    """Changes nothing; without an inner ranker ``rank`` turns its input into a signal."""

    def references(self):
        return list(self.ranker.references()) if self.ranker is not None else ["tautology"]

    def transform(self, ranks, *args, **kwargs):
        return ranks

    def rank(self, graph=None, personalization=None, *args, **kwargs):
        inner = self.ranker
        return to_signal(graph, personalization) if inner is None else inner.rank(graph, personalization, *args, **kwargs)

    def propagate(self, graph, features, *args, **kwargs):
        """The inner ranker's ``propagate``; without one the features themselves, as a slab."""
        self.last_propagate = dict(route="ranks", chunks=[], calls=_Calls())
        if not self.batch or type(self).rank is not Tautology.rank:
            return super().propagate(graph, features, *args, **kwargs)
        out = _as_slab(features) if self.ranker is None else self.ranker.propagate(graph, features, *args, **kwargs)
        if isinstance(out, DeviceMatrix):
            self.last_propagate.update(route="slab", chunks=[min(CHUNK, out.b - first) for first in range(0, out.b, CHUNK)])
        return out


def _is_ranker(obj):
    return callable(getattr(obj, "rank", None))


class _NoOptions(Postprocessor):
    """Postprocessors whose transformation takes no keyword of its own: whatever is still there when the call arrives was
    meant for nobody (the reference's ``ensure_used_args`` at the top of every ``_transform``); the work is in ``_values``."""

    def _transform(self, ranks, **leftover):
        ensure_used_args(leftover)
        return self._values(ranks)


class Normalize(_NoOptions):
    """Rescales ranks by their maximum ("max", default), sum ("sum"), Euclidean norm ("L2"), or onto [0, 1] ("range").
    ``Normalize("sum", ranker)`` and ``Normalize(ranker, "sum")`` are the same thing (postprocess.py:124-131)."""

    _METHODS = ("max", "sum", "L2", "range")

    def __init__(self, ranker=None, method="max"):
        if ranker is not None and not _is_ranker(ranker):          # the method came first
            ranker, method = (method if _is_ranker(method) else None), ranker
        super().__init__(ranker if ranker is not None else Tautology())
        self.method = method

    def _values(self, ranks):
        how = self.method
        if how not in self._METHODS:
            raise Exception("Normalize: method must be one of " + ", ".join(self._METHODS) + ", not " + repr(how))
        x = ranks.np
        low = float(backend.min(x)) if how == "range" else 0.0
        high = float({"sum": backend.sum, "L2": lambda v: float(backend.dot(v, v)) ** 0.5}.get(how, backend.max)(x))
        if high == low:
            return ranks                                           # constant (or zero) signals stay as they are
        return (x - low) / (high - low)

    def _slab(self, graph, chunk, calls):
        """Every method from one pgh_mat_col_stats (sum, sum of squares, max, min per column), then (x - low) / (high - low) as
        pgh_post_col_affine; a column with high == low is copied."""
        how = self.method
        if how not in self._METHODS:
            raise Exception("Normalize: method must be one of " + ", ".join(self._METHODS) + ", not " + repr(how))
        stats = chunk.col_stats()
        if stats is None:
            return None
        calls.add("pgh_mat_col_stats")
        low = [float(s[3]) if how == "range" else 0.0 for s in stats]
        high = [float({"sum": s[0], "L2": float(s[1]) ** 0.5}.get(how, s[2])) for s in stats]
        out = chunk.col_affine(low, [0.0 if h == l else h - l for h, l in zip(high, low)])      # 0: constant (or zero) columns stay
        if out is not None:
            calls.add("pgh_post_col_affine")
        return out


def _device(ranks):
    x = ranks.np
    return x if isinstance(x, DeviceVector) else backend.to_array(x)


def _swap(first, second):
    """The reference's constructors accept (ranker, value) in either order (postprocess.py:124-131,246-252)."""
    if first is not None and not _is_ranker(first):
        first, second = (second if _is_ranker(second) else None), first
    return (first if first is not None else Tautology()), second


class Ordinals(_NoOptions):
    """1 for the highest rank, 2 for the second highest, ... (postprocess.py:163-195); ties keep node order."""

    def __init__(self, ranker=None):
        super().__init__(_swap(ranker, None)[0])

    def _values(self, ranks):
        return _device(ranks).ordinals()

    def _slab(self, graph, chunk, calls):
        out = chunk.ordinals()
        if out is not None:
            calls.add("pgh_post_ordinals")
        return out


class Transformer(_NoOptions):
    """Element-by-element expression, backend.exp by default (postprocess.py:198-243)."""

    def __init__(self, ranker=None, expr=None):
        ranker, expr = _swap(ranker, expr)
        super().__init__(ranker)
        self.expr = backend.exp if expr is None else expr
        self._default_expr = self.expr if expr is None else None

    def _values(self, ranks):
        return self.expr(ranks.np)

    def _slab(self, graph, chunk, calls):
        """The default expression is one pgh_ewise_unary over the slab's storage, n * b entries; any other goes column by column."""
        if self._default_expr is None or self.expr is not self._default_expr:
            return None
        out = DeviceMatrix.empty(chunk.n, chunk.b)
        source, target = chunk.flat(), out.flat()                     # (the views live until the call has been made)
        L.check(L.lib().pgh_ewise_unary(L.EXP, source._h, target._h))
        calls.add("pgh_ewise_unary")
        return out


class Top(_NoOptions):
    """1 for the top-scored nodes, 0 for the rest; ``fraction_of_training`` >= 1 counts nodes, < 1 is a share of the graph
    (postprocess.py:246-290: every node that ties with the last kept one is kept too)."""

    def __init__(self, ranker=None, fraction_of_training=1):
        ranker, fraction = _swap(ranker, fraction_of_training)
        super().__init__(ranker)
        self.fraction_of_training = 1 if fraction is None else fraction

    def _values(self, ranks):
        x = _device(ranks)
        keep = self.fraction_of_training
        keep = int(keep * len(x)) if keep < 1 else int(keep)
        threshold = x.kth_largest(keep) if 1 <= keep <= len(x) else 0     # the reference's loop leaves 0 otherwise
        return (x >= threshold) * 1.0

    def _slab(self, graph, chunk, calls):
        """Every column's cut from one radix select (pgh_post_kth_largest), then one compare pass (pgh_post_col_threshold)."""
        keep = self.fraction_of_training
        keep = int(keep * chunk.n) if keep < 1 else int(keep)
        cuts = [0.0] * chunk.b                                         # the reference's loop leaves 0 for a keep outside [1, n]
        if 1 <= keep <= chunk.n:
            cuts = chunk.kth_largest(keep)
            if cuts is None:
                return None
            calls.add("pgh_post_kth_largest")
        out = chunk.col_threshold(cuts, inclusive=True)
        if out is not None:
            calls.add("pgh_post_col_threshold")
        return out


class Threshold(_NoOptions):
    """1 above a threshold, 0 elsewhere (postprocess.py:293-350); "gap" = the score after the largest relative drop."""

    def __init__(self, ranker=None, threshold=0, inclusive=False):
        ranker, threshold = _swap(ranker, threshold)
        super().__init__(ranker)
        self.threshold = 0 if threshold is None else threshold
        self.inclusive = inclusive

    def _values(self, ranks):
        x = _device(ranks)
        # "gap": one device sort + two reductions (pgh_vec_gap_threshold)
        cut = x.gap_threshold() if self.threshold == "gap" else self.threshold
        return ((x >= cut) if self.inclusive else (x > cut)) * 1.0

    def _slab(self, graph, chunk, calls):
        """A fixed cut goes straight to pgh_post_col_threshold; "gap" takes every column's cut from pgh_vec_gap_threshold first."""
        if self.threshold == "gap":
            cuts = [column.gap_threshold() for column in chunk.columns()]
            calls.add("pgh_mat_get_col", chunk.b)
            calls.add("pgh_vec_gap_threshold", chunk.b)
        else:
            cuts = [float(self.threshold)] * chunk.b
        out = chunk.col_threshold(cuts, inclusive=bool(self.inclusive))
        if out is not None:
            calls.add("pgh_post_col_threshold")
        return out


class _UniformBaseline(_NoOptions):
    """Sweep family: personalized ranks set against the same ranker's non-personalized outcome, computed once per graph."""

    def __init__(self, ranker=None, uniform_ranker=None):
        super().__init__(ranker)
        self.uniform_ranker = uniform_ranker if uniform_ranker is not None else ranker
        self._baseline = {}

    def _uniforms(self, ranks):
        return self._uniforms_on(ranks.graph)

    def _uniforms_on(self, graph):
        key = id(graph)
        if key not in self._baseline:
            self._baseline[key] = (graph, _device(self.uniform_ranker.rank(graph)))   # keeps the graph alive: ids are not reused
        return self._baseline[key][1]

    def _row_slab(self, graph, chunk, calls, op, offset=0.0):
        """One baseline vector per graph, then one pgh_post_row_op over the slab."""
        out = chunk.row_op(self._uniforms_on(graph), op, offset)
        if out is not None:
            calls.add("pgh_post_row_op")
        return out

    def __lshift__(self, ranker):
        self.uniform_ranker = super().__lshift__(ranker)
        return self.uniform_ranker


class Sweep(_UniformBaseline):
    """ranks / (1e-12 + uniform ranks) (postprocess.py:353-404)."""

    def _values(self, ranks):
        return _device(ranks) / (self._uniforms(ranks) + 1.E-12)

    def _slab(self, graph, chunk, calls):
        return self._row_slab(graph, chunk, calls, L.POST_ROW_SWEEP, 1.E-12)


class LinearSweep(_UniformBaseline):
    """ranks - uniform ranks (postprocess.py:407-450)."""

    def _values(self, ranks):
        return _device(ranks) - self._uniforms(ranks)

    def _slab(self, graph, chunk, calls):
        return self._row_slab(graph, chunk, calls, L.POST_ROW_SUB)


class MabsMaintain(Postprocessor):
    """Rescales the ranks so that the sum of their absolute values is that of the personalization (postprocess.py:83-103); a zero
    personalization leaves them as they are.

    ``propagate`` runs the inner ``propagate`` once, takes every column's sum |features| and sum |ranks| (pgh_mat_col_abssum) and rescales
    the slab in one pass (pgh_mat_col_scale, include/pgh_select.h): route "slab".  ``fused = False``, a library without the entry or a
    column whose ranks sum to zero rescales the inner batch's columns one by one ("columns"); ``batch = False`` is one ``rank()`` per
    column ("ranks")."""

    _needs = ("pgh_mat_col_scale",)

    def __init__(self, ranker=None):
        super().__init__(Tautology() if ranker is None else ranker)

    def rank(self, graph=None, personalization=None, *args, **kwargs):
        personalization = to_signal(graph, personalization)
        norm = backend.sum(backend.abs(personalization.np))
        ranks = self.ranker(graph, personalization, *args, **kwargs)
        if norm != 0:
            ranks.np = ranks.np * norm / backend.sum(backend.abs(ranks.np))
        return ranks

    def _slab(self, norms, chunk, calls):
        """chunk * (norm / sum |chunk|) per column: the one f32 product ``ranks * norm / total`` stores."""
        totals = chunk.col_abssum()
        calls.add("pgh_mat_col_abssum")
        if any(total == 0 and norm != 0 for norm, total in zip(norms, totals)):
            return None
        out = chunk.col_scale([norm * (1.0 / total) if norm != 0 else 1.0 for norm, total in zip(norms, totals)])
        if out is not None:
            calls.add("pgh_mat_col_scale")
        return out

    def propagate(self, graph, features, *args, **kwargs):
        calls = _Calls()
        self.last_propagate = dict(route="ranks", chunks=[], calls=calls)
        if not self.batch or not self._has_slab_form():
            return NodeRanking.propagate(self, graph, features, *args, **kwargs)
        F = _as_slab(features)
        inner = self.ranker.propagate(graph, F, *args, **kwargs)
        norms = F.col_abssum()
        served = all(L.entry(name) is not None for name in self._needs)
        if self.fused and served and isinstance(inner, DeviceMatrix) and inner.n > 0:
            calls.add("pgh_mat_col_abssum")
            widths = [min(CHUNK, inner.b - first) for first in range(0, inner.b, CHUNK)]
            out = DeviceMatrix.empty(inner.n, inner.b) if inner.b > CHUNK else None
            for first, chunk in inner.chunks(CHUNK):
                done = self._slab(norms[first:first + chunk.b], chunk, calls)
                if done is None:
                    break
                if out is None:
                    out = done
                else:
                    out.set_cols(first, done)
            else:
                self.last_propagate.update(route="slab", chunks=widths)
                return out
            calls.clear()
        self.last_propagate.update(route="columns", chunks=[inner.b] if isinstance(inner, DeviceMatrix) else [])
        columns = [column * norm / backend.sum(backend.abs(column)) if norm != 0 else column
                   for norm, column in zip(norms, backend.separate_cols(inner))]
        return backend.combine_cols(columns)

    def _reference(self):
        return "mabs preservation"


class Sequential(Postprocessor):
    """Passes the outcome of its first ranker through the others, each called on the signal as it stands (postprocess.py:461-472).  There
    is no slab form: ``propagate`` is one ``rank()`` per column."""

    def __init__(self, *rankers):
        super().__init__(rankers[0] if rankers else None)
        self.rankers = list(rankers)

    def _transform(self, ranks, **kwargs):
        for ranker in self.rankers:
            if ranker is not self.ranker:
                ranks = ranker(ranks)
        return ranks


class SeparateNormalization(Postprocessor):
    """Normalises two groups of nodes apart: with a separator s in [0, 1] the ranks become r s / sum(r s) + r (1 - s) / sum(r (1 - s))
    (postprocess.py:475-503; a zero sum leaves its part zero).  ``SeparateNormalization(ranker, separator)`` is accepted too.

    The slab form takes every column's two sums from pgh_mat_split_sums and blends in one pass (pgh_mat_split_blend,
    include/pgh_select.h)."""

    _needs = ("pgh_mat_split_sums", "pgh_mat_split_blend")

    def __init__(self, separator=None, ranker=None):
        if isinstance(separator, NodeRanking):
            separator, ranker = ranker, separator
        super().__init__(Tautology() if ranker is None else ranker)
        self.separator = separator

    def _transform(self, ranks, **kwargs):
        separator = to_signal(ranks, self.separator)
        first = ranks * separator
        second = ranks * (1 - separator)
        return first * backend.safe_div(1., backend.sum(first.np)) + second * backend.safe_div(1., backend.sum(second.np))

    def _slab(self, graph, chunk, calls):
        separator = _device(to_signal(graph, self.separator))
        sums = chunk.split_sums(separator)
        if sums is None:
            return None
        calls.add("pgh_mat_split_sums")
        out = chunk.split_blend(separator, [backend.safe_div(1., float(s)) for s in sums[:, 0]],
                                [backend.safe_div(1., float(s)) for s in sums[:, 1]])
        if out is not None:
            calls.add("pgh_mat_split_blend")
        return out
