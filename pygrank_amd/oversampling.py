"""Seed oversampling postprocessors [krasanakis2019boosted]: SeedOversampling and BoostedSeedOversampling.

Restates pygrank/algorithms/postprocess/oversampling.py:9-61 (``SeedOversampling``) and :64-130 (``BoostedSeedOversampling``).

Both re-invoke the base ranker on seed sets grown from its own outcome.  The reference finds the threshold with
``min(ranks[u] for u in personalization if personalization[u] == 1)`` and builds every next seed set with a dictionary comprehension: on
device vectors that is one read per node.  Here the work between two runs of the ranker is four passes over [n, b] slabs
(include/pgh_oversample.h), and the rule runs on up to 64 seed sets at once: ``propagate(graph, features)`` ranks
every round of a chunk's columns with ONE ``ranker.propagate`` (the adjacency streamed once per iteration for all columns) while every
column keeps its own threshold, weight and weight-convergence manager; a column of the boosted loop whose weights have converged leaves
the batch.  ``rank`` is the same loop on one column, with ``ranker.rank`` inside.

Extensions of the constructors: ``fused=False`` (or a library without the entries -- the host test double -- or a declined call) runs the
same rule from backend primitives, column by column; ``batch=False`` makes ``propagate`` rank the columns one by one;
``min_batch_width`` (default ``MIN_BATCH_WIDTH`` = 8, the measured crossover) is the least number of live columns the inner ranker is
asked to ``propagate`` -- below it the slab passes still serve all live columns at once, the ranker takes them one ``rank`` each.
"""
import copy
import ctypes as C

import numpy as np

from pygrank_amd import _lib as L
from pygrank_amd import backend
from pygrank_amd.convergence import ConvergenceManager
from pygrank_amd.device import DeviceMatrix
from pygrank_amd.measures import MaxDifference
from pygrank_amd.postprocess import Postprocessor, _is_ranker
from pygrank_amd.preprocessing import graph_to_scipy, preprocessor as default_preprocessor
from pygrank_amd.signals import GraphSignal, to_signal

_ENTRIES = ("pgh_seed_floor", "pgh_seed_resample", "pgh_boost_forms", "pgh_boost_update")
CHUNK = L.OVERSAMPLE_MAX_COLS


def _doubles(values):
    return (C.c_double * len(values))(*[float(v) for v in values])


class _SlabPasses:
    """The four passes of include/pgh_oversample.h on DeviceMatrix slabs.  ``fused``: through the entries while the library has them and
    they accept the call; otherwise -- and after the first declined call -- the same rules from backend primitives, column by column.
    ``calls`` counts the passes by route."""

    def __init__(self, fused):
        self.entries = {name: L.entry(name) for name in _ENTRIES} if fused else {}
        if any(entry is None for entry in self.entries.values()):
            self.entries = {}
        self.calls = dict(fused=0, primitive=0)

    def _fused(self, name, *args):
        """True when the entry served the call; False (and no further fused call) when there is none or it declined."""
        entry = self.entries.get(name)
        if entry is not None:
            status = entry(*args)
            if L.accepted(status):
                self.calls["fused"] += 1
                return True
            self.entries = {}
        self.calls["primitive"] += 1
        return False

    # ---- floor[c] = min of ranks[:, c] over seeds[:, c] == 1, count[c] = how many such rows
    def floor(self, ranks, seeds):
        b = ranks.b
        floors, counts = (C.c_double * b)(), (C.c_int64 * b)()
        if self._fused("pgh_seed_floor", ranks._h, seeds._h, floors, counts):
            return list(floors), [int(c) for c in counts]
        return self._floor_of_columns(ranks.columns(), seeds.columns())

    @staticmethod
    def _floor_of_columns(ranks, seeds):
        floors, counts = [], []
        for r, s in zip(ranks, seeds):
            hit = s == 1.0
            count = int(round(hit.sum()))
            counts.append(count)
            floors.append(float("inf") if count == 0 else float(r[hit].min()))
        return floors, counts

    # ---- out = 1 where ranks >= floor (strict: >) or keep == 1, else 0; count[c] = ones written
    def resample(self, ranks, floors, strict=False, keep=None):
        b = ranks.b
        counts = (C.c_int64 * b)()
        out = DeviceMatrix.empty(ranks.n, b)
        if self._fused("pgh_seed_resample", ranks._h, _doubles(floors), 1 if strict else 0, None if keep is None else keep._h, out._h, counts):
            return out, [int(c) for c in counts]
        columns, totals = [], []
        kept = keep.columns() if keep is not None else [None] * b
        for r, cut, k in zip(ranks.columns(), floors, kept):
            cut = float(np.float32(cut))
            one = (r > cut) if strict else (r >= cut)
            if k is not None:
                one = (one + (k == 1.0)) > 0.0
            columns.append(one)
            totals.append(int(round(one.sum())))
        return DeviceMatrix.from_columns(columns), totals

    # ---- S1 = sum s R^2, S2 = sum R^2, S3 = sum s RN R per column
    def forms(self, seeds, fresh, total):
        b = seeds.b
        out = (C.c_double * (3 * b))()
        if self._fused("pgh_boost_forms", seeds._h, fresh._h, total._h, out):
            return [tuple(out[3 * c:3 * c + 3]) for c in range(b)]
        sums = []
        for s, R, RN in zip(seeds.columns(), fresh.columns(), total.columns()):
            sums.append((float((s * R).dot(R)), float(R.dot(R)), float((s * RN).dot(R))))   # s is 0 / 1: both products are exact
        return sums

    # ---- total += weights[c] * fresh in place; returns floor(total after, mask)
    def update(self, total, fresh, weights, mask):
        b = total.b
        floors, counts = (C.c_double * b)(), (C.c_int64 * b)()
        if self._fused("pgh_boost_update", total._h, fresh._h, _doubles(weights), mask._h, floors, counts):
            return list(floors), [int(c) for c in counts]
        columns = [RN.axpby(1.0, R, float(w)) for RN, R, w in zip(total.columns(), fresh.columns(), weights)]
        for c, column in enumerate(columns):
            total.set_column(c, column)
        return self._floor_of_columns(columns, mask.columns())


def _as_slab(features):
    F = features if isinstance(features, DeviceMatrix) else backend.to_primitive(features)
    return F if isinstance(F, DeviceMatrix) else DeviceMatrix.from_columns([F])


def _take(slab, columns):
    return DeviceMatrix.from_columns([slab.column(c) for c in columns])


class _Oversampler(Postprocessor):
    """What the two postprocessors share: ``rank`` and ``propagate`` over one loop on a slab of seed sets, and the inner ranker's call."""

    # Measured on an MI355X (tools/oversample_bench.py, profiles/oversampling/, PageRank(0.9, L1, 1e-6) inside, batch / one by one): at
    # RMAT scale 20 a boosted run of 2 columns takes 1.93 times and of 4 columns 1.22 times as long batched as one by one, of 8 columns
    # 0.76 and of 64 columns 0.32 times (all with disjoint spreads).  Widths 5 to 7 are not measured.  At scale 23, 8 columns take 1.10.
    MIN_BATCH_WIDTH = 8

    def __init__(self, ranker, fused, batch, min_batch_width):
        super().__init__(ranker)
        self.fused, self.batch, self.min_batch_width = bool(fused), bool(batch), min_batch_width
        self.last_passes = dict(fused=0, primitive=0)

    def _inner(self, graph, seeds, kwargs):
        """The base ranker on every column of `seeds`: ``propagate`` from ``min_batch_width`` columns on (a ranker without a batch of
        its own falls back to NodeRanking.propagate, one rank() per column), one ``rank`` per column below it -- always for one."""
        least = self.MIN_BATCH_WIDTH if self.min_batch_width is None else self.min_batch_width
        if seeds.b == 1 or seeds.b < least:
            columns = [self.ranker.rank(graph, to_signal(graph, column), **kwargs).np for column in seeds.columns()]
            return DeviceMatrix.from_columns([backend.to_array(column) for column in columns])
        return _as_slab(self.ranker.propagate(graph, seeds, **kwargs))

    def _loop(self, graph, seeds, passes, kwargs):
        """The ranks [n, b] of one chunk of seed sets; the per-column statistics (``last_*``) are extended."""
        raise NotImplementedError

    def _run(self, graph, F, width, kwargs):
        self._reset()
        passes = _SlabPasses(self.fused)
        out = DeviceMatrix.empty(F.n, F.b) if F.b > width else None
        for first, chunk in F.chunks(width):
            ranks = self._loop(graph, chunk, passes, kwargs)
            self.last_passes = dict(passes.calls)
            if out is None:
                return ranks
            out.set_cols(first, ranks)
        return out

    def rank(self, graph=None, personalization=None, **kwargs):
        personalization = to_signal(graph, personalization)
        slab = DeviceMatrix.from_columns([backend.to_array(personalization.np)])
        return to_signal(personalization, self._run(personalization.graph, slab, 1, kwargs).column(0))

    def propagate(self, graph, features, **kwargs):
        """``rank`` of every column of `features` ([n, B] zeros and ones), up to 64 columns per chunk as one batch; a DeviceMatrix."""
        if isinstance(graph, GraphSignal):
            graph = graph.graph
        return self._run(graph, _as_slab(features), CHUNK if self.batch else 1, kwargs)


def _number_of_edges(graph):
    """graph.number_of_edges() (networkx, fastgraph); for an AdjacencyWrapper -- which the reference never asks -- the stored entries
    when directed, and every undirected edge once (its two entries, or the one on the diagonal) when not."""
    counter = getattr(graph, "number_of_edges", None)
    if counter is not None:
        return counter()
    adjacency = graph_to_scipy(graph)
    if graph.is_directed():
        return adjacency.nnz
    return (adjacency.nnz + int(np.count_nonzero(adjacency.diagonal()))) / 2


class SeedOversampling(_Oversampler):
    """oversampling.py:9-61: ranks, grows the seed set from the outcome, ranks again.

    ranker: the base ranking algorithm.
    method: "safe" (default) -- every node that scores at least as high as the lowest-scored seed becomes a seed; "top" -- the
        int(n * n / edges) highest-scored nodes join the seeds; "neighbors" -- the seeds' neighbors join them (no preliminary run).
    ``SeedOversampling("top", ranker)`` and ``SeedOversampling(ranker, "top")`` are the same thing (oversampling.py:28-29).
    The personalization must hold zeros and ones only.  After a run ``last_seed_counts`` holds the size of every column's grown seed
    set and ``last_passes`` how many slab passes went through the engine's entries and how many through backend primitives."""

    _METHODS = ("safe", "neighbors", "top")

    def __init__(self, ranker=None, method="safe", fused=True, batch=True, min_batch_width=None):
        if ranker is not None and not _is_ranker(ranker):            # the method came first
            ranker, method = (method if _is_ranker(method) else None), ranker
        super().__init__(ranker, fused, batch, min_batch_width)
        self.method = str(method).lower()
        self._raw = default_preprocessor(normalization="none")       # the raw-adjacency image of "neighbors", as Unsupervised builds its own
        self._reset()

    def _reset(self):
        self.last_seed_counts = []

    @staticmethod
    def _assert_binary(seeds):                                      # preprocessing.py:155-163
        for column in seeds.columns():
            if int(round(((column == 0.0) + (column == 1.0)).sum())) != len(column):
                raise Exception("Binary ranks required")

    def _neighbors(self, graph, seeds, passes):
        adjacency = graph_to_scipy(graph)
        if adjacency.nnz and adjacency.data.min() < 0:
            # weights of both signs can cancel in A^T s: the rows of the seeds are read on the host instead
            import scipy.sparse as sp
            rows = sp.csr_array(adjacency)
            grown = np.array(seeds.numpy() == 1.0, dtype=np.float64)
            for c in range(seeds.b):
                for u in np.flatnonzero(grown[:, c]):
                    grown[rows.indices[rows.indptr[u]:rows.indptr[u + 1]], c] = 1.0
            grown = np.maximum(grown, seeds.numpy())
            return DeviceMatrix.from_host(grown), [int(v) for v in (grown == 1.0).sum(axis=0)]
        image = backend.conv(seeds, self._raw(graph))               # [A^T s > 0]: somebody with an edge to the node is a seed
        return passes.resample(_as_slab(image), [0.0] * seeds.b, strict=True, keep=seeds)

    def _loop(self, graph, seeds, passes, kwargs):
        self._assert_binary(seeds)
        method = self.method
        if method == "neighbors":
            grown, counts = self._neighbors(graph, seeds, passes)
        elif method == "safe":
            ranks = self._inner(graph, seeds, kwargs)
            floors, have = passes.floor(ranks, seeds)
            if not all(have):
                raise Exception("safe seed oversampling needs at least one seed")
            grown, counts = passes.resample(ranks, floors)
        elif method == "top":
            nodes = seeds.n
            top = int(nodes * nodes / _number_of_edges(graph))
            if not 1 <= top <= nodes:
                raise Exception(f"top seed oversampling would keep {top} of {nodes} nodes")
            ranks = self._inner(graph, seeds, kwargs)
            floors = [column.kth_largest(top) for column in ranks.columns()]
            grown, counts = passes.resample(ranks, floors, keep=seeds)
        else:
            raise Exception("Supported oversampling methods: safe, neighbors, top")
        self.last_seed_counts.extend(counts)
        return self._inner(graph, grown, kwargs)

    def _reference(self):
        return self.method + " seed oversampling \\cite{krasanakis2019boosted}"


class BoostedSeedOversampling(_Oversampler):
    """oversampling.py:64-130: oversamples the seeds round after round and adds the rounds' ranks up with boosting weights.

    ranker: the base ranking algorithm.
    objective: "partial" (default) or "naive", the rule of a round's weight a_N from the three sums S1 = sum s R^2, S2 = sum R^2,
        S3 = sum s RN R over the round's seeds s, its ranks R and the sum so far RN:  S1 / S2 - S3 / S2, or 0.5 - 0.5 S3 / S2.
    oversample_from_iteration: "previous" (default) -- the next threshold is the lowest score among the seeds of the round before;
        "original" -- among the nodes the personalization holds a 1 for.
    weight_convergence: stops the rounds on the weights; ConvergenceManager(error_type=MaxDifference, tol=0.001, max_iters=100) by
        default.  ``rank`` drives this very object; every column of a batch drives a copy of it.
    After a run ``last_rounds`` holds every column's rounds, ``last_weights`` and ``last_seed_counts`` its weight and the size of its
    seed set round by round, ``last_widths`` the live columns of every round of a chunk (ranked as one batch from ``min_batch_width``
    on), ``last_passes`` the slab passes by route."""

    def __init__(self, ranker=None, objective="partial", oversample_from_iteration="previous", weight_convergence=None, fused=True,
                 batch=True, min_batch_width=None):
        super().__init__(ranker, fused, batch, min_batch_width)
        self._objective = objective.lower()
        self._oversample_from_iteration = oversample_from_iteration.lower()
        self._weight_convergence = ConvergenceManager(error_type=MaxDifference, tol=0.001, max_iters=100) \
            if weight_convergence is None else weight_convergence
        self._reset()

    def _reset(self):
        self.last_rounds, self.last_weights, self.last_seed_counts, self.last_widths = [], [], [], []

    def _boosting_weight(self, S1, S2, S3):                          # oversampling.py:95-103
        if self._objective == "partial":
            return S1 / float(S2) - S3 / float(S2)
        if self._objective == "naive":
            return 0.5 - 0.5 * S3 / float(S2)
        raise Exception("Supported boosting objectives: partial, naive")

    def _loop(self, graph, seeds, passes, kwargs):
        source = self._oversample_from_iteration
        if self._objective not in ("partial", "naive"):
            raise Exception("Supported boosting objectives: partial, naive")
        if source not in ("previous", "original"):
            raise Exception("Boosting only supports oversampling from iterations: previous, original")
        b = seeds.b
        managers = [self._weight_convergence] if b == 1 else [copy.deepcopy(self._weight_convergence) for _ in range(b)]
        total = self._inner(graph, seeds, kwargs)                    # RN of the live columns, in place from here on
        floors, have = passes.floor(total, seeds)
        if not all(have):
            raise Exception("boosted seed oversampling needs a personalization with at least one entry equal to 1")
        out = None if b == 1 else DeviceMatrix.empty(seeds.n, b)
        live = list(range(b))                                        # the chunk's columns still in the batch, in slab order
        weights = {c: [] for c in live}
        sizes = {c: [] for c in live}
        widths = []
        for manager in managers:
            manager.start()
        original = seeds
        going = [not managers[c].has_converged(1) for c in live]     # a_N = 1 before the first round
        while True:
            if not all(going):
                # the finished columns leave: their sums go to the outcome, the others close ranks
                stay = [k for k, on in enumerate(going) if on]
                if out is not None:
                    for k, on in enumerate(going):
                        if not on:
                            out.set_column(live[k], total.column(k))
                elif not stay:
                    out = total
                if not stay:
                    break
                total, original = _take(total, stay), _take(original, stay)
                floors, live = [floors[k] for k in stay], [live[k] for k in stay]
            grown, counts = passes.resample(total, floors)
            fresh = self._inner(graph, grown, kwargs)
            widths.append(grown.b)
            sums = passes.forms(grown, fresh, total)
            step = [self._boosting_weight(*triple) for triple in sums]
            floors, _ = passes.update(total, fresh, step, grown if source == "previous" else original)
            going = []
            for k, c in enumerate(live):
                weights[c].append(float(step[k]))
                sizes[c].append(int(counts[k]))
                going.append(not managers[c].has_converged(float(step[k])))
        self.last_rounds.extend(len(weights[c]) for c in range(b))
        self.last_weights.extend(weights[c] for c in range(b))
        self.last_seed_counts.extend(sizes[c] for c in range(b))
        self.last_widths.append(widths)
        return out

    def _reference(self):
        return "iterative " + self._objective + " boosted seed oversampling of " + self._oversample_from_iteration + \
            " node scores \\cite{krasanakis2019boosted}"
