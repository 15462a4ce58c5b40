"""The supervised measures on the GPU: the reference's recorded values (tests/golden/golden_supervised.json) through the real library
on the slab route (pgh_pair_forms; AUC and MannWhitneyParity: pgh_probe_auc) and, under measures._FORCE_PER_COLUMN, on the columns
route.  Both routes are held to the bound of tests/test_supervised_host.py against the reference (16 * 2^-24 relative, divided by the
generator's conditioning floor for KLDivergence / MKLDivergence, PearsonCorrelation and TNR) and to twice that bound against each
other; no other case has a bound of its own (BinaryCrossEntropy on pagerank_max: the base is built as the reference builds it, x / max x
with the largest entry exactly 1 -- supervised_common.Bases).  AUC.evaluate_many equals AUC.evaluate per column exactly, and the classes that existed before return what they
returned."""
import ctypes as C
import math

import numpy as np
import pytest

import supervised_common as sc

pytestmark = pytest.mark.gpu

GRAPHS = ["er10k", "rmat10_dir", "weighted300"]


@pytest.fixture(scope="module")
def fx():
    return sc.fixture()


@pytest.fixture(scope="module")
def all_bases(gpu_engine, fx):
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = sc.Bases(gpu_engine, fx, key)
        return cache[key]
    return get


@pytest.fixture()
def per_column():
    from pygrank_amd import measures

    def force(value):
        measures._FORCE_PER_COLUMN = value
    yield force
    measures._FORCE_PER_COLUMN = False


@pytest.mark.parametrize("key", GRAPHS)
def test_golden_cases_on_both_routes(gpu_engine, fx, all_bases, per_column, key):
    from pygrank_amd import _lib as L
    assert L.entry("pgh_pair_forms") is not None
    bases = all_bases(key)
    columns = [bases.signals[base] for base in sc.BASES]
    for excluded in (False, True):
        for name in sc.NEW + sc.EXISTING:
            per_column(False)
            slab = sc.check_many(bases, fx, name, excluded, "slab")
            one = bases.measure(name, excluded).evaluate(columns[1])
            if name in sc.NEW and name != "MannWhitneyParity":
                # evaluate of a new class is the one-column case of the same machinery
                assert sc.agrees(one, bases.cases(name, excluded)[1], sc.bound(fx, name)), (name, one)
            per_column(True)
            cols = sc.check_many(bases, fx, name, excluded, "columns")
            per_column(False)
            tol = 2 * sc.bound(fx, name)
            for a, b, case in zip(slab, cols, bases.cases(name, excluded)):
                if math.isfinite(a) and math.isfinite(b):
                    assert abs(a - b) <= tol * max(abs(a), abs(b)), (key, name, case, a, b)
                else:
                    assert sc.same(a, b), (key, name, case, a, b)


@pytest.mark.parametrize("b", [1, 5, 64])
def test_auc_of_a_slab_equals_auc_per_column(gpu_engine, fx, all_bases, b):
    pg = gpu_engine
    bases = all_bases("rmat10_dir")
    n = len(bases.graph)
    rng = np.random.default_rng(40 + b)
    host = rng.random((n, b))
    host[:, 0] = np.round(host[:, 0] * 8) / 8                              # ties
    if b > 1:
        host[:, 1] = 0                                                     # one tie group: 0.5
    slab = pg.DeviceMatrix.from_host(host)
    for excluded in (False, True):
        for name in ("AUC", "MannWhitneyParity"):
            measure = bases.measure(name, excluded)
            many = measure.evaluate_many(slab)
            assert measure.last_route == "slab" and len(many) == b
            singles = [bases.measure(name, excluded).evaluate(pg.to_signal(bases.graph, column)) for column in slab.columns()]
            assert many == singles, (name, excluded, many, singles)
            if b > 1:
                assert many[1] == (0.5 if name == "AUC" else 1.0)
    # known scores per column: no shared plan, one pgh_auc per column
    per_known = pg.DeviceMatrix.from_columns([bases.known.np for _ in range(b)])
    measure = pg.AUC(per_known)
    assert measure.evaluate_many(slab) == [pg.AUC(bases.known).evaluate(pg.to_signal(bases.graph, c)) for c in slab.columns()]
    assert measure.last_route == "columns"


def test_known_scores_and_exclude_values_per_column(gpu_engine, fx, all_bases):
    pg = gpu_engine
    bases = all_bases("weighted300")
    columns = [bases.signals[base] for base in sc.BASES]
    excluded_signal = pg.to_signal(bases.graph, {v: 1.0 for v in bases.exclude})
    per_known = pg.DeviceMatrix.from_columns([bases.known.np for _ in columns])
    per_exclude = pg.DeviceMatrix.from_columns([excluded_signal.np for _ in columns])
    for name in ("PPV", "BinaryCrossEntropy", "L1", "KLDivergence"):
        shared = bases.measure(name, True)
        want = shared.evaluate_many(columns)
        # excluding needs a graph (as evaluate does): the score columns are its signals, packed into a slab by evaluate_many
        measure = getattr(pg, name)(per_known, per_exclude)
        got = measure.evaluate_many(columns)
        assert shared.last_route == measure.last_route == "slab"
        assert all(sc.same(a, b) for a, b in zip(got, want)), (name, got, want)      # the same rows in the same order: the same bits
        # a slab of plain columns against known scores per column, nothing excluded
        shared = bases.measure(name, False)
        want = shared.evaluate_many(columns)
        measure = getattr(pg, name)(per_known)
        got = measure.evaluate_many(pg.DeviceMatrix.from_columns([c.np for c in columns]))
        assert shared.last_route == measure.last_route == "slab"
        assert all(sc.same(a, b) for a, b in zip(got, want)), (name, got, want)
        # and a slab of plain columns has no graph to exclude nodes by, whatever holds the exclude values
        with pytest.raises(Exception, match="to be able to exclude"):
            getattr(pg, name)(per_known, per_exclude).evaluate_many(pg.DeviceMatrix.from_columns([c.np for c in columns]))
    # 65 columns: 64 and 1
    many = [bases.signals["pagerank_max"] * (0.25 + 0.01 * j) for j in range(65)]
    for name in ("Accuracy", "KLDivergence", "Cos"):
        measure = bases.measure(name, True)
        got = measure.evaluate_many(many)
        assert measure.last_route == "slab" and len(got) == 65
        tol = 2 * sc.bound(fx, name)
        for value, column in zip(got, many):
            want = bases.measure(name, True).evaluate_many([column])[0]
            assert abs(value - want) <= tol * abs(want), (name, value, want)


def test_existing_classes_return_what_they_returned(gpu_engine, fx, all_bases):
    pg = gpu_engine
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceVector
    bases = all_bases("er10k")
    # plain vectors in HBM (the stored f32 values, uploaded again): no unevaluated expression, no resident iterate
    scores = pg.to_signal(bases.graph, DeviceVector.from_host(np.asarray(bases.signals["pagerank_max"].np)))
    known = pg.to_signal(bases.graph, DeviceVector.from_host(np.asarray(bases.known.np)))
    for cls, kind, finish in ((pg.Mabs, L.ERR_MABS, lambda v: v), (pg.L1, L.ERR_L1, lambda v: v), (pg.MaxDifference, L.ERR_LINF, lambda v: v),
                              (pg.RMabs, L.ERR_L1, lambda v: v / known.np.abssum())):
        out = C.c_double()
        L.check(L.lib().pgh_residual(kind, known.np._h, scores.np._h, C.byref(out)))
        assert cls(known).evaluate(scores) == finish(out.value), cls.__name__
    assert pg.Dot(known).evaluate(scores) == known.np.dot(scores.np)
    out, positives = C.c_double(), C.c_int64()
    L.check(L.lib().pgh_auc(known.np._h, scores.np._h, C.byref(out), C.byref(positives)))
    assert pg.AUC(known).evaluate(scores) == out.value
