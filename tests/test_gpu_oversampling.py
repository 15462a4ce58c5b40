"""pg.SeedOversampling and pg.BoostedSeedOversampling on the GPU against the reference's recorded vectors
(tests/golden/golden_oversampling.npz): the golden cases through rank(), the fused route (include/pgh_oversample.h) against the same
rule in backend primitives, and a three-column propagate() whose columns leave the batch one after the other.

Bars: the project's rel-Linf 1e-6 against the fixture, with the reference's round counts and seed counts (the fixture's generator keeps
every threshold, weight step and inner stopping test clear of its tolerance and asserts the same bar for a numpy evaluation with f32
storage).  The two routes differ in the update's arithmetic alone -- f64 with one rounding against pgh_axpby's f32 -- a relative 2^-23
per round on weights that sum to less than 4: they are held to the same bar against each other."""
import numpy as np
import pytest

import oversampling_common as oc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("method", oc.SO_METHODS)
@pytest.mark.parametrize("key", oc.GRAPHS)
def test_seed_oversampling_golden_case(gpu_engine, key, method):
    algo, _ = oc.Case(gpu_engine, key).check_seed_oversampling(method)
    assert algo.last_passes == dict(fused=1 + int(method == "safe"), primitive=0)


@pytest.mark.parametrize("objective,source", oc.BOOSTED)
@pytest.mark.parametrize("key", oc.GRAPHS)
def test_boosted_golden_case(gpu_engine, key, objective, source):
    algo, _ = oc.Case(gpu_engine, key).check_boosted(objective, source)
    assert algo.last_passes == dict(fused=1 + 3 * algo.last_rounds[0], primitive=0)


def test_f64_case(gpu_engine):
    key, objective, source = oc.TIGHT
    case = oc.Case(gpu_engine, key)
    case.check_boosted(objective, source, tag="_tol1e-9", ranker=case.ranker(tol=1e-9))


@pytest.mark.parametrize("which", ["safe", "top", "neighbors", "partial previous", "naive original"])
@pytest.mark.parametrize("key", ["rmat10_dir", "weighted300"])
def test_fused_against_primitives(gpu_engine, key, which):
    case = oc.Case(gpu_engine, key)
    if which in oc.SO_METHODS:
        run = lambda **kw: case.seed_oversampling(which, **kw)                       # noqa: E731
    else:
        run = lambda **kw: case.boosted(*which.split(), **kw)                         # noqa: E731
    on, fused = run(fused=True)
    off, plain = run(fused=False)
    worst = oc.rel_linf(fused, plain)
    print(key, which, "fused against primitives: rel-Linf", worst, "passes", on.last_passes, off.last_passes)
    assert on.last_passes["primitive"] == 0 and on.last_passes["fused"] > 0
    assert off.last_passes["fused"] == 0 and off.last_passes["primitive"] == on.last_passes["fused"]
    assert on.last_seed_counts == off.last_seed_counts
    if which not in oc.SO_METHODS:
        assert on.last_rounds == off.last_rounds
        assert np.allclose(on.last_weights[0], off.last_weights[0], rtol=0, atol=1e-5)
    assert worst <= oc.BAR


def test_propagate_against_the_columns_one_by_one(gpu_engine):
    pg = gpu_engine
    fx, case = oc.fixture(), oc.Case(pg, oc.MULTI)
    F = oc.multi_features()
    want_rounds = [int(r) for r in fx[f"{oc.MULTI}/multi/rounds"]]
    assert want_rounds[0] > want_rounds[1] > want_rounds[2]

    class Recording(pg.PageRank):
        """the widths of every multi-seed batch the inner ranker ran"""
        widths = None

        def propagate(self, *args, **kwargs):
            out = super().propagate(*args, **kwargs)
            self.widths.append([len(batch) for batch in self.last_batches])
            return out
    inner = Recording(error_type=pg.L1, **oc.RANKER)
    inner.widths = []
    batch = pg.BoostedSeedOversampling(inner, min_batch_width=2)           # three columns are below the default MIN_BATCH_WIDTH
    got = batch.propagate(case.graph, F)
    assert isinstance(got, pg.DeviceMatrix) and got.shape == F.shape
    got = got.numpy()
    print("rounds", batch.last_rounds, "widths", batch.last_widths, "inner batches", inner.widths)
    assert batch.last_rounds == want_rounds
    # the first run and the rounds all three columns share, then two columns, then the last one through rank()
    assert inner.widths == [[3]] * (1 + want_rounds[2]) + [[2]] * (want_rounds[1] - want_rounds[2])
    assert batch.last_widths == [[3] * want_rounds[2] + [2] * (want_rounds[1] - want_rounds[2]) + [1] * (want_rounds[0] - want_rounds[1])]
    assert batch.last_passes["primitive"] == 0
    single = pg.BoostedSeedOversampling(case.ranker(), batch=False)
    one_by_one = single.propagate(case.graph, F).numpy()
    assert single.last_rounds == want_rounds and single.last_seed_counts == batch.last_seed_counts
    for j in range(3):
        worst = oc.rel_linf(got[:, j], one_by_one[:, j]), oc.rel_linf(got[:, j], fx[f"{oc.MULTI}/multi/ranks"][:, j])
        print("column", j, "batch against one by one", worst[0], "against the reference", worst[1])
        assert max(worst) <= oc.BAR
    so = pg.SeedOversampling(case.ranker(), "top", min_batch_width=2)
    many = so.propagate(case.graph, F).numpy()
    for j in range(3):
        alone = pg.SeedOversampling(case.ranker(), "top")
        ranks = np.asarray(alone.rank(case.graph, pg.to_signal(case.graph, F[:, j].copy())).np, dtype=np.float64)
        assert alone.last_seed_counts == [so.last_seed_counts[j]]
        assert oc.rel_linf(many[:, j], ranks) <= oc.BAR
