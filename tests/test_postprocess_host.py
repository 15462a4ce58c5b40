"""Postprocessor.propagate on the host test double (no GPU): the inner ranker's batch is kept -- ONE inner propagate, whatever wraps
it -- and every column comes out as ``transform`` of that batch's column.  The double lacks include/pgh_post.h, so the transformation
takes the "columns" route here, whatever `fused` says; tests/test_gpu_postprocess.py runs the same comparison on the slab route."""
import numpy as np
import pytest

import oversampling_common as oc
import postprocess_common as pc


@pytest.mark.parametrize("name", sorted(pc.EXACT))
@pytest.mark.parametrize("width", pc.WIDTHS)
@pytest.mark.parametrize("key", pc.GRAPHS)
def test_propagate_keeps_the_inner_batch(host_engine, key, width, name):
    from pygrank_amd import _lib as L
    assert all(L.entry(entry) is None for entry in L.POST_SIGNATURES)
    _, steps, _, _ = pc.check_propagate(host_engine, key, width, name, "columns")
    for step in steps:
        assert step.last_propagate["chunks"] == [width] and dict(step.last_propagate["calls"]) == {}


@pytest.mark.parametrize("name", ["Chain", "NormalizeRange", "Ordinals"])
def test_batch_false_is_the_column_loop_bit_for_bit(host_engine, name):
    pg = host_engine
    case = oc.Case(pg, "weighted300")
    F = pc.features(case.n, 3)
    post, steps = pc.build(pg, name, case.ranker(), case.n)
    post.batch = False
    got = post.propagate(case.graph, F).numpy()
    assert post.last_propagate["route"] == "ranks"
    again, _ = pc.build(pg, name, case.ranker(), case.n)
    loop = pg.NodeRanking.propagate(again, case.graph, F).numpy()          # today's propagate, as written
    assert np.array_equal(got, loop)
    for j in range(3):
        alone, _ = pc.build(pg, name, case.ranker(), case.n)
        ranks = np.asarray(alone.rank(case.graph, F[:, j].copy()).np, dtype=np.float64)
        assert np.array_equal(got[:, j], ranks)


def test_fused_false_changes_nothing_on_the_double(host_engine):
    _, _, _, on = pc.check_propagate(host_engine, "weighted300", 3, "Chain", "columns")
    _, _, _, off = pc.check_propagate(host_engine, "weighted300", 3, "Chain", "columns", fused=False)
    assert np.array_equal(on, off)


def test_a_leftover_keyword_raises(host_engine):
    pg = host_engine
    case = oc.Case(pg, "weighted300")
    F = pc.features(case.n, 3)
    # what the inner ranker did not take reaches _transform as rank passes it on: the option-less postprocessors refuse whatever arrives
    with pytest.raises(Exception, match="No usage of argument"):
        pg.Normalize(case.ranker()).rank(case.graph, F[:, 0].copy(), leftover=1)
    with pytest.raises(Exception, match="No usage of argument"):
        pg.Normalize(case.ranker()).propagate(case.graph, F, leftover=1)
    with pytest.raises(Exception, match="No usage of argument"):
        pg.Top(pg.Normalize(case.ranker()), 5).propagate(case.graph, F, leftover=1)
    # ... and a keyword no parameter of _transform is named after is dropped on the way, in propagate as in rank
    ranks = pg.Normalize(case.ranker()).rank(case.graph, F[:, 0].copy(), nobody_takes_this=1)
    many = pg.Normalize(case.ranker()).propagate(case.graph, F, nobody_takes_this=1).numpy()
    assert pc.within(many[:, 0], np.asarray(ranks.np, dtype=np.float64), False)


def test_zero_and_constant_columns_stay_as_rank_leaves_them(host_engine):
    pg = host_engine
    case = oc.Case(pg, "weighted300")
    F = pc.features(case.n, 4)
    F[:, 1] = 0.0                                                   # PageRank leaves a zero column zero; Normalize leaves it too
    for method in ("max", "sum", "L2", "range"):
        ranker = case.ranker()
        got = pg.Normalize(ranker, method).propagate(case.graph, F).numpy()
        assert len(ranker.last_batches) == 1 and not got[:, 1].any()
        for j in range(4):
            ranks = pg.Normalize(case.ranker(), method).rank(case.graph, F[:, j].copy())
            assert pc.within(got[:, j], np.asarray(ranks.np, dtype=np.float64), False)
    # without an inner ranker the features themselves are transformed: a constant column stays, per column
    G = np.abs(np.random.default_rng(3).normal(size=(case.n, 3)))
    G[:, 2] = 0.25
    for method in ("max", "sum", "L2", "range"):
        post = pg.Normalize(method=method)
        got = post.propagate(case.graph, G).numpy()
        assert post.last_propagate["route"] == "columns"
        for j in range(3):
            ranks = pg.Normalize(method=method).rank(case.graph, pg.to_signal(case.graph, G[:, j].copy()))
            assert np.array_equal(got[:, j], np.asarray(ranks.np, dtype=np.float64))
        if method == "range":
            assert np.array_equal(got[:, 2], np.full(case.n, np.float64(np.float32(0.25))))


def test_tautology_without_a_ranker_returns_the_features_as_a_slab(host_engine):
    pg = host_engine
    case = oc.Case(pg, "weighted300")
    F = pc.features(case.n, 3)
    got = pg.Tautology().propagate(case.graph, F)
    assert isinstance(got, pg.DeviceMatrix) and np.array_equal(got.numpy(), F)
    slab = pg.DeviceMatrix.from_host(F)
    assert pg.Tautology().propagate(case.graph, slab) is slab
    ranker = case.ranker()
    through = pg.Tautology(ranker).propagate(case.graph, F).numpy()
    assert len(ranker.last_batches) == 1
    assert np.array_equal(through, case.ranker().propagate(case.graph, F).numpy())


def test_a_user_subclass_with_only_a_transform_takes_the_old_loop(host_engine):
    pg = host_engine

    class Halve(pg.Postprocessor):
        def _transform(self, ranks):
            return ranks.np * 0.5

    class Shifted(pg.Normalize):                                    # changes what the slab form stands for
        def _values(self, ranks):
            return super()._values(ranks) + 1.0

    case = oc.Case(pg, "weighted300")
    F = pc.features(case.n, 3)
    for make in (Halve, Shifted):
        post = make(case.ranker())
        got = post.propagate(case.graph, F).numpy()
        assert post.last_propagate["route"] == "ranks"
        assert np.array_equal(got, pg.NodeRanking.propagate(make(case.ranker()), case.graph, F).numpy())


def test_create_many_variation_types(host_engine):
    pg = host_engine
    types = pg.create_many_variation_types()
    assert list(types) == ["", "Sweep", "O", "SweepO", "Neigh", "SweepNeigh"]
    case = oc.Case(pg, "rmat10_dir")
    ranker = case.ranker()
    wrapped = {name: make(ranker) for name, make in types.items()}
    assert isinstance(wrapped[""], pg.Tautology) and isinstance(wrapped["Sweep"], pg.Sweep)
    for name, method in (("O", "safe"), ("SweepO", "safe"), ("Neigh", "neighbors"), ("SweepNeigh", "neighbors")):
        assert isinstance(wrapped[name], pg.SeedOversampling) and wrapped[name].method == method
        assert isinstance(wrapped[name].ranker, pg.Sweep) == name.startswith("Sweep")
    assert sorted(pg.create_variations({"PPR": ranker}, types)) == sorted("PPR" + name for name in types)
    # SweepO: 8 seed sets, two rounds ("safe": a preliminary run, then the run on the grown seeds), ONE inner batch each
    F = pc.features(case.n, 8)
    batches, ranks = [], []
    propagate, rank = ranker.propagate, ranker.rank
    ranker.propagate = lambda *a, **k: (propagate(*a, **k), batches.append([len(b) for b in ranker.last_batches]))[0]
    ranker.rank = lambda *a, **k: (rank(*a, **k), ranks.append(1))[0]
    swept = wrapped["SweepO"]
    got = swept.propagate(case.graph, F).numpy()
    assert batches == [[8], [8]] and len(ranks) == 1                # (the one rank() is the sweep's baseline, once per graph)
    assert swept.ranker.last_propagate["route"] == "columns"
    for j in range(8):
        alone = types["SweepO"](case.ranker()).rank(case.graph, F[:, j].copy())
        assert oc.rel_linf(got[:, j], np.asarray(alone.np, dtype=np.float64)) <= oc.BAR
