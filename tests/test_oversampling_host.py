"""pg.SeedOversampling and pg.BoostedSeedOversampling on the host test double (no GPU) against the reference's recorded vectors
(tests/golden/golden_oversampling.npz).  The double lacks include/pgh_oversample.h, so every run here takes the backend-primitive route,
whatever `fused` says; one test swaps numpy evaluations of the four entries in to drive the fused route's host side."""
import numpy as np
import pytest
import scipy.sparse as sp

import oversampling_common as oc


@pytest.mark.parametrize("method", oc.SO_METHODS)
@pytest.mark.parametrize("key", oc.GRAPHS)
def test_seed_oversampling_golden_case(host_engine, key, method):
    from pygrank_amd import _lib as L
    assert all(L.entry(name) is None for name in L.OVERSAMPLE_SIGNATURES)
    algo, _ = oc.Case(host_engine, key).check_seed_oversampling(method)
    assert algo.last_passes["fused"] == 0


@pytest.mark.parametrize("objective,source", oc.BOOSTED)
@pytest.mark.parametrize("key", oc.GRAPHS)
def test_boosted_golden_case(host_engine, key, objective, source):
    algo, _ = oc.Case(host_engine, key).check_boosted(objective, source)
    assert algo.last_passes["fused"] == 0 and algo.last_passes["primitive"] == 1 + 3 * algo.last_rounds[0]
    assert algo._weight_convergence.iteration == algo.last_rounds[0] + 1       # rank() drives the manager itself


def test_f64_case(host_engine):
    """Around PageRank(tol=1e-9) the inner ranker takes the f64 loops."""
    key, objective, source = oc.TIGHT
    case = oc.Case(host_engine, key)
    case.check_boosted(objective, source, tag="_tol1e-9", ranker=case.ranker(tol=1e-9))


@pytest.mark.parametrize("which", ["safe", "top", "neighbors", "boosted"])
def test_fused_flag_changes_nothing_on_the_double(host_engine, which):
    case = oc.Case(host_engine, "weighted300")
    run = (lambda **kw: case.boosted("naive", "original", **kw)) if which == "boosted" else (lambda **kw: case.seed_oversampling(which, **kw))
    on, a = run(fused=True)
    off, b = run(fused=False)
    assert np.array_equal(a, b) and on.last_passes == off.last_passes and on.last_seed_counts == off.last_seed_counts


def test_propagate_equals_the_columnwise_rank(host_engine):
    pg = host_engine
    fx, case = oc.fixture(), oc.Case(host_engine, oc.MULTI)
    F = oc.multi_features()
    batch = pg.BoostedSeedOversampling(case.ranker(), min_batch_width=2)
    got = batch.propagate(case.graph, F)
    assert isinstance(got, pg.DeviceMatrix)
    got = got.numpy()
    want_rounds = [int(r) for r in fx[f"{oc.MULTI}/multi/rounds"]]
    print("rounds", batch.last_rounds, "widths", batch.last_widths)
    assert batch.last_rounds == want_rounds and len(set(want_rounds)) == 3
    assert batch.last_widths == [[3] * want_rounds[2] + [2] * (want_rounds[1] - want_rounds[2]) + [1] * (want_rounds[0] - want_rounds[1])]
    assert batch._weight_convergence.iteration == 0                  # the columns of a batch drive copies
    single = pg.BoostedSeedOversampling(case.ranker(), batch=False)
    one_by_one = single.propagate(case.graph, F).numpy()
    assert single.last_rounds == want_rounds and single.last_widths == [[1] * r for r in want_rounds]
    for j in range(3):
        alone = pg.BoostedSeedOversampling(case.ranker())
        ranks = np.asarray(alone.rank(case.graph, pg.to_signal(case.graph, F[:, j].copy())).np, dtype=np.float64)
        assert np.array_equal(ranks, one_by_one[:, j])
        assert oc.rel_linf(got[:, j], ranks) <= oc.BAR
        assert oc.rel_linf(got[:, j], fx[f"{oc.MULTI}/multi/ranks"][:, j]) <= oc.BAR
    # three columns are below the default MIN_BATCH_WIDTH: the same slab loop, the inner ranker column by column -- rank()'s own bits
    narrow = pg.BoostedSeedOversampling(case.ranker())
    assert pg.BoostedSeedOversampling.MIN_BATCH_WIDTH > 3 and narrow.min_batch_width is None
    assert np.array_equal(narrow.propagate(case.graph, F).numpy(), one_by_one) and narrow.last_widths == batch.last_widths
    # SeedOversampling has the same batch
    so = pg.SeedOversampling(case.ranker(), "safe", min_batch_width=2)
    many = so.propagate(case.graph, F).numpy()
    for j in range(3):
        alone = pg.SeedOversampling(case.ranker(), "safe")
        ranks = np.asarray(alone.rank(case.graph, pg.to_signal(case.graph, F[:, j].copy())).np, dtype=np.float64)
        assert alone.last_seed_counts == [so.last_seed_counts[j]]
        assert oc.rel_linf(many[:, j], ranks) <= oc.BAR


def test_a_ranker_without_a_batch_falls_back_to_its_column_loop(host_engine):
    pg = host_engine
    case = oc.Case(host_engine, "weighted300")
    F = np.zeros((case.n, 2))
    F[list(case.seeds), 0] = 1.0
    F[[1, 2, 3], 1] = 1.0
    inner = pg.Normalize(case.ranker(), "sum")                       # a postprocessor: NodeRanking.propagate, one rank() per column
    got = pg.BoostedSeedOversampling(inner, "naive", "original", min_batch_width=2).propagate(case.graph, F).numpy()
    for j in range(2):
        ranks = pg.BoostedSeedOversampling(pg.Normalize(case.ranker(), "sum"), "naive", "original").rank(case.graph, F[:, j].copy())
        assert oc.rel_linf(got[:, j], np.asarray(ranks.np, dtype=np.float64)) <= oc.BAR


def test_refusals(host_engine):
    pg = host_engine
    case = oc.Case(pg, "weighted300")
    graph, signal = case.graph, case.signal()
    fractional = pg.to_signal(graph, {**case.seeds, 7: 0.5})
    for method in oc.SO_METHODS:
        with pytest.raises(Exception, match="Binary ranks required"):
            pg.SeedOversampling(case.ranker(), method).rank(graph, fractional)
    with pytest.raises(Exception, match="Supported oversampling methods: safe, neighbors, top"):
        pg.SeedOversampling(case.ranker(), "best").rank(graph, signal)
    pg.SeedOversampling(case.ranker(), "best")                      # ... only at rank
    with pytest.raises(Exception, match="Supported boosting objectives: partial, naive"):
        pg.BoostedSeedOversampling(case.ranker(), objective="full").rank(graph, signal)
    with pytest.raises(Exception, match="Boosting only supports oversampling from iterations: previous, original"):
        pg.BoostedSeedOversampling(case.ranker(), oversample_from_iteration="first").rank(graph, signal)
    with pytest.raises(Exception, match="at least one entry equal to 1"):
        pg.BoostedSeedOversampling(case.ranker()).rank(graph, pg.to_signal(graph, {3: 0.5, 4: 2.0}))
    # top = int(n * n / edges) outside 1 .. n: four nodes and two edges ask for the top 8
    sparse = pg.AdjacencyWrapper(sp.csr_array(np.array([[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0.]])), directed=True)
    with pytest.raises(Exception, match="top seed oversampling"):
        pg.SeedOversampling(case.ranker(), "top").rank(sparse, {0: 1.0})


def test_number_of_edges_of_an_adjacency_wrapper(host_engine):
    from pygrank_amd.oversampling import _number_of_edges
    A = sp.csr_array(np.array([[1, 1, 0], [1, 0, 1], [0, 1, 0.]]))
    assert _number_of_edges(host_engine.AdjacencyWrapper(A, directed=True)) == 5
    assert _number_of_edges(host_engine.AdjacencyWrapper(A, directed=False)) == 3      # two edges and one self-loop


def test_neighbors_with_a_negative_weight_take_the_host_route(host_engine):
    pg = host_engine
    A = sp.csr_array(np.array([[0, 1, -1, 0], [0, 0, 1, 0], [1, 0, 0, 1], [0, 0, 0, 0.]]))
    B = abs(A)
    seeds = {0: 1.0}
    ranker = lambda: pg.PageRank(alpha=0.5, tol=1e-6, max_iters=1000, normalization=lambda M: abs(M))   # noqa: E731
    signed = pg.SeedOversampling(ranker(), "neighbors")
    signed.rank(pg.AdjacencyWrapper(A, directed=True), seeds)
    plain = pg.SeedOversampling(ranker(), "neighbors")
    plain.rank(pg.AdjacencyWrapper(B, directed=True), seeds)
    assert signed.last_seed_counts == plain.last_seed_counts == [3]   # nodes 0, 1 and 2
    assert signed.last_passes == dict(fused=0, primitive=0) and plain.last_passes["primitive"] == 1


def test_references_and_cite(host_engine):
    pg = host_engine
    inner = pg.PageRank(0.9)
    for method in oc.SO_METHODS:
        assert pg.SeedOversampling(inner, method)._reference() == method + " seed oversampling \\cite{krasanakis2019boosted}"
    assert pg.SeedOversampling(inner).references() == inner.references() + ["safe seed oversampling \\cite{krasanakis2019boosted}"]
    chained = pg.PageRank(0.9) >> pg.SeedOversampling("TOP")          # arguments in either order, the method in any case
    assert chained.method == "top" and isinstance(chained.ranker, pg.PageRank)
    assert pg.SeedOversampling("top", inner).ranker is inner and pg.SeedOversampling(inner, "top").method == "top"
    assert chained.cite() == inner.cite() + " with top seed oversampling \\cite{krasanakis2019boosted}"
    boosted = pg.BoostedSeedOversampling(inner, "Naive", "Original")
    assert boosted.references()[-1] == "iterative naive boosted seed oversampling of original node scores \\cite{krasanakis2019boosted}"
    assert pg.BoostedSeedOversampling(inner)._reference() == \
        "iterative partial boosted seed oversampling of previous node scores \\cite{krasanakis2019boosted}"
    manager = pg.BoostedSeedOversampling(inner)._weight_convergence
    assert manager.error_type is pg.MaxDifference and manager.tol == 0.001 and manager.max_iters == 100


def test_create_variations(host_engine):
    pg = host_engine
    case = oc.Case(pg, "weighted300")
    algorithms = {"ppr": case.ranker(), "hk": pg.HeatKernel(t=3)}
    family = pg.create_variations(algorithms, {"+SO": pg.SeedOversampling, "+BSO": pg.BoostedSeedOversampling})
    assert sorted(family) == ["hk+BSO", "hk+SO", "ppr+BSO", "ppr+SO"]
    assert isinstance(family["ppr+SO"], pg.SeedOversampling) and family["ppr+SO"].ranker is algorithms["ppr"]
    assert isinstance(family["hk+BSO"], pg.BoostedSeedOversampling) and family["hk+BSO"].ranker is algorithms["hk"]
    got = np.asarray(family["ppr+SO"].rank(case.graph, case.signal()).np, dtype=np.float64)
    assert oc.rel_linf(got, oc.fixture()["weighted300/so_safe/ranks"]) <= oc.BAR


@pytest.mark.parametrize("which", ["safe", "top", "neighbors", "partial previous", "naive original", "propagate"])
def test_fused_route_with_numpy_entries(host_engine, which):
    """The fused route's host side on the double, the four entries replaced by numpy evaluations of their header."""
    pg = host_engine
    from pygrank_amd import _lib as L
    cdll = L.lib()
    assert L.entry("pgh_seed_floor") is None
    calls = {name: 0 for name in L.OVERSAMPLE_SIGNATURES}

    def counted(fn, name):
        def call(*args):
            calls[name] += 1
            return fn(*args)
        return call
    saved = cdll._pgh_oversample_entries
    cdll._pgh_oversample_entries = {name: counted(fn, name) for name, fn in oc.numpy_entries(cdll).items()}
    try:
        if which in oc.SO_METHODS:
            algo, _ = oc.Case(pg, "rmat10_dir").check_seed_oversampling(which)
            assert calls == dict(pgh_seed_floor=int(which == "safe"), pgh_seed_resample=1, pgh_boost_forms=0, pgh_boost_update=0)
            assert algo.last_passes == dict(fused=1 + int(which == "safe"), primitive=0)
        elif which == "propagate":
            fx, case = oc.fixture(), oc.Case(pg, oc.MULTI)
            algo = pg.BoostedSeedOversampling(case.ranker(), min_batch_width=2)
            got = algo.propagate(case.graph, oc.multi_features()).numpy()
            rounds = [int(r) for r in fx[f"{oc.MULTI}/multi/rounds"]]
            assert algo.last_rounds == rounds and algo.last_passes["primitive"] == 0
            assert calls == dict(pgh_seed_floor=1, pgh_seed_resample=rounds[0], pgh_boost_forms=rounds[0], pgh_boost_update=rounds[0])
            for j in range(3):
                assert oc.rel_linf(got[:, j], fx[f"{oc.MULTI}/multi/ranks"][:, j]) <= oc.BAR
        else:
            objective, source = which.split()
            algo, _ = oc.Case(pg, "rmat10_dir").check_boosted(objective, source)
            rounds = algo.last_rounds[0]
            assert calls == dict(pgh_seed_floor=1, pgh_seed_resample=rounds, pgh_boost_forms=rounds, pgh_boost_update=rounds)
            assert algo.last_passes == dict(fused=1 + 3 * rounds, primitive=0)
    finally:
        cdll._pgh_oversample_entries = saved


def test_a_declined_entry_sends_the_rest_of_the_run_to_the_primitives(host_engine):
    pg = host_engine
    from pygrank_amd import _lib as L
    cdll = L.lib()
    assert L.entry("pgh_boost_update") is None
    entries = oc.numpy_entries(cdll)
    updates = []

    def update(*args):
        updates.append(1)
        return L.DECLINED if len(updates) == 2 else entries["pgh_boost_update"](*args)
    saved = cdll._pgh_oversample_entries
    cdll._pgh_oversample_entries = dict(entries, pgh_boost_update=update)
    try:
        algo, _ = oc.Case(pg, "rmat10_dir").check_boosted("partial", "previous")
        rounds = algo.last_rounds[0]
        assert len(updates) == 2                                      # nothing fused after the decline
        assert algo.last_passes == dict(fused=1 + 3 + 2, primitive=1 + 3 * (rounds - 2))
    finally:
        cdll._pgh_oversample_entries = saved
