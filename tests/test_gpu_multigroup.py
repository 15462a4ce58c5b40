"""LinkAssessment, ClusteringCoefficient, Modularity, MultiSupervised and MultiUnsupervised on the GPU: the fixture replay of
tests/test_multigroup_host.py on the device route with the same bounds, and the device route against fused=False on the slab of a real
multi-seed propagate."""
import warnings

import numpy as np
import pytest

import link_common as lc

pytestmark = pytest.mark.gpu

GRAPHS = ["weighted300", "rmat10_dir", "rmat12_sym", "er10k"]


@pytest.fixture(scope="module")
def fx():
    return lc.fixture()


@pytest.mark.parametrize("key", GRAPHS)
def test_golden_cases_on_the_device_route(gpu_engine, fx, key):
    inputs = lc.Inputs(gpu_engine, fx, key)
    lc.replay_link(inputs, "device")
    lc.replay_clustering(inputs, "device")
    for measure, _ in lc.replay_modularity(inputs):
        assert measure.last_route == "slab"
    lc.replay_multi(inputs)


@pytest.fixture(scope="module")
def propagated(gpu_engine):
    """The [n, 8] slab of one PageRank.propagate over 8 seed sets of rmat12_sym."""
    import cases
    pg = gpu_engine
    A, directed, _ = cases.GRAPHS["rmat12_sym"]()
    graph = pg.AdjacencyWrapper(A, directed=directed)
    n = A.shape[0]
    rng = np.random.default_rng(12)
    seeds = np.zeros((n, 8))
    for j in range(8):
        seeds[rng.choice(n, 40, replace=False), j] = 1.0
    slab = pg.PageRank(alpha=0.85, tol=1e-9, max_iters=1000).propagate(graph, pg.DeviceMatrix.from_host(seeds))
    assert isinstance(slab, pg.DeviceMatrix) and slab.shape == (n, 8)
    return graph, A, slab


def test_device_route_against_the_host_route_on_a_propagated_slab(gpu_engine, propagated):
    pg = gpu_engine
    graph, A, slab = propagated
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for similarity in ("cos", "dot"):
            for hops in (1, 2):
                kwargs = dict(similarity=similarity, hops=hops, max_positive_samples=300, max_negative_samples=500)
                device, host = pg.LinkAssessment(graph, **kwargs), pg.LinkAssessment(graph, fused=False, **kwargs)
                got, want = device.evaluate(slab), host.evaluate(slab)
                print(f"link {similarity} hops {hops}: device {got!r} host {want!r} pairs {device.plan().num_pairs}")
                assert (device.last_route, host.last_route) == ("device", "host")
                assert got == want                          # equal to the bit
                predicted, _ = device.predictions(slab)
                assert device.last_route == "device"
                assert np.array_equal(predicted.view(np.uint64), host.predictions(slab)[0].view(np.uint64))
            device, host = pg.ClusteringCoefficient(graph, similarity=similarity), pg.ClusteringCoefficient(graph, similarity=similarity, fused=False)
            got, want = device.evaluate(slab), host.evaluate(slab)
            print(f"clustering {similarity}: device {got!r} host {want!r}")
            assert (device.last_route, host.last_route) == ("device", "host") and lc.close(got, want)
            assert lc.close(want, lc.clustering(A, slab.numpy(), similarity, 2000, 1), 1e-12)
    S = slab.numpy()
    for max_positive in (500, 5000):
        device, host = pg.Modularity(graph, max_positive_samples=max_positive), pg.Modularity(graph, max_positive_samples=max_positive, fused=False)
        got, want = device.evaluate_many(slab), host.evaluate_many(slab)
        assert (device.last_route, host.last_route) == ("slab", "columns")
        looped = [device.evaluate(column) for column in slab.columns()]
        for j in range(slab.b):
            internal, expected, m = lc.modularity_terms(A, False, S[:, j], 1, max_positive, 0)
            bound = lc.PARITY * (internal + expected) / 2 / m
            print(f"modularity samples {max_positive} column {j}: slab {got[j]!r} columns {want[j]!r} loop {looped[j]!r} bound {bound:.3e}")
            assert abs(got[j] - want[j]) <= bound and abs(got[j] - (internal - expected) / 2 / m) <= bound
            assert abs(looped[j] - got[j]) <= bound         # evaluate_many against a loop over evaluate


def test_a_second_evaluate_builds_no_second_plan(gpu_engine, propagated, monkeypatch):
    from pygrank_amd import _lib as L
    pg = gpu_engine
    graph, _, slab = propagated
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        measure = pg.LinkAssessment(graph, max_positive_samples=100, max_negative_samples=100)
        first = measure.evaluate(slab)
        handle = measure.plan()._h
        assert handle is not None
        assert measure.evaluate(slab) == first and measure.plans_built == 1 and measure.plan()._h is handle
        # non-finite scores: what sklearn says to the reference
        bad = slab.numpy()
        bad[:, -1] = np.inf                                 # inf / inf under "cos"
        with pytest.raises(ValueError, match="Input contains NaN"):
            measure.evaluate(pg.DeviceMatrix.from_host(bad))
        # more pairs than a plan holds: the Python layer says so and suggests smaller samples
        fresh = pg.LinkAssessment(graph, max_positive_samples=100, max_negative_samples=100)
        monkeypatch.setattr(L, "LINK_MAX_PAIRS", 10)
        with pytest.raises(Exception, match="take smaller max_positive_samples"):
            fresh.evaluate(slab)
