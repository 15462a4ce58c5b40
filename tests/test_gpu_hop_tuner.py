"""HopTuner and arnoldi_iteration on the GPU against the reference's recorded behaviour (tests/golden/golden_hop.npz; the bounds are
those of tests/hop_common.py): the fused route -- the hop sweep on slabs, the two-pass Arnoldi step of include/pgh_arnoldi.h, an offset
step's candidates in one pass -- and, within the same bounds, the primitive route beside it."""
import numpy as np
import pytest

import hop_common as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return hc.fixture()


@pytest.mark.parametrize("variant", [name for name in hc.VARIANTS if name not in hc.OFFSET_VARIANTS])
def test_variant_follows_the_reference_on_the_fused_route(gpu_engine, fx, variant):
    tuner = hc.check_variant(gpu_engine, fx, variant, "fused")
    stats, hops = tuner.last_tune, hc.VARIANTS[variant][3] + hc.VARIANTS[variant][4]
    assert stats["scoring"] == ["slab", "slab"], stats
    if hc.VARIANTS[variant][2] == "krylov":
        assert stats["sweep"] == "steps" and stats["slab_passes"] == 2 and stats["products"] == 2 * (hops - 1)
    else:
        assert stats["sweep"] == "arnoldi:fused"
        assert stats["products"] == 3 * (hops - 1) and stats["slab_passes"] == 2 + 3 * 2 * (hops - 1)     # two halves and the final basis


@pytest.mark.parametrize("variant", ["rmat12/cos/krylov/10", "rmat12/auc/krylov/10", "rmat12/cos/arnoldi/10", "rmat12/auc/arnoldi/10",
                                     "rmat12/cos/krylov/8+3", "w300/cos/arnoldi/10"])
def test_primitive_route_agrees_within_the_same_bounds(gpu_engine, fx, variant):
    tuner = hc.check_variant(gpu_engine, fx, variant, "primitive", fused=False)
    assert set(tuner.last_tune["scoring"]) == {"columns"}


@pytest.mark.parametrize("variant", hc.OFFSET_VARIANTS)
def test_offset_search_reaches_the_reference_loss(gpu_engine, fx, variant):
    tuner = hc.check_offset(gpu_engine, fx, variant, "fused")
    assert tuner.last_tune["fused_steps"] >= 1 and tuner.last_tune["unfused_steps"] == 0, tuner.last_tune
    hc.check_offset(gpu_engine, fx, variant, "primitive", fused=False)


@pytest.mark.parametrize("key", sorted(hc.GRAPHS))
@pytest.mark.parametrize("k", hc.ARNOLDI_DIMS)
def test_arnoldi_iteration_follows_the_reference(gpu_engine, fx, key, k):
    hc.check_arnoldi(gpu_engine, fx, key, k, True, "fused")
    hc.check_arnoldi(gpu_engine, fx, key, k, False, "primitive")


def test_arnoldi_fallbacks_and_an_exhausted_space(gpu_engine, fx):
    pg = gpu_engine
    from pygrank_amd import krylov
    graph, signal = hc.graph_and_signal(pg, fx, "w300")
    M = pg.GenericGraphFilter([1.0]).preprocessor(graph)
    # more than 64 columns and a host vector take the primitive loop; nothing raises
    assert krylov.arnoldi_run(M, signal.np, 65, True)[2] == "primitive"
    host = np.asarray(signal.np, dtype=np.float64)
    Q, h, route = krylov.arnoldi_run(M, host, 6, True)
    assert route == "primitive"
    want = fx["w300/arnoldi_Q"][:, :6]
    assert float(np.abs(Q.numpy() - want).max() / np.abs(want).max()) <= hc.FACTOR * float(fx["w300/arnoldi_Q_dev_primitive/6"])
    # a node without out-edges (id % 10 == 3) spans a space of one dimension: the product vanishes, zero columns follow
    alone = pg.to_signal(graph, {3: 1.0})
    for fused, route in ((True, "fused"), (False, "primitive")):
        Q, h, took = krylov.arnoldi_run(M, alone.np, 4, fused)
        Q = Q.numpy()
        assert took == route and Q[3, 0] == 1.0 and not Q[:, 1:].any() and not np.array(h, dtype=np.float64).any(), (fused, h)


def test_default_tuner_returns_zero_ranks_after_two_iterations(gpu_engine, fx):
    pg = gpu_engine
    graph, signal = hc.graph_and_signal(pg, fx, "rmat12")
    tuner = pg.HopTuner()
    ranker = tuner.tune(graph, signal)
    assert tuner.last_tune["route"] == "fused" and tuner.last_values[0].tolist() == [0.0, 0.0] and tuner.last_params[0] == 0.0
    ranks = ranker.rank(graph, signal)
    assert not np.asarray(ranks.np, dtype=np.float64).any()
    assert ranker.convergence.iteration == int(fx["rmat12/cos/krylov/20/iters"]) == 2
    taut = hc.tuner_for(pg, "w300/cos/arnoldi/10")
    assert type(taut.tune(*hc.graph_and_signal(pg, fx, "w300"))) is pg.Tautology


def test_more_than_64_parameters_take_the_primitive_route(gpu_engine, fx):
    pg = gpu_engine
    graph, signal = hc.graph_and_signal(pg, fx, "w300")
    for basis in ("krylov", "arnoldi"):
        tuner = pg.HopTuner(basis=basis, num_parameters=66, measure=pg.AUC if basis == "krylov" else pg.Cos)
        ranks = tuner.rank(graph, signal)
        assert len(tuner.last_params) == 66 and tuner.last_tune["route"] == "primitive", tuner.last_tune
        assert np.all(np.isfinite(np.asarray(ranks.np, dtype=np.float64)))
