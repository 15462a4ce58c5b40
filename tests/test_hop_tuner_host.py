"""HopTuner and arnoldi_iteration on the host test double (no GPU) against the reference's recorded behaviour
(tests/golden/golden_hop.npz; the bounds are those of tests/hop_common.py).  The double has neither the Arnoldi passes nor the slab
measures, so every run takes the primitive route here -- the reference's loop, one backend primitive at a time."""
import numpy as np
import pytest

import hop_common as hc


@pytest.fixture(scope="module")
def fx():
    return hc.fixture()


@pytest.mark.parametrize("variant", [name for name in hc.VARIANTS if name not in hc.OFFSET_VARIANTS])
def test_variant_follows_the_reference(host_engine, fx, variant):
    tuner = hc.check_variant(host_engine, fx, variant, "primitive")
    assert tuner.last_tune["sweep"] in ("primitive", "arnoldi:primitive") and set(tuner.last_tune["scoring"]) == {"columns"}


@pytest.mark.parametrize("variant", hc.OFFSET_VARIANTS)
def test_offset_search_reaches_the_reference_loss(host_engine, fx, variant):
    hc.check_offset(host_engine, fx, variant, "primitive")


@pytest.mark.parametrize("variant", hc.STAGE_VARIANTS)
def test_autoregression_stage_on_the_reference_values(fx, variant):
    import pygrank_amd as pg
    hc.check_stage(pg, fx, variant)


def test_stage_without_autoregression_is_the_mean_of_the_halves():
    import pygrank_amd as pg
    values = np.random.default_rng(3).random((12, 2))
    assert np.allclose(pg.hop_parameters(values, 10), values.mean(axis=1)[:10], rtol=1e-13, atol=0)


@pytest.mark.parametrize("key", sorted(hc.GRAPHS))
@pytest.mark.parametrize("k", hc.ARNOLDI_DIMS)
def test_arnoldi_iteration_follows_the_reference(host_engine, fx, key, k):
    for fused in (False, True):                  # (fused=True falls back: the double lacks the entries)
        hc.check_arnoldi(host_engine, fx, key, k, fused, "primitive")


def test_default_tuner_returns_zero_ranks_after_two_iterations(host_engine, fx):
    pg = host_engine
    graph, signal = hc.graph_and_signal(pg, fx, "rmat12")
    tuner = pg.HopTuner()
    assert tuner.measure is pg.Cos and tuner.basis == "krylov" and tuner.num_parameters == 20 and tuner.fused is True
    ranker = tuner.tune(graph, signal)
    assert isinstance(ranker, pg.GenericGraphFilter) and isinstance(ranker.optimization_dict, pg.SelfClearDict)
    assert tuner.last_values[0].tolist() == [0.0, 0.0] and tuner.last_params[0] == 0.0
    assert np.allclose(tuner.last_params, fx["rmat12/cos/krylov/20/params"], rtol=0, atol=hc.FACTOR * float(fx["rmat12/cos/krylov/20/params_dev"]))
    ranks = ranker.rank(graph, signal)
    assert not np.asarray(ranks.np, dtype=np.float64).any()
    assert ranker.convergence.iteration == int(fx["rmat12/cos/krylov/20/iters"]) == 2
    assert tuner.references() == ["HopTuner"]


def test_arnoldi_basis_returns_a_tautology(host_engine, fx):
    pg = host_engine
    graph, signal = hc.graph_and_signal(pg, fx, "w300")
    tuner = hc.tuner_for(pg, "w300/cos/arnoldi/10")
    ranker = tuner.tune(graph, signal)
    assert type(ranker) is pg.Tautology


def test_more_than_64_parameters_and_bad_arguments(host_engine, fx):
    pg = host_engine
    graph, signal = hc.graph_and_signal(pg, fx, "w300")
    for basis in ("krylov", "arnoldi"):
        tuner = pg.HopTuner(basis=basis, num_parameters=66, measure=pg.AUC if basis == "krylov" else pg.Cos)
        ranks = tuner.rank(graph, signal)
        assert len(tuner.last_params) == 66 and tuner.last_tune["route"] == "primitive"
        assert np.all(np.isfinite(np.asarray(ranks.np, dtype=np.float64)))
    with pytest.raises(Exception, match="tuning_backend"):
        pg.HopTuner(tuning_backend="numpy")
    with pytest.raises(Exception, match="No usage of argument"):
        pg.HopTuner(ranker_generator=lambda params: pg.GenericGraphFilter(params), tol=1e-9)
    assert pg.HopTuner(pre_diffuse=pg.PageRank()).pre_diffuse is not None
