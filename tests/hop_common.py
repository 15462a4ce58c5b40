"""Shared by the tests of HopTuner and arnoldi_iteration (host double and GPU) and by tests/golden/make_golden_hop.py: the variants, the
fixture and the checks.

Bounds.  A recorded quantity is held to FACTOR (= 8) times the deviation the fixture records for it -- the generator's own f32-storage
evaluation of the engine's route against the reference's f64 value (the convention of tests/test_krylov_host.py): the engine only adds
other summation orders on top of the same storage rounding.  The primitive Arnoldi loop rounds its coefficients to f32 and is less
accurate than the fused step; the fixture records a deviation for either route and a run is held to that of the route it took.
An AUC-scored hop is held to its flip budget instead: the share of (positive, negative) pairs whose reference scores lie within
4 * hop * eps32 * max |score| of each other, which a different rounding may order the other way.  Such a change moves what is derived
from the hop values, so for AUC variants without autoregression and offset the bounds of params and ranks add its first-order
propagation, with b_i the mean over the halves of the hop's budget (pairs of two exact zeros left out: a node no walk reaches is an
exact zero in every evaluation), m the mean of the reference's raw weights (the means of the hop values: AUCs, so non-negative) and bm
the mean of b:
    |d params_i| <= (b_i + params_i bm) / (m - bm)                 params = raw / mean |raw|
    |d ranks|    <= sum_i |d params_i| max |power_i|                ("arnoldi": max |Q[:, i]| / K, since _run divides by sum |params| = K)
With autoregression the weights come out of an Adam loop whose sensitivity has no such bound: there the stage itself is checked on the
reference's values (check_stage) and the run is held to hop_parameters of its OWN values.  With an offset the chosen offset may differ
(the reference's first two steps tie to 8 digits), so only the hop values and the loss reached are compared."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 8.0
ARNOLDI_DIMS = (6, 10, 20)

# name -> (graph, measure, basis, num_parameters, autoregression, tunable_offset)
VARIANTS = {
    "rmat12/cos/krylov/20": ("rmat12", "Cos", "krylov", 20, 0, None),
    "rmat12/cos/krylov/10": ("rmat12", "Cos", "krylov", 10, 0, None),
    "rmat12/auc/krylov/20": ("rmat12", "AUC", "krylov", 20, 0, None),
    "rmat12/auc/krylov/10": ("rmat12", "AUC", "krylov", 10, 0, None),
    "rmat12/cos/arnoldi/10": ("rmat12", "Cos", "arnoldi", 10, 0, None),
    "rmat12/cos/arnoldi/20": ("rmat12", "Cos", "arnoldi", 20, 0, None),
    "rmat12/auc/arnoldi/10": ("rmat12", "AUC", "arnoldi", 10, 0, None),
    "rmat12/cos/krylov/8+3": ("rmat12", "Cos", "krylov", 8, 3, None),
    "rmat12/auc/krylov/8+3": ("rmat12", "AUC", "krylov", 8, 3, None),
    "rmat12/auc/krylov/10/offset": ("rmat12", "AUC", "krylov", 10, 0, "AUC"),
    "rmat12/auc/arnoldi/10/offset": ("rmat12", "AUC", "arnoldi", 10, 0, "AUC"),
    "w300/cos/krylov/10": ("w300", "Cos", "krylov", 10, 0, None),
    "w300/cos/arnoldi/10": ("w300", "Cos", "arnoldi", 10, 0, None),
    "w300/cos/krylov/8+3": ("w300", "Cos", "krylov", 8, 3, None),
}
GRAPHS = {"rmat12": "rmat12_sym", "w300": "weighted300"}
OFFSET_VARIANTS = [name for name, spec in VARIANTS.items() if spec[5] is not None]
STAGE_VARIANTS = [name for name, spec in VARIANTS.items() if spec[4] != 0]

_cache = {}


def fixture():
    if "fx" not in _cache:
        with np.load(os.path.join(ROOT, "tests", "golden", "golden_hop.npz")) as data:
            _cache["fx"] = {key: data[key] for key in data.files}
    return _cache["fx"]


def graph_and_signal(pg, fx, key):
    """(graph, personalization) of the fixture's graph `key`; the host matrices are built once."""
    import cases
    if key not in _cache:
        _cache[key] = cases.GRAPHS[GRAPHS[key]]()[:2]
    A, directed = _cache[key]
    graph = pg.AdjacencyWrapper(A, directed=directed)
    signal = pg.to_signal(graph, {int(v): float(x) for v, x in zip(fx[key + "/seeds"], fx[key + "/seed_values"])})
    return graph, signal


def tuner_for(pg, variant, **more):
    _, measure, basis, num_parameters, autoregression, offset = VARIANTS[variant]
    return pg.HopTuner(measure=getattr(pg, measure), basis=basis, num_parameters=num_parameters, autoregression=autoregression,
                       tunable_offset=None if offset is None else getattr(pg, offset), **more)


def normalised(params):
    """hop_tuner.py:161-163."""
    params = np.array(params, dtype=np.float64)
    return params / np.mean(np.abs(params)) if np.sum(np.abs(params)) != 0 else params


def check_variant(pg, fx, variant, route, **more):
    """A full run of `variant` against the fixture; returns the tuner."""
    key, measure, basis, num_parameters, autoregression, offset = VARIANTS[variant]
    graph, signal = graph_and_signal(pg, fx, key)
    tuner = tuner_for(pg, variant, **more)
    ranks = tuner.rank(graph, signal)
    assert isinstance(ranks, pg.GraphSignal)
    ranks = np.asarray(ranks.np, dtype=np.float64)
    hops = num_parameters + autoregression
    values, params = tuner.last_values, np.array(tuner.last_params)
    want_values, want_params, want_ranks = fx[variant + "/values"], fx[variant + "/params"], fx[variant + "/ranks"]
    assert values.shape == (hops, 2) and params.shape == (num_parameters,)
    assert tuner.last_tune["route"] == route, tuner.last_tune
    tail = "_dev_primitive" if basis != "krylov" and route == "primitive" else "_dev"      # (the primitive Arnoldi loop: its own deviation)
    off = np.abs(values - want_values)
    print(variant, tuner.last_tune, "values off by", float(off.max()), "recorded", float(fx[variant + "/values" + tail]))
    dparams = None
    if measure == "AUC":
        assert np.all(off <= fx[variant + "/flip"] + 1e-12), (variant, off.tolist(), fx[variant + "/flip"].tolist())
        if autoregression == 0 and offset is None:
            raw = want_values.mean(axis=1)[:num_parameters]
            b = fx[variant + "/flip_strict"].mean(axis=1)[:num_parameters]
            m, bm = float(raw.mean()), float(b.mean())
            assert np.all(raw >= 0) and m > bm
            dparams = (b + np.abs(want_params) * bm) / (m - bm)
    else:
        assert float(off.max()) <= FACTOR * float(fx[variant + "/values" + tail]), (variant, float(off.max()))
        dparams = np.zeros(num_parameters)
    if offset is None:                       # (what the tuner makes of its OWN values, always)
        own = normalised(pg.hop_parameters(values, num_parameters, autoregression))
        assert np.allclose(params, own, rtol=1e-12, atol=1e-300), (variant, params.tolist(), own.tolist())
    scale = float(np.abs(want_ranks).max())
    if dparams is not None and (measure != "AUC" or autoregression == 0):
        poff = np.abs(params - want_params)
        print("    params off by", float(poff.max()), "recorded", float(fx[variant + "/params" + tail]), "propagated", float(dparams.max()))
        assert np.all(poff <= FACTOR * float(fx[variant + "/params" + tail]) + dparams), (variant, poff.tolist())
        if basis == "krylov":
            moved = float(np.sum(dparams * fx[key + "/power_linf"][:num_parameters]))
        else:
            moved = float(np.sum(dparams / num_parameters * np.abs(fx[key + "/arnoldi_Q"][:, :num_parameters]).max(axis=0)))
        if scale == 0:
            assert not ranks.any(), variant                      # the default-Cos outcome: a first weight of 0 ends the filter at once
        else:
            roff = float(np.abs(ranks - want_ranks).max() / scale)
            print("    ranks off by", roff, "recorded", float(fx[variant + "/ranks" + tail]), "propagated", moved / scale)
            assert roff <= FACTOR * float(fx[variant + "/ranks" + tail]) + moved / scale, (variant, roff)
    return tuner


def check_arnoldi(pg, fx, key, k, fused, route):
    """pg.arnoldi_iteration at k columns against the reference's Q and h."""
    from pygrank_amd import krylov
    graph, signal = graph_and_signal(pg, fx, key)
    M = pg.GenericGraphFilter([1.0]).preprocessor(graph)
    Q, h, took = krylov.arnoldi_run(M, signal.np, k, fused)
    assert took == route, (key, k, took)
    Q2, h2 = pg.arnoldi_iteration(M, signal.np, k, fused=fused)
    Q, h = np.asarray(Q.numpy(), dtype=np.float64), np.array(h, dtype=np.float64)
    assert np.array_equal(Q, Q2.numpy()) and np.array_equal(h, np.array(h2, dtype=np.float64))
    assert Q.shape == (len(signal.np), k) and h.shape == (k + 1, k)
    want_Q, want_h = fx[key + "/arnoldi_Q"][:, :k], fx[key + "/arnoldi_h"][:k, :k - 1]
    q_dev = float(fx[f"{key}/arnoldi_Q_dev{'' if route == 'fused' else '_primitive'}/{k}"])
    h_dev = float(fx[f"{key}/arnoldi_h_dev{'' if route == 'fused' else '_primitive'}/{k}"])
    q_off = float(np.abs(Q - want_Q).max() / np.abs(want_Q).max())
    h_off = float(np.abs(h[:k, :k - 1] - want_h).max() / np.abs(want_h).max())
    print(key, k, took, "Q off by", q_off, "recorded", q_dev, "h off by", h_off, "recorded", h_dev)
    assert q_off <= FACTOR * q_dev, (key, k, q_off)
    assert h_off <= FACTOR * h_dev, (key, k, h_off)
    assert not h[:, k - 1].any() and not np.tril(h[:k + 1, :k], -2).any()      # the last column stays empty; upper Hessenberg


def check_stage(pg, fx, variant):
    """The autoregression stage on the reference's recorded values: the same f64 arithmetic, so the reference's parameters."""
    _, _, _, num_parameters, autoregression, _ = VARIANTS[variant]
    got = normalised(pg.hop_parameters(fx[variant + "/values"], num_parameters, autoregression))
    want = fx[variant + "/params"]
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), (variant, got.tolist(), want.tolist())


def check_offset(pg, fx, variant, route, **more):
    """The offset search: the reference's candidates through loss() and loss.many(), and the loss the port's own search reaches."""
    from pygrank_amd import autotune, krylov
    key, _, basis, num_parameters, autoregression, offset = VARIANTS[variant]
    tuner = check_variant(pg, fx, variant, route, **more)
    graph, signal = graph_and_signal(pg, fx, key)
    training, validation = pg.split(pg.to_signal(signal, signal.np), 0.8)
    base = None
    if basis != "krylov":
        M = tuner.ranker_generator([None] * num_parameters).preprocessor(graph)
        base = krylov.arnoldi_run(M, pg.split(training, 0.5)[0].np, num_parameters, tuner.fused)[0]

    def loss_from(parameters):
        return autotune._HopOffsetLoss(tuner, getattr(pg, offset)(validation, training), training, validation, parameters, base, (), {})
    loss = loss_from(fx[variant + "/pre_offset"])
    assert callable(getattr(loss, "many", None)) == bool(tuner.fused)
    for offsets, wants, budgets in zip(fx[variant + "/offsets"], fx[variant + "/losses"], fx[variant + "/loss_flip"]):
        candidates = [[float(v)] for v in offsets]
        routes = [[loss(c) for c in candidates]] + ([list(loss.many(candidates))] if tuner.fused else [])
        for got in routes:
            for mine, want, budget in zip(got, wants, budgets):
                assert abs(mine - want) <= budget + 1e-12, (variant, mine, want, budget)
    own = loss_from(tuner.last_pre_offset)([tuner.last_offset])
    print("    offset", tuner.last_offset, "reference", float(fx[variant + "/offset"]), "loss", own, "reference's best", float(fx[variant + "/best_loss"]))
    assert 0 <= tuner.last_offset <= 1
    assert own <= float(fx[variant + "/best_loss"]) + float(fx[variant + "/loss_flip"].max()) + 1e-12, (variant, own)
    return tuner
