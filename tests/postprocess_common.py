"""Shared by the postprocessor propagate tests (host double and GPU): the postprocessors with a slab form, the chain, the feature slabs
and the one comparison both suites make -- ``post.propagate(graph, F)`` against ``post.transform`` of every column of the inner
ranker's own ``propagate`` outcome."""
import numpy as np

import oversampling_common as oc

GRAPHS = ["weighted300", "rmat10_dir"]
WIDTHS = [3, 70]                     # fewer columns than a quad walk's lanes meet at once; more than one 64-column chunk
# The bound where the slab form and the primitive route round differently (Normalize, Transformer): the primitive route's x / s is a
# lazy product with a reciprocal, two f32 roundings; the slab form rounds the divisor and the quotient, two more.
REL = 4.0 * 2.0 ** -24
EXACT = {"Top": True, "TopShare": True, "Threshold": True, "ThresholdGap": True, "Ordinals": True, "Sweep": True, "LinearSweep": True,
         "NormalizeMax": False, "NormalizeSum": False, "NormalizeL2": False, "NormalizeRange": False, "Transformer": False, "Chain": True}


def stages(pg, name, n):
    """The postprocessing steps of case `name`, innermost first, as callables ranker -> postprocessor."""
    one = {
        "Top": lambda r: pg.Top(r, 5),
        "TopShare": lambda r: pg.Top(r, 0.1),
        "Threshold": lambda r: pg.Threshold(r, 0.5 / n, inclusive=True),
        "ThresholdGap": lambda r: pg.Threshold(r, "gap"),
        "Ordinals": lambda r: pg.Ordinals(r),
        "Sweep": lambda r: pg.Sweep(r),
        "LinearSweep": lambda r: pg.LinearSweep(r),
        "NormalizeMax": lambda r: pg.Normalize(r),
        "NormalizeSum": lambda r: pg.Normalize(r, "sum"),
        "NormalizeL2": lambda r: pg.Normalize("L2", r),
        "NormalizeRange": lambda r: pg.Normalize(r, "range"),
        "Transformer": lambda r: pg.Transformer(r),
    }
    if name == "Chain":                 # PageRank >> Sweep >> Normalize("sum") >> Top(5)
        return [one["Sweep"], one["NormalizeSum"], one["Top"]]
    return [one[name]]


def build(pg, name, ranker, n):
    """(the outermost postprocessor, every step innermost first) around `ranker`."""
    steps, post = [], ranker
    for make in stages(pg, name, n):
        post = make(post)
        steps.append(post)
    return post, steps


def features(n, width, seed=7):
    """[n, width] zeros and ones, about 2% ones, at least two per column."""
    rng = np.random.default_rng(seed + 1000 * width + n)
    F = (rng.random((n, width)) < 0.02).astype(np.float64)
    for j in range(width):
        F[rng.choice(n, 2, replace=False), j] = 1.0
    return F


def within(got, want, exact):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if exact:
        return np.array_equal(got, want)
    return bool(np.all(np.abs(got - want) <= REL * np.abs(want)))


def worst(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.where(want != 0, np.abs(want), 1.0)
    return float(np.max(np.abs(got - want) / scale)) if got.size else 0.0


def check_propagate(pg, key, width, name, route, **switches):
    """Runs case `name` on graph `key` with `width` feature columns; returns (post, steps, ranker, got) after the shared assertions."""
    case = oc.Case(pg, key)
    F = features(case.n, width)
    ranker = case.ranker()
    post, steps = build(pg, name, ranker, case.n)
    for step in steps:
        for switch, value in switches.items():
            setattr(step, switch, value)
    got = post.propagate(case.graph, F)
    assert isinstance(got, pg.DeviceMatrix) and got.shape == (case.n, width)
    # the inner filter ran ONE propagate: one multi-seed loop per 64 columns
    assert [len(batch) for batch in ranker.last_batches] == [min(64, width - first) for first in range(0, width, 64)]
    for step in steps:
        assert step.last_propagate["route"] == route, (type(step).__name__, step.last_propagate)
    # the reference: the inner ranker's own propagate outcome, every column through each step's transform
    plain = case.ranker()
    _, fresh = build(pg, name, plain, case.n)
    inner = plain.propagate(case.graph, F)
    got = got.numpy()
    want = np.empty_like(got)
    for j, column in enumerate(inner.columns()):
        signal = pg.to_signal(case.graph, column)
        for step in fresh:
            signal = step.transform(signal)
        want[:, j] = np.asarray(signal.np, dtype=np.float64)
    print(f"{key} B={width} {name} {switches}: worst relative difference {worst(got, want):.3e}")
    for j in range(width):
        assert within(got[:, j], want[:, j], EXACT[name]), (key, width, name, j, worst(got[:, j], want[:, j]))
    return post, steps, ranker, got
