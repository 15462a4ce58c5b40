"""pg.LFPR on the host test double (no GPU) against the reference's recorded vectors (tests/golden/golden_lfpr.npz).  The double lacks
include/pgh_lfpr.h, so every run here takes the backend-primitive route, whatever `fused` says."""
import numpy as np
import pytest

import lfpr_common as lc


@pytest.mark.parametrize("name", lc.REDISTRIBUTORS)
@pytest.mark.parametrize("key", lc.GRAPHS)
def test_golden_case(host_engine, key, name):
    from pygrank_amd import _lib as L
    assert L.entry("pgh_lfpr_setup") is None and L.entry("pgh_lfpr_close") is None
    algo, _ = lc.Case(host_engine, key).check(name)
    if name == "original":                                  # the shared manager counts the inner PageRank and the outer loop
        assert algo.convergence.iteration > int(lc.fixture()[f"{key}/original/inner"]) > 0
    for leftover in ("d", "dR", "dB", "xR", "xB", "sensitive", "phi"):
        assert not hasattr(algo, leftover)


@pytest.mark.parametrize("name", ["uniform", "original"])
def test_fused_flag_changes_nothing_on_the_double(host_engine, name):
    case = lc.Case(host_engine, "weighted300")
    on, a = case.run(name, fused=True)
    off, b = case.run(name, fused=False)
    assert np.array_equal(a, b) and on.convergence.iteration == off.convergence.iteration


def test_assume_immutability_changes_nothing(host_engine):
    pg = host_engine
    n = lc.graph_of("rmat10_dir")[0].shape[0]
    pre = pg.preprocessor(normalization="none", assume_immutability=True)
    case = lc.Case(pg, "rmat10_dir")                        # one graph object: the remembering preprocessor builds one image
    seen = []
    for seed in (300, 301):                                 # two sensitive groups
        members = np.sort(np.random.default_rng(seed).choice(n, n // 5, replace=False))
        case.sensitive = {int(v): 1.0 for v in members}
        fresh, a = case.run("uniform")
        kept, b = case.run("uniform", preprocessor=pre)
        assert kept.preprocessor is pre and fresh.preprocessor is not pre
        assert np.array_equal(a, b) and fresh.convergence.iteration == kept.convergence.iteration
        seen.append(b)
    assert not np.array_equal(seen[0], seen[1])             # the second group really gave other ranks


def test_refusals(host_engine):
    pg = host_engine
    case = lc.Case(pg, "weighted300")
    signal = pg.to_signal(case.graph, case.seeds)
    with pytest.raises(Exception):
        pg.LFPR(**lc.LFPR).rank(case.graph, signal)        # no sensitive attribute
    with pytest.raises(Exception, match="redistributor"):
        pg.LFPR(redistributor="fair", **lc.LFPR).rank(case.graph, signal, sensitive=pg.to_signal(case.graph, case.sensitive))
    with pytest.raises(Exception):
        pg.LFPR(tolerance=1e-6)                             # a keyword nobody declares


def test_references(host_engine):
    pg = host_engine
    assert pg.LFPR().references() == ["fairness-aware PageRank \\cite{tsioutsiouliklis2021fairness}", "diffusion rate 0.850",
                                      "uniform rank redistribution strategy"]
    assert pg.LFPR(0.9, "original").references()[1:] == ["diffusion rate 0.900", "original rank redistribution strategy"]
    heat = pg.HeatKernel(t=3)
    assert pg.LFPR(redistributor=heat).references()[2] == heat.cite() + " rank redistribution strategy"
    assert pg.LFPR().cite() == "fairness-aware PageRank \\cite{tsioutsiouliklis2021fairness} with diffusion rate 0.850 and " \
                               "uniform rank redistribution strategy"


@pytest.mark.parametrize("name", ["uniform", "original"])
@pytest.mark.parametrize("key", ["weighted300", "rmat10_dir"])
def test_fused_loop_with_numpy_entries(host_engine, key, name):
    """The fused loop's host side on the double's resident iterates, the two entries replaced by numpy evaluations of their header."""
    from pygrank_amd import _lib as L
    cdll = L.lib()
    assert L.entry("pgh_lfpr_close") is None
    calls = dict(pgh_lfpr_setup=0, pgh_lfpr_close=0)

    def counted(fn, which):
        def call(*args):
            calls[which] += 1
            return fn(*args)
        return call
    entries = {which: counted(fn, which) for which, fn in lc.numpy_entries(cdll).items()}
    saved = cdll._pgh_lfpr_entries
    cdll._pgh_lfpr_entries = entries
    try:
        algo, fused = lc.Case(host_engine, key).check(name)
        inner = int(lc.fixture()[f"{key}/original/inner"]) if name == "original" else 0
        steps = algo.convergence.iteration - inner - 1
        assert calls == dict(pgh_lfpr_setup=1, pgh_lfpr_close=steps + 1)       # one close per step, one more for _end
        assert algo.last_loop["steps"] == steps and algo.last_loop["converged"]
        if not lc.graph_of(key)[1] and name == "uniform":
            assert all(abs(total - 1.0) <= 1e-5 for total in algo.last_loop["step_sums"])
    finally:
        cdll._pgh_lfpr_entries = saved
    _, plain = lc.Case(host_engine, key).run(name, fused=False)
    assert lc.rel_linf(fused, plain) <= lc.BAR


def _with_entries(cdll, entries):
    saved = cdll._pgh_lfpr_entries
    cdll._pgh_lfpr_entries = entries
    return saved


@pytest.mark.parametrize("name", ["uniform", "original"])
@pytest.mark.parametrize("at", [1, 3])
def test_close_declining_in_mid_loop_goes_on_in_primitives(host_engine, name, at):
    """The k-th close declines: the iterate before that step goes back to the caller's ids and the run goes on in backend primitives
    with the manager's count intact -- the ranks and the iteration count of the primitive route."""
    from pygrank_amd import _lib as L
    cdll = L.lib()
    assert L.entry("pgh_lfpr_close") is None
    entries = lc.numpy_entries(cdll)
    closes = []

    def close(*args):
        closes.append(len(closes) + 1)
        return L.DECLINED if len(closes) == at else entries["pgh_lfpr_close"](*args)
    saved = _with_entries(cdll, dict(entries, pgh_lfpr_close=close))
    try:
        case = lc.Case(host_engine, "weighted300")
        algo, got = case.check(name)
        assert len(closes) == at                              # nothing fused after the decline, not even _end
    finally:
        cdll._pgh_lfpr_entries = saved
    plain, want = lc.Case(host_engine, "weighted300").run(name, fused=False)
    assert algo.convergence.iteration == plain.convergence.iteration
    assert lc.rel_linf(got, want) <= lc.BAR
    for leftover in ("d", "dR", "dB", "xR", "xB", "sensitive", "phi"):
        assert not hasattr(algo, leftover)


def test_end_declining_falls_back_to_the_primitive_end(host_engine):
    """The close that stands for _end declines (as the loop itself decides for a zero quotient): _end runs in backend primitives."""
    from pygrank_amd import _lib as L
    cdll = L.lib()
    assert L.entry("pgh_lfpr_close") is None
    entries = lc.numpy_entries(cdll)
    declined = []

    def close(y0, x, *rest):
        if y0 == x:                                           # only _end passes the iterate as both operands
            declined.append(1)
            return L.DECLINED
        return entries["pgh_lfpr_close"](y0, x, *rest)
    saved = _with_entries(cdll, dict(entries, pgh_lfpr_close=close))
    try:
        algo, got = lc.Case(host_engine, "weighted300").check("uniform")
        assert declined == [1] and algo.last_loop["converged"]
    finally:
        cdll._pgh_lfpr_entries = saved
    saved = _with_entries(cdll, entries)
    try:
        _, want = lc.Case(host_engine, "weighted300").run("uniform")
    finally:
        cdll._pgh_lfpr_entries = saved
    assert lc.rel_linf(got, want) <= lc.BAR
    assert not hasattr(algo, "xR")
