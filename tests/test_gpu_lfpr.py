"""pg.LFPR on the GPU against the reference's recorded vectors (tests/golden/golden_lfpr.npz): every case within the project's 1e-6
rel-Linf bar (the fixture generator's f32 evaluation of the fused route stays below 4.2e-7) with the reference's
iteration count, on the fused route -- engine calls are counted at the ctypes boundary -- and on the backend-primitive route."""
import collections

import numpy as np
import pytest

import lfpr_common as lc

pytestmark = pytest.mark.gpu

WATCHED = ("pgh_resident_step", "pgh_resident_gather", "pgh_resident_in", "pgh_resident_out", "pgh_spmv", "pgh_graph_from_adjacency",
           "pgh_graph_from_adjacency_ex", "pgh_graph_from_csr", "pgh_graph_from_factored_csr", "pgh_graph_resident_len")


class Counted:
    """Counts the watched entries of include/pgh.h and both entries of include/pgh_lfpr.h while it is open."""

    def __enter__(self):
        from pygrank_amd import _lib as L
        self.lib, self.counts = L.lib(), collections.Counter()
        assert L.entry("pgh_lfpr_setup") is not None and L.entry("pgh_lfpr_close") is not None
        self.originals = {name: getattr(self.lib, name) for name in WATCHED}
        self.entries = self.lib._pgh_lfpr_entries
        for name, fn in self.originals.items():
            setattr(self.lib, name, self._counted(name, fn))
        self.lib._pgh_lfpr_entries = {name: self._counted(name, fn) for name, fn in self.entries.items()}
        return self.counts

    def _counted(self, name, fn):
        def call(*args):
            self.counts[name] += 1
            if name == "pgh_resident_step":
                self.counts[f"step_mode{int(args[1])}"] += 1
            return fn(*args)
        return call

    def __exit__(self, *exc):
        for name, fn in self.originals.items():
            setattr(self.lib, name, fn)
        self.lib._pgh_lfpr_entries = self.entries


@pytest.fixture(scope="module")
def fused_runs(gpu_engine):
    """Every golden case once on the fused route: {(graph, redistributor): (filter, ranks, engine calls)}, shared and left unchanged."""
    runs = {}
    for key in lc.GRAPHS:
        case = lc.Case(gpu_engine, key)
        for name in lc.REDISTRIBUTORS:
            with Counted() as counts:
                algo, got = case.check(name)
            runs[key, name] = (algo, got, dict(counts))
    return runs


@pytest.mark.parametrize("name", lc.REDISTRIBUTORS)
@pytest.mark.parametrize("key", lc.GRAPHS)
def test_golden_case_on_the_fused_route(gpu_engine, fused_runs, key, name):
    algo, _, counts = fused_runs[key, name]              # (the bars themselves were asserted by Case.check)
    inner = int(lc.fixture()[f"{key}/original/inner"]) if name == "original" else 0
    steps = algo.convergence.iteration - inner - 1
    assert steps >= 5
    assert counts.get("pgh_lfpr_setup") == 1 and counts.get("pgh_lfpr_close") == steps + 1, counts     # one per step, one more for _end
    assert counts.get("step_mode1") == steps and algo.last_loop["steps"] == steps and algo.last_loop["converged"], counts
    assert counts.get("pgh_resident_gather", 0) in (0, steps), counts
    assert counts.get("pgh_spmv", 0) == 0, counts
    # the raw graph, and the col-normalised one of the inner PageRank; a ranker as the redistributor builds its own
    built = sum(counts.get(entry, 0) for entry in WATCHED if entry.startswith("pgh_graph_from"))
    assert built == {"uniform": 1, "original": 2, "heat": 2}[name], counts
    assert counts.get("pgh_graph_from_adjacency", 0) == built, counts
    # out of the id space: outR, outB, and the result -- once, at the end
    assert counts.get("pgh_resident_out", 0) <= 3 + (name == "heat"), counts


@pytest.mark.parametrize("key", [key for key in lc.GRAPHS if not lc.graph_of(key)[1]])
def test_every_step_conserves_mass_on_undirected_graphs(gpu_engine, fused_runs, key):
    algo = fused_runs[key, "uniform"][0]
    sums = algo.last_loop["step_sums"]
    assert len(sums) == algo.last_loop["steps"]
    worst = max(abs(total - 1.0) for total in sums)      # sum y = alpha * sum x + (1 - alpha) with sum x = 1 after the quotient
    print(key, "largest |sum y - 1|", worst)
    assert worst <= 1e-5


@pytest.mark.parametrize("name", lc.REDISTRIBUTORS)
@pytest.mark.parametrize("key", lc.GRAPHS)
def test_primitive_route_agrees(gpu_engine, fused_runs, key, name):
    fused_algo, fused, _ = fused_runs[key, name]
    with Counted() as counts:
        algo, got = lc.Case(gpu_engine, key).check(name, fused=False)
    assert counts.get("pgh_lfpr_setup", 0) == 0 and counts.get("pgh_lfpr_close", 0) == 0, counts
    assert algo.convergence.iteration == fused_algo.convergence.iteration
    assert lc.rel_linf(got, fused) <= lc.BAR


def test_row_major_image_takes_the_primitive_route(gpu_engine, fused_runs, monkeypatch):
    monkeypatch.setenv("PGH_FORMAT", "csr")              # read when the graph is built, inside rank()
    with Counted() as counts:
        algo, got = lc.Case(gpu_engine, "rmat10_dir").check("uniform")
    assert counts.get("pgh_lfpr_close", 0) == 0 and counts.get("step_mode1", 0) == 0 and counts["pgh_spmv"] >= algo.convergence.iteration, counts
    assert getattr(algo, "last_loop", None) is None
    assert lc.rel_linf(got, fused_runs["rmat10_dir", "uniform"][1]) <= lc.BAR


def test_remembered_image_serves_two_sensitive_groups(gpu_engine):
    pg = gpu_engine
    n = lc.graph_of("rmat12_sym")[0].shape[0]
    pre = pg.preprocessor(normalization="none", assume_immutability=True)
    case = lc.Case(pg, "rmat12_sym")
    with Counted() as counts:
        for seed in (300, 301):
            members = np.sort(np.random.default_rng(seed).choice(n, n // 5, replace=False))
            case.sensitive = {int(v): 1.0 for v in members}
            _, kept = case.run("uniform", preprocessor=pre)
            _, fresh = case.run("uniform")
            assert np.array_equal(kept, fresh)
    assert counts["pgh_graph_from_adjacency"] == 3, counts     # one remembered image, one per rank() without the promise


def test_tolerance_below_fp32_eps(gpu_engine):
    """tol=1e-9 on f32 iterates: the loop is clamped at fp32 eps and stops early.  Bar: rel-Linf against the
    reference's tol=1e-9 vector at most twice what the fixture generator's f32 evaluation of this route recorded for the case (8.5e-5)."""
    fx = lc.fixture()
    key, name = lc.TIGHT
    algo, got = lc.Case(gpu_engine, key).run(name, tol=1e-9)
    recorded = float(fx[f"{key}/{name}/f32_rel_linf_tol1e-9"])
    worst = lc.rel_linf(got, fx[f"{key}/{name}/ranks_tol1e-9"])
    print(key, name, "tol=1e-9: rel-Linf", worst, "recorded f32 evaluation", recorded, "iterations", algo.convergence.iteration)
    assert worst <= 2 * recorded
