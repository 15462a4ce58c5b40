"""The multi-seed loops of include/pgh_batch.h at the C-ABI (no GPU): the HIP library exports them and _lib binds them, pgh.h's
table is unchanged, and on a library without them (the host test double) propagate falls back to the column loop."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"\b(pgh_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def hip_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pygrank_amd", "csrc")])
    return LIB


def test_batch_header_and_table_agree():
    from pygrank_amd import _lib
    assert sorted(_lib.BATCH_SIGNATURES) == _declared("pgh_batch.h")
    assert _lib.OPTIONAL["pgh_batch.h"] is _lib.BATCH_SIGNATURES
    for header, other in [("pgh.h", _lib.SIGNATURES), *_lib.OPTIONAL.items()]:
        if header != "pgh_batch.h":
            assert set(_lib.BATCH_SIGNATURES).isdisjoint(other), header
    defined = re.search(r"#define\s+PGH_BATCH_DECLINED\s+(\d+)", open(os.path.join(ROOT, "include", "pgh_batch.h")).read())
    assert _lib.DECLINED == int(defined.group(1))


def test_hip_library_exports_and_binds_the_batch_loops(hip_lib):
    from pygrank_amd import _lib
    cdll = _lib.load_library(hip_lib)
    bound = _lib.bind_optional(cdll, _lib.BATCH_SIGNATURES)
    for name in _declared("pgh_batch.h"):
        assert hasattr(cdll, name), name
        assert bound[name] is not None and bound[name].argtypes == _lib.BATCH_SIGNATURES[name][1], name


def test_pgh_h_table_is_unchanged():
    from pygrank_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared("pgh.h")


@pytest.mark.parametrize("algo", ["heat", "absorbing", "sarw"])
def test_host_double_falls_back_to_the_column_loop(host_engine, algo):
    from pygrank_amd import _lib
    from pygrank_amd.signals import NodeRanking
    pg = host_engine
    assert _lib.entry("pgh_poly_run_batch") is None
    rng = np.random.default_rng(2)
    n = 60
    A = (rng.random((n, n)) < 0.1).astype(float)
    np.fill_diagonal(A, 0)
    graph = pg.AdjacencyWrapper(__import__("scipy.sparse").sparse.csr_array(A), directed=True)
    F = np.zeros((n, 3))
    F[[1, 5, 9], 0] = 1.0
    F[[2, 40], 2] = 2.0
    make = {"heat": lambda: pg.HeatKernel(5), "absorbing": lambda: pg.AbsorbingWalks(0.85, max_iters=1000),
            "sarw": lambda: pg.SymmetricAbsorbingRandomWalks(max_iters=1000)}[algo]
    ranker = make()
    got = np.asarray(ranker.propagate(graph, pg.to_primitive(F)), dtype=np.float64)
    assert not hasattr(ranker, "last_batches")
    want = np.asarray(NodeRanking.propagate(make(), graph, pg.to_primitive(F)), dtype=np.float64)
    assert np.array_equal(got, want)
    assert np.all(got[:, 1] == 0)
