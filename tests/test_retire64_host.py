"""include/pgh_retire64.h on the host (no GPU): header, _lib table, Makefile and the built library agree, and the one decision of
``f64_retire=`` (filters._batch_call) on the host test double with stand-ins.  tests/test_gpu_retire64.py runs the engine's entries."""
import os
import re
import subprocess

import numpy as np

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")
ENTRIES = ["pgh_absorb_run_batch_f64_retire", "pgh_ppr_run_batch_f64_retire", "pgh_sarw_run_batch_f64_retire", "pgh_spmm_f64_pair"]


def test_header_table_makefile_and_library_agree():
    from pygrank_amd import _lib
    text = open(os.path.join(ROOT, "include", "pgh_retire64.h")).read()
    assert sorted(_lib.RETIRE64_SIGNATURES) == sorted(set(re.findall(r"\b(pgh_[a-z0-9_]+)\s*\(", text))) == ENTRIES
    assert _lib.TABLES["pgh_retire64.h"] is _lib.RETIRE64_SIGNATURES and "pgh_retire64.h" not in _lib.OPTIONAL
    for header, other in [("pgh.h", _lib.SIGNATURES), *[(h, t) for h, t in _lib.TABLES.items() if h != "pgh_retire64.h"]]:
        assert set(ENTRIES).isdisjoint(other), header
    makefile = open(os.path.join(ROOT, "pygrank_amd", "csrc", "Makefile")).read()
    assert re.search(r"^_build/%\.o:.*include/pgh_retire64\.h\b", makefile, re.M)
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pygrank_amd", "csrc")])
    bound = _lib.bind_optional(_lib.load_library(LIB), _lib.RETIRE64_SIGNATURES)
    assert sorted(bound) == ENTRIES and all(bound[name] is not None for name in ENTRIES)


def test_the_decision(host_engine):
    pg = host_engine
    from pygrank_amd import _lib as L
    cdll, log, status = L.lib(), [], [0]
    assert L.entry("pgh_ppr_run_batch_f64") is None and all(L.entry(name) is None for name in ENTRIES)
    saved = cdll._pgh_batch64_entries, cdll._pgh_retire64_entries

    def plain(g, p, out, cfg, scales, results, norms):          # five columns, each converged after three iterations
        log.append("plain")
        for j in range(5):
            results[j].iterations, results[j].converged = 3, 1
        return 0

    def retiring(g, p, out, cfg, scales, results, norms, levels, count, report):
        log.append(("retire", None if levels is None else list(levels[:count]), count))
        if status[0] == 0:
            plain(g, p, out, cfg, scales, results, norms)
            report._obj.num_stages, report._obj.ld[0], report._obj.live[0], report._obj.first_step[0], report._obj.column_steps = 1, 6, 5, 1, 12
        return status[0]
    cdll._pgh_batch64_entries = dict(saved[0], pgh_ppr_run_batch_f64=plain)
    cdll._pgh_retire64_entries = dict(saved[1], pgh_ppr_run_batch_f64_retire=retiring)
    try:
        A, directed, _ = cases.GRAPHS["weighted300"]()
        graph, F = pg.AdjacencyWrapper(A, directed=directed), np.zeros((A.shape[0], 5))
        F[[3, 40, 77, 150, 299], range(5)] = 1.0
        make = lambda **kw: pg.PageRank(0.85, tol=1e-9, max_iters=1000, **kw)      # noqa: E731
        on, off = make(f64_retire=True), make()
        assert np.array_equal(np.asarray(on.propagate(graph, F)), np.asarray(off.propagate(graph, F))) and log == []      # no f64_batch: no effect
        # retire= stays ignored by the f64 batch
        ranker = make(f64_batch=True, retire=True)
        ranker.propagate(graph, F)
        assert log == ["plain"] and all(c["f64"] is True and "stages" not in c for c in ranker.last_batches[0])
        # asked for and present: the retiring entry, its report under "stages"
        ranker = make(f64_batch=True, f64_retire=[8, 2])
        ranker.propagate(graph, F)
        want = dict(ld=[6], live=[5], first_step=[1], column_steps=12)
        assert log[1:] == [("retire", [8, 2], 2), "plain"] and all(c["f64"] is True and c["stages"] == want for c in ranker.last_batches[0])
        # DECLINED: the plain f64 entry
        status[0] = L.DECLINED
        ranker.f64_retire = True
        ranker.propagate(graph, F)
        assert log[3:] == [("retire", None, -1), "plain"] and all("stages" not in c for c in ranker.last_batches[0])
    finally:
        cdll._pgh_batch64_entries, cdll._pgh_retire64_entries = saved
