"""include/pgh_retire.h on the host (no GPU): its table in _lib matches the header and the Makefile, the HIP library exports the four
entries, and the Python side of ``retire=`` -- which entry propagate calls, with which levels, where the report ends up, and the plain
call where the library lacks the entry or the entry DECLINED -- on the host test double, which has none of them, with stand-ins in
``_pgh_retire_entries``.  tests/test_gpu_retire.py runs the engine's own entries."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")
ENTRIES = ["pgh_absorb_run_batch_retire", "pgh_ppr_run_batch_mixed_retire", "pgh_ppr_run_batch_retire", "pgh_sarw_run_batch_retire"]
RULE = dict(tol=1e-6, max_iters=1000)


def test_header_table_and_makefile_agree():
    from pygrank_amd import _lib
    text = open(os.path.join(ROOT, "include", "pgh_retire.h")).read()
    assert sorted(_lib.RETIRE_SIGNATURES) == sorted(set(re.findall(r"\b(pgh_[a-z0-9_]+)\s*\(", text))) == ENTRIES
    assert _lib.TABLES["pgh_retire.h"] is _lib.RETIRE_SIGNATURES and "pgh_retire.h" not in _lib.OPTIONAL
    for header, other in [("pgh.h", _lib.SIGNATURES), *[(h, t) for h, t in _lib.TABLES.items() if h != "pgh_retire.h"]]:
        assert set(ENTRIES).isdisjoint(other), header

    def defined(name):
        return int(re.search(r"#define\s+" + name + r"\s+(\d+)", text).group(1))
    assert _lib.DECLINED == defined("PGH_RETIRE_DECLINED") == 2
    assert _lib.RETIRE_MAX_STAGES == defined("PGH_RETIRE_MAX_STAGES") == 8 and _lib.RETIRE_NARROWED == defined("PGH_RETIRE_NARROWED") == 32
    # two int32, three int32[8], one int64
    assert C.sizeof(_lib.RetireReport) == 8 + 3 * 4 * 8 + 8 and _lib.RetireReport.column_steps.offset == 104
    # each entry: its plain sibling's arguments, then levels, num_levels, report
    plain = dict(pgh_ppr_run_batch_retire=_lib.SIGNATURES["pgh_ppr_run_batch"], pgh_ppr_run_batch_mixed_retire=_lib.MIXED_SIGNATURES[
        "pgh_ppr_run_batch_mixed"], pgh_absorb_run_batch_retire=_lib.BATCH_SIGNATURES["pgh_absorb_run_batch"],
        pgh_sarw_run_batch_retire=_lib.BATCH_SIGNATURES["pgh_sarw_run_batch"])
    for name, (restype, argtypes) in _lib.RETIRE_SIGNATURES.items():
        assert restype is C.c_int and argtypes == plain[name][1] + [C.POINTER(C.c_int32), C.c_int32, C.POINTER(_lib.RetireReport)], name
    makefile = open(os.path.join(ROOT, "pygrank_amd", "csrc", "Makefile")).read()
    assert re.search(r"^_build/%\.o:.*include/pgh_retire\.h\b", makefile, re.M)


def test_hip_library_exports_and_binds_the_entries():
    from pygrank_amd import _lib
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pygrank_amd", "csrc")])
    cdll = _lib.load_library(LIB)
    bound = _lib.bind_optional(cdll, _lib.RETIRE_SIGNATURES)
    assert sorted(bound) == ENTRIES and all(bound[name] is not None for name in ENTRIES)


def test_levels_and_switch():
    from pygrank_amd import _lib
    assert [_lib.retire_on(v) for v in (False, None, True, [], [8, 4], (16,), 0)] == [False, False, True, True, True, True, False]
    assert _lib.retire_levels(True) == (None, -1)
    levels, count = _lib.retire_levels([48, 20, 12, 4])
    assert count == 4 and list(levels) == [48, 20, 12, 4]
    assert _lib.retire_levels([])[1] == 0


def _features(n, width):
    rng = np.random.default_rng(width)
    F = np.zeros((n, width))
    for j in range(width):
        F[rng.choice(n, 1 + j % 7, replace=False), j] = rng.uniform(0.5, 1.5, 1 + j % 7)
    F[:, width // 2] = 0.0                                          # a zero column stays zero and is not counted
    return F


def _graph(pg, key="weighted300"):
    A, directed, _ = cases.GRAPHS[key]()
    return pg.AdjacencyWrapper(A, directed=directed), A.shape[0]


def test_host_double_has_no_entry_and_takes_the_plain_call(host_engine):
    pg = host_engine
    from pygrank_amd import _lib
    assert all(_lib.entry(name) is None for name in ENTRIES)
    graph, n = _graph(pg)
    F = _features(n, 9)
    on, off = pg.PageRank(0.85, retire=True, **RULE), pg.PageRank(0.85, **RULE)
    assert on.retire is True and off.retire is False
    got, want = on.propagate(graph, F).numpy(), off.propagate(graph, F).numpy()
    assert np.array_equal(got, want)
    strip = lambda batches: [[{k: v for k, v in column.items() if k != "loop_ms"} for column in batch] for batch in batches]   # noqa: E731
    assert strip(on.last_batches) == strip(off.last_batches)
    assert all("stages" not in column for batch in on.last_batches for column in batch)


@pytest.fixture()
def stand_in(host_engine):
    """The host double with a stand-in for pgh_ppr_run_batch_retire: the plain entry on the same arguments, bit 5 on every column's
    flags and a report made from the call's own widths.  Yields (pg, log, behaviour): log gains (width, levels, num_levels) per call,
    behaviour["status"] (None: run) is what the stand-in returns instead of running."""
    from pygrank_amd import _lib as L
    cdll, log, behaviour = L.lib(), [], dict(status=None)
    assert L.entry("pgh_ppr_run_batch_retire") is None
    saved = cdll._pgh_retire_entries

    def ppr(g, p, ranks, cfg, scales, results, levels, count, report):
        n, b = C.c_int64(), C.c_int32()
        assert cdll.pgh_mat_shape(p, C.byref(n), C.byref(b)) == 0
        log.append((b.value, None if levels is None else list(levels[:count]), count))
        if behaviour["status"] is not None:
            return behaviour["status"]
        status = cdll.pgh_ppr_run_batch(g, p, ranks, cfg, scales, results)
        for j in range(b.value):
            results[j].flags |= L.RETIRE_NARROWED
        rep = report._obj
        rep.num_stages = 2
        rep.ld[0], rep.live[0], rep.first_step[0] = (b.value + 3) & ~3, b.value, 1
        rep.ld[1], rep.live[1], rep.first_step[1] = 4, 1, 100 + len(log)
        rep.column_steps = 1000 * len(log) + b.value
        return status
    cdll._pgh_retire_entries = dict(saved, pgh_ppr_run_batch_retire=ppr)
    try:
        yield host_engine, log, behaviour
    finally:
        cdll._pgh_retire_entries = saved


def test_propagate_calls_the_entry_and_keeps_its_report(stand_in):
    pg, log, _ = stand_in
    graph, n = _graph(pg)
    F = _features(n, 81)                                            # two chunks: 64 and 17 columns
    on, off = pg.PageRank(0.85, retire=True, **RULE), pg.PageRank(0.85, **RULE)
    got, want = on.propagate(graph, F).numpy(), off.propagate(graph, F).numpy()
    assert log == [(64, None, -1), (17, None, -1)]
    assert np.array_equal(got, want) and not got[:, 40].any()
    assert [len(batch) for batch in on.last_batches] == [64, 17]
    for c, (batch, plain) in enumerate(zip(on.last_batches, off.last_batches)):
        width = len(batch)
        want_stages = dict(ld=[(width + 3) & ~3, 4], live=[width, 1], first_step=[1, 101 + c], column_steps=1000 * (c + 1) + width)
        for column, other in zip(batch, plain):                     # the caller's column order, chunk by chunk
            assert column["stages"] == want_stages and "stages" not in other
            assert column["iterations"] == other["iterations"] and column["converged"] == other["converged"]
            assert column["flags"] == other["flags"] | 32
    # a list of levels travels as it is; the attribute may be set after construction
    del log[:]
    off.retire = [48, 20, 12, 4]
    off.propagate(graph, F[:, :5])
    assert log == [(5, [48, 20, 12, 4], 4)] and "stages" in off.last_batches[0][0]
    del log[:]
    off.retire = []
    off.propagate(graph, F[:, :5])
    assert log == [(5, [], 0)]
    # graph_dropout takes the plain loop
    del log[:]
    dropped = pg.PageRank(0.85, retire=True, error_type="iters", max_iters=10)      # (a fresh mask per step: no tolerance is met)
    dropped.propagate(graph, F[:, :5], graph_dropout=0.25)
    assert log == [] and all("stages" not in column for column in dropped.last_batches[0])


def test_wrappers_keep_the_inner_batch(stand_in):
    pg, log, _ = stand_in
    graph, n = _graph(pg)
    F = _features(n, 6)
    inner = pg.PageRank(0.85, retire=True, **RULE)
    post = inner >> pg.Top(10)
    got = post.propagate(graph, F).numpy()
    assert log == [(6, None, -1)] and "stages" in inner.last_batches[0][0]
    assert np.array_equal(got, (pg.PageRank(0.85, **RULE) >> pg.Top(10)).propagate(graph, F).numpy())


def test_declined_and_failed_calls(stand_in):
    pg, log, behaviour = stand_in
    from pygrank_amd import _lib as L
    graph, n = _graph(pg)
    F = _features(n, 7)
    want = pg.PageRank(0.85, **RULE).propagate(graph, F).numpy()
    behaviour["status"] = L.DECLINED                                # nothing was written: the plain call runs
    on = pg.PageRank(0.85, retire=True, **RULE)
    assert np.array_equal(on.propagate(graph, F).numpy(), want)
    assert log == [(7, None, -1)] and all("stages" not in column for column in on.last_batches[0])
    behaviour["status"] = 1                                         # any other status is an error, as from the plain entry
    with pytest.raises(L.EngineError):
        pg.PageRank(0.85, retire=[8, 16], **RULE).propagate(graph, F)
    assert log[-1] == (7, [8, 16], 2)


def test_keyword_of_the_other_rankers(host_engine):
    pg = host_engine
    assert pg.AbsorbingWalks(0.85, retire=[16, 4]).retire == [16, 4] and pg.AbsorbingWalks().retire is False
    assert pg.SymmetricAbsorbingRandomWalks(retire=True).retire is True and pg.SymmetricAbsorbingRandomWalks().retire is False
    assert pg.AlgorithmSelection(retire=True).retire is True and pg.AlgorithmSelection().retire is False
    with pytest.raises(Exception):
        pg.HeatKernel(retire=True)                                  # the closed-form filters have no such loop
