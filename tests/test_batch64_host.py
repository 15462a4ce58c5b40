"""include/pgh_batch64.h on the host (no GPU): its table in _lib matches the header and the Makefile, the HIP library exports the five
entries, and the Python side of ``f64_batch=`` -- which entry propagate calls, with which slab, norms and tolerance, how a wide slab is
cut, and today's column loop where the library lacks the entry or the entry DECLINED -- on the host test double, which has none of
them, with stand-ins in ``_pgh_batch64_entries`` that run the double's single-vector f64 loops column by column.  Also: the row-wise
bound tests/test_gpu_batch64.py holds the product to rejects a product whose row sums were kept in f32.
tests/test_gpu_batch64.py runs the engine's own entries."""
import ctypes as C
import gc
import os
import re
import subprocess

import numpy as np
import pytest

import batch64_common as bc
import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")
ENTRIES = ["pgh_absorb_run_batch_f64", "pgh_poly_run_batch_f64", "pgh_ppr_run_batch_f64", "pgh_sarw_run_batch_f64", "pgh_spmm_f64"]
EPS64 = float(np.finfo(np.float64).eps)
RULE = dict(tol=1e-9, max_iters=1000)


@pytest.fixture(autouse=True)
def _graphs_die_with_their_library():
    """A caught exception keeps its frames -- rankers and device graphs among their locals -- alive in a reference cycle: they are
    collected here, while the library that made their handles is still the loaded one."""
    yield
    gc.collect()


def test_header_table_and_makefile_agree():
    from pygrank_amd import _lib
    text = open(os.path.join(ROOT, "include", "pgh_batch64.h")).read()
    assert sorted(_lib.BATCH64_SIGNATURES) == sorted(set(re.findall(r"\b(pgh_[a-z0-9_]+)\s*\(", text))) == ENTRIES
    assert _lib.TABLES["pgh_batch64.h"] is _lib.BATCH64_SIGNATURES and "pgh_batch64.h" not in _lib.OPTIONAL
    for header, other in [("pgh.h", _lib.SIGNATURES), *[(h, t) for h, t in _lib.TABLES.items() if h != "pgh_batch64.h"]]:
        assert set(ENTRIES).isdisjoint(other), header
    assert _lib.DECLINED == int(re.search(r"#define\s+PGH_BATCH64_DECLINED\s+(\d+)", text).group(1)) == 2
    # the recursive loops: their f32 sibling's arguments, then in_norms; the closed form: its f32 sibling's arguments
    plain = dict(pgh_ppr_run_batch_f64=_lib.SIGNATURES["pgh_ppr_run_batch"], pgh_absorb_run_batch_f64=_lib.BATCH_SIGNATURES["pgh_absorb_run_batch"],
                 pgh_sarw_run_batch_f64=_lib.BATCH_SIGNATURES["pgh_sarw_run_batch"])
    for name, (restype, argtypes) in plain.items():
        assert _lib.BATCH64_SIGNATURES[name] == (restype, argtypes + [C.c_void_p]), name
    assert _lib.BATCH64_SIGNATURES["pgh_poly_run_batch_f64"] == _lib.BATCH_SIGNATURES["pgh_poly_run_batch"]
    makefile = open(os.path.join(ROOT, "pygrank_amd", "csrc", "Makefile")).read()
    assert re.search(r"^_build/%\.o:.*include/pgh_batch64\.h\b", makefile, re.M)
    assert re.search(r"^_build/%\.o:.*\bpgh_mm_run\.h\b", makefile, re.M)
    assert re.search(r"^SRCS\s*=.*\bpgh_spmm64\.hip\b", makefile, re.M)


def test_hip_library_exports_and_binds_the_entries():
    from pygrank_amd import _lib
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pygrank_amd", "csrc")])
    cdll = _lib.load_library(LIB)
    bound = _lib.bind_optional(cdll, _lib.BATCH64_SIGNATURES)
    assert sorted(bound) == ENTRIES and all(bound[name] is not None for name in ENTRIES)


def _features(n, width):
    rng = np.random.default_rng(width)
    F = np.zeros((n, width))
    for j in range(width):
        F[rng.choice(n, 1 + j % 7, replace=False), j] = rng.uniform(0.5, 1.5, 1 + j % 7)
    if width > 2:
        F[:, width // 2] = 0.0                                      # a zero column stays zero and is not counted
    return F


def _graph(pg, key="weighted300"):
    A, directed, _ = cases.GRAPHS[key]()
    return pg.AdjacencyWrapper(A, directed=directed), A.shape[0]


def _rankers(pg, **kw):
    """name -> (make(f64_batch), propagate keywords): every filter the f64 batch serves, each wanting f64 iterates"""
    lam = {"absorption": None}
    return {
        "pgh_ppr_run_batch_f64": (lambda on: pg.PageRank(0.85, dtype="float64", f64_batch=on, **dict(RULE, **kw)), {}),
        "pgh_absorb_run_batch_f64": (lambda on: pg.AbsorbingWalks(0.85, f64_batch=on, **dict(RULE, **kw)), lam),
        "pgh_sarw_run_batch_f64": (lambda on: pg.SymmetricAbsorbingRandomWalks(f64_batch=on, **dict(RULE, **kw)), {}),
        "pgh_poly_run_batch_f64": (lambda on: pg.HeatKernel(3, f64_batch=on, **dict(RULE, **kw)), {}),
    }


def test_default_is_off(host_engine):
    pg = host_engine
    for cls in (pg.PageRank, pg.AbsorbingWalks, pg.SymmetricAbsorbingRandomWalks, pg.HeatKernel, pg.GenericGraphFilter, pg.PageRankClosed):
        assert cls().f64_batch is False and cls(f64_batch=True).f64_batch is True


def test_host_double_has_no_entry_and_keeps_the_column_loop(host_engine):
    pg = host_engine
    from pygrank_amd import _lib
    assert all(_lib.entry(name) is None for name in ENTRIES)
    graph, n = _graph(pg)
    F = _features(n, 5)
    for name, (make, kw) in _rankers(pg).items():
        on, off = make(True), make(False)
        got, want = np.asarray(on.propagate(graph, F, **kw)), np.asarray(off.propagate(graph, F, **kw))
        assert np.array_equal(got, want), name
        assert not hasattr(on, "last_batches"), name


@pytest.fixture()
def stand_in(host_engine):
    """The host double with stand-ins for the four loops of include/pgh_batch64.h: each records what it was called with and runs the
    double's single-vector f64 entry on every column, as the header says column j behaves.  Yields (pg, log, behaviour): log gains a
    dict per call, behaviour["status"] (None: run) is what a stand-in returns instead of running."""
    from pygrank_amd import _lib as L
    cdll, log, behaviour = L.lib(), [], dict(status=None)
    assert L.entry("pgh_ppr_run_batch_f64") is None
    saved = cdll._pgh_batch64_entries

    def columns(name, g, p, out, cfg, scales, results, norms, single):
        n, b = C.c_int64(), C.c_int32()
        assert cdll.pgh_mat_shape(p, C.byref(n), C.byref(b)) == 0
        slab = np.empty((n.value, b.value))
        assert cdll.pgh_mat_d2h_f64(p, slab.ctypes.data_as(C.c_void_p)) == 0
        cfg = cfg._obj
        log.append(dict(entry=name, width=b.value, slab=slab, tol=cfg.tol, start_from_p=cfg.start_from_p,
                        norms=None if norms is None else [norms[j] for j in range(b.value)], scales=[scales[j] for j in range(b.value)]))
        if behaviour["status"] is not None:
            return behaviour["status"]
        for j in range(b.value):
            v, r = L.c_vec(), L.c_vec()
            assert cdll.pgh_vec_alloc(n.value, C.byref(v)) == 0 and cdll.pgh_vec_alloc(n.value, C.byref(r)) == 0
            assert cdll.pgh_mat_get_col(p, j, v) == 0 and cdll.pgh_vec_fill(r, 0.0) == 0
            one = L.LoopCfg.from_buffer_copy(cfg)
            one.out_scale, one.start_from_p = scales[j], 1
            res = L.LoopResult()
            if norms is None or norms[j] != 0:
                if norms is not None:
                    one.in_norm = norms[j]
                status = single(g, v, r, one, res)
                if status != 0:
                    return status
            results[j] = res
            assert cdll.pgh_mat_set_col(out, j, r) == 0
            cdll.pgh_vec_free(v), cdll.pgh_vec_free(r)
        return 0

    def ppr(g, p, out, cfg, scales, results, norms):
        return columns("pgh_ppr_run_batch_f64", g, p, out, cfg, scales, results, norms,
                       lambda g, v, r, one, res: cdll.pgh_ppr_run_f64(g, v, r, C.byref(one), C.byref(res)))

    def absorb(g, p, lam, out, cfg, scales, results, norms):
        return columns("pgh_absorb_run_batch_f64", g, p, out, cfg, scales, results, norms,
                       lambda g, v, r, one, res: cdll.pgh_absorb_run_f64(g, v, lam, r, C.byref(one), C.byref(res)))

    def sarw(g, p, out, cfg, scales, results, norms):
        return columns("pgh_sarw_run_batch_f64", g, p, out, cfg, scales, results, norms,
                       lambda g, v, r, one, res: cdll.pgh_sarw_run_f64(g, v, r, C.byref(one), C.byref(res)))

    def poly(g, p, coeffs, count, out, cfg, scales, results):
        return columns("pgh_poly_run_batch_f64", g, p, out, cfg, scales, results, None,
                       lambda g, v, r, one, res: cdll.pgh_poly_run(g, v, coeffs, count, 2, r, C.byref(one), C.byref(res)))
    cdll._pgh_batch64_entries = dict(saved, pgh_ppr_run_batch_f64=ppr, pgh_absorb_run_batch_f64=absorb, pgh_sarw_run_batch_f64=sarw,
                                     pgh_poly_run_batch_f64=poly)
    try:
        yield host_engine, log, behaviour
    finally:
        cdll._pgh_batch64_entries = saved


def _counted(ranker):
    """ranker.convergence with its finish_device_loop calls counted in the returned list"""
    calls, finish = [], ranker.convergence.finish_device_loop

    def counting(iterations, converged):
        calls.append(iterations)
        return finish(iterations, converged)
    ranker.convergence.finish_device_loop = counting
    return calls


def test_propagate_calls_the_right_entry_with_raw_slab_norms_and_tolerance(stand_in):
    pg, log, _ = stand_in
    graph, n = _graph(pg)
    F = _features(n, 7)
    F32 = F.astype(np.float32).astype(np.float64)
    for name, (make, kw) in _rankers(pg).items():
        del log[:]
        on, off = make(True), make(False)
        counted = _counted(on)
        got, want = np.asarray(on.propagate(graph, F, **kw)), np.asarray(off.propagate(graph, F, **kw))
        assert [call["entry"] for call in log] == [name]
        call = log[0]
        assert call["width"] == 7 and call["tol"] == 1e-9 and call["start_from_p"] == 1
        assert call["scales"] == list(np.abs(F32).sum(axis=0))             # preserve_norm: the columns' norms
        if name == "pgh_poly_run_batch_f64":
            sums = np.abs(call["slab"]).sum(axis=0)                         # L1-normalised in f32, the zero column stays zero
            assert np.allclose(np.delete(sums, 3), 1.0, rtol=0, atol=1e-6) and sums[3] == 0
        else:
            assert np.array_equal(call["slab"], F32), name                  # UN-normalised ...
            assert call["norms"] == list(np.abs(F32).sum(axis=0)), name      # ... with the norms beside it
        assert len(counted) == 6, name                                      # the zero column is not counted
        assert len(on.last_batches) == 1 and len(on.last_batches[0]) == 7 and all(c["f64"] is True for c in on.last_batches[0])
        assert not got[:, 3].any() and not hasattr(off, "last_batches")
        # the stand-in ran the double's own f64 loop per column: what the column loop runs
        assert np.allclose(got, want, rtol=2e-7, atol=0), name
        live = [c["iterations"] for j, c in enumerate(on.last_batches[0]) if j != 3]
        assert live[-1] == off.convergence.iteration and min(live) > 2, name


def test_tolerance_is_clamped_at_fp64_eps_and_scales_follow_preserve_norm(stand_in):
    pg, log, _ = stand_in
    graph, n = _graph(pg)
    F = _features(n, 2)
    for name, (make, kw) in _rankers(pg, tol=1e-20, max_iters=40, preserve_norm=False).items():
        del log[:]
        ranker = make(True)
        try:
            ranker.propagate(graph, F, **kw)
        except Exception:                                                   # (40 iterations need not reach fp64 eps)
            pass
        assert log and log[0]["tol"] == EPS64 and log[0]["scales"] == [1.0, 1.0], name


def test_wide_slabs_are_cut_into_chunks_of_64(stand_in):
    pg, log, _ = stand_in
    graph, n = _graph(pg)
    F = _features(n, 65)
    make, kw = _rankers(pg)["pgh_ppr_run_batch_f64"]
    on, off = make(True), make(False)
    got, want = np.asarray(on.propagate(graph, F, **kw)), np.asarray(off.propagate(graph, F, **kw))
    assert [call["width"] for call in log] == [64, 1]
    assert [len(batch) for batch in on.last_batches] == [64, 1]
    assert np.allclose(got, want, rtol=2e-7, atol=0) and not got[:, 32].any()


def test_declined_call_keeps_the_column_loop_and_errors_raise(stand_in):
    pg, log, behaviour = stand_in
    from pygrank_amd import _lib as L
    graph, n = _graph(pg)
    F = _features(n, 4)
    for name, (make, kw) in _rankers(pg).items():
        del log[:]
        behaviour["status"] = L.DECLINED
        on, off = make(True), make(False)
        got, want = np.asarray(on.propagate(graph, F, **kw)), np.asarray(off.propagate(graph, F, **kw))
        assert [call["entry"] for call in log] == [name]
        assert np.array_equal(got, want) and not hasattr(on, "last_batches"), name
        behaviour["status"] = 1
        with pytest.raises(L.EngineError):
            make(True).propagate(graph, F, **kw)


def test_what_the_f64_batch_does_not_serve(stand_in):
    pg, log, _ = stand_in
    graph, n = _graph(pg)
    F = _features(n, 3)
    # off by default; a tolerance the f32 loop honours; graph_dropout; the "chebyshev" form
    pg.AbsorbingWalks(0.85, **RULE).propagate(graph, F)
    pg.AbsorbingWalks(0.85, f64_batch=True, tol=1e-6).propagate(graph, F)
    pg.PageRank(0.85, f64_batch=True, error_type="iters", max_iters=5).propagate(graph, F, graph_dropout=0.25)
    pg.HeatKernel(3, f64_batch=True, coefficient_type="chebyshev", **RULE).propagate(graph, F)
    assert log == []
    # retire= together with f64: the plain f64 batch
    walker = pg.AbsorbingWalks(0.85, f64_batch=True, retire=True, **RULE)
    walker.propagate(graph, F)
    assert [call["entry"] for call in log] == ["pgh_absorb_run_batch_f64"] and "stages" not in walker.last_batches[0][0]
    # a tolerance below fp32 eps switches it on without dtype=
    del log[:]
    pg.PageRank(0.85, f64_batch=True, **RULE).propagate(graph, F)
    assert [call["entry"] for call in log] == ["pgh_ppr_run_batch_f64"]


@pytest.mark.parametrize("kind", ["col", "symmetric", "col-valued", "symmetric-valued"])
def test_the_product_bound_rejects_an_f32_row_accumulation(kind):
    rng = np.random.default_rng(11)
    W, hub0, hub1, empty = bc.hub_graph(rng, weights="real" if kind.endswith("valued") else "mult")
    op, _ = bc.operator_of(W, kind)
    X = bc.draw_x(rng, W.shape[0], 5)
    exact = bc.product_reference(op, X).astype(np.float64)                 # the f64 rounding of the reference: inside the bound ...
    ratio, zeros = bc.product_ratio(exact, op, X)
    assert ratio <= 1.0 and zeros
    assert not exact[empty].any() and op.nnz_row[hub0] >= 6000 and op.nnz_row[hub1] >= 1100
    bad = bc.f32_row_accumulation(op, X)                                    # ... an f32 running sum: far outside it
    ratio, _ = bc.product_ratio(bad, op, X)
    assert ratio > 1.0
    bound, err = bc.product_bound(op, X), np.abs(bad - exact)
    live = [j for j in range(5) if j != 2]
    assert np.all(err[hub0, live] > bound[hub0, live]) and np.all(err[hub1, live] > bound[hub1, live])
