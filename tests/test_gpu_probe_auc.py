"""pgh_probe_auc (include/pgh_tune.h) on the GPU against exact host arithmetic on the SAME f32 scores: the [n, P] product of
pgh_mat_gemm is downloaded, (positive, negative) pairs are counted in integers, and the returned AUC must equal S / (2 n_pos n_neg)
formed in f64 from that integer -- no tolerance on S.  Also against pgh_auc on the filtered columns (1e-12 relative: both are ratios
of exact counts in f64), and the declines."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _slab(rng, n, kind):
    if kind == "dense":
        return rng.random((n, 64)) - 0.3
    if kind == "ppr":                                        # most rows exactly zero: one huge tie group
        S = np.zeros((n, 64))
        rows = rng.choice(n, size=max(n // 20, 4), replace=False)
        S[rows] = rng.random((len(rows), 64)) ** 8
        return S
    if kind == "dup":                                        # few distinct rows: many ties between positives and negatives
        base = rng.random((37, 64))
        return base[rng.integers(0, 37, n)]
    raise KeyError(kind)


def _lds_limit(L, terms, probes):
    """the largest number of positives whose sorted scores still fit LDS beside the coefficients"""
    return (L.TUNE_LDS_BYTES - 8 * terms * probes) // (4 * probes)


def _check(pg, n, terms, probes, n_pos, kind="dense", exclude="some", seed=0, negative_coeffs=True):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix, DeviceVector
    rng = np.random.default_rng(seed)
    slab = DeviceMatrix.from_host(_slab(rng, n, kind))
    coeffs = rng.normal(size=(terms, probes)) if negative_coeffs else rng.random((terms, probes))
    known = np.zeros(n)
    ex = np.zeros(n)
    if exclude == "some":
        ex[rng.choice(n, size=n // 7, replace=False)] = rng.random(n // 7) + 0.5
    free = np.flatnonzero(ex == 0)
    known[rng.choice(free, size=n_pos, replace=False)] = 1.0
    if exclude == "some":                                    # ... and some positives that the exclude removes
        taken = np.flatnonzero(ex != 0)[:5]
        known[taken] = 2.0
    d_known = DeviceVector.from_host(known)
    d_ex = DeviceVector.from_host(ex) if exclude != "none" else None
    plan = L.c_plan()
    L.check(L.entry("pgh_probe_plan_create")(d_known._h, None if d_ex is None else d_ex._h, C.byref(plan)))
    try:
        pos_count, neg_count = C.c_int64(), C.c_int64()
        L.check(L.entry("pgh_probe_plan_info")(plan, C.byref(pos_count), C.byref(neg_count)))
        keep = ex == 0
        assert pos_count.value == n_pos == int(np.sum(keep & (known != 0)))
        assert neg_count.value == int(np.sum(keep & (known == 0)))
        out = (C.c_double * probes)(*([-7.0] * probes))
        flat = np.ascontiguousarray(coeffs, dtype=np.float64)
        L.check(L.entry("pgh_probe_auc")(slab._h, flat.ctypes.data_as(C.c_void_p), terms, probes, plan, out))
    finally:
        L.check(L.entry("pgh_probe_plan_destroy")(plan))
    product = slab.gemm(coeffs)
    scores = product.numpy()                                 # f32 values, exactly
    worst = 0.0
    for q in range(probes):
        pos = np.sort(scores[keep & (known != 0), q])
        neg = scores[keep & (known == 0), q]
        lb = np.searchsorted(pos, neg, side="left")
        ub = np.searchsorted(pos, neg, side="right")
        S = int(np.sum(2 * (len(pos) - ub) + (ub - lb), dtype=np.int64))
        want = S / (2 * len(pos) * len(neg))
        assert out[q] == want, (q, out[q], want, S)
        column = product.column(q)
        ref = pg.AUC(pg.filter_out(d_known, d_ex) if d_ex is not None else d_known).evaluate(
            pg.filter_out(column, d_ex) if d_ex is not None else column)
        worst = max(worst, abs(ref - out[q]) / max(abs(ref), 1e-300))
    print(f"n={n} terms={terms} P={probes} n_pos={n_pos} {kind}: largest relative difference to pgh_auc {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("probes", [1, 5, 64])
@pytest.mark.parametrize("terms", [1, 41, 64])
def test_shapes(gpu_engine, probes, terms):
    _check(gpu_engine, 20037, terms, probes, 50, seed=probes * 100 + terms)


@pytest.mark.parametrize("kind", ["ppr", "dup"])
@pytest.mark.parametrize("probes", [5, 17])
def test_tie_groups(gpu_engine, kind, probes):
    _check(gpu_engine, 30011, 41, probes, 120, kind=kind, seed=3)
    _check(gpu_engine, 30011, 41, probes, 120, kind=kind, seed=4, negative_coeffs=False, exclude="none")


def test_one_positive(gpu_engine):
    _check(gpu_engine, 5003, 41, 5, 1, seed=5)
    _check(gpu_engine, 5003, 7, 33, 1, kind="ppr", seed=6, exclude="zeros")


@pytest.mark.parametrize("terms, probes", [(41, 5), (64, 64), (12, 9)])
def test_around_the_lds_budget(gpu_engine, terms, probes):
    from pygrank_amd import _lib as L
    limit = _lds_limit(L, terms, probes)
    n = 3 * limit + 20011
    _check(gpu_engine, n, terms, probes, limit, seed=7)              # the last size searched in LDS
    _check(gpu_engine, n, terms, probes, limit + 1, seed=8)          # the first one searched in global memory
    _check(gpu_engine, n, terms, probes, min(2 * limit, L.TUNE_MAX_POSITIVES), kind="dup", seed=9)


def test_small_inputs(gpu_engine):
    _check(gpu_engine, 3, 2, 2, 1, exclude="none", seed=10)
    _check(gpu_engine, 257, 5, 3, 100, exclude="none", seed=11)


def test_declines_write_nothing(gpu_engine):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix, DeviceVector
    rng = np.random.default_rng(12)
    n = 4099
    slab = DeviceMatrix.from_host(rng.random((n, 64)))
    known = np.zeros(n)
    known[rng.choice(n, 30, replace=False)] = 1.0
    create, destroy, auc = (L.entry(name) for name in ("pgh_probe_plan_create", "pgh_probe_plan_destroy", "pgh_probe_auc"))

    def call(known_host, coeffs, terms, probes):
        plan = L.c_plan()
        vec = DeviceVector.from_host(known_host)
        L.check(create(vec._h, None, C.byref(plan)))
        out = (C.c_double * probes)(*([-7.0] * probes))
        flat = np.ascontiguousarray(coeffs, dtype=np.float64)
        status = auc(slab._h, flat.ctypes.data_as(C.c_void_p), terms, probes, plan, out)
        L.check(destroy(plan))
        return status, list(out)
    assert call(known, rng.random((65, 3)), 65, 3) == (L.DECLINED, [-7.0] * 3)
    assert call(np.zeros(n), rng.random((10, 3)), 10, 3) == (L.DECLINED, [-7.0] * 3)
    assert call(np.ones(n), rng.random((10, 3)), 10, 3) == (L.DECLINED, [-7.0] * 3)
    bad = rng.random((10, 3))
    bad[4, 1] = np.nan
    assert call(known, bad, 10, 3) == (L.DECLINED, [-7.0] * 3)
    bad[4, 1] = np.inf
    assert call(known, bad, 10, 3) == (L.DECLINED, [-7.0] * 3)
    assert b"declined" in L.lib().pgh_last_error()
    status, out = call(known, rng.random((10, 3)), 10, 3)
    assert status == 0 and all(0.0 <= v <= 1.0 for v in out)


def test_too_many_positives_decline(gpu_engine):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix, DeviceVector
    n = 3 * L.TUNE_MAX_POSITIVES
    slab = DeviceMatrix.from_host(np.random.default_rng(13).random((n, 8)))
    known = np.zeros(n)
    known[:L.TUNE_MAX_POSITIVES + 1] = 1.0
    plan = L.c_plan()
    d_known = DeviceVector.from_host(known)                  # (kept in a name: the handle must outlive the call)
    L.check(L.entry("pgh_probe_plan_create")(d_known._h, None, C.byref(plan)))
    out = (C.c_double * 2)(-7.0, -7.0)
    coeffs = np.ones((8, 2))
    status = L.entry("pgh_probe_auc")(slab._h, coeffs.ctypes.data_as(C.c_void_p), 8, 2, plan, out)
    L.check(L.entry("pgh_probe_plan_destroy")(plan))
    assert status == L.DECLINED and list(out) == [-7.0, -7.0], L.lib().pgh_last_error()
