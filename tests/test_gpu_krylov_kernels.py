"""pgh_lanczos_close and pgh_krylov_residuals (include/pgh_krylov.h) at the C-ABI on the GPU against numpy f64 evaluated from the
downloaded f32 operands (krylov_common.close_reference / residual_reference).

Bounds, all derivable.
  Stores: |got - f32(want)| <= max(2^-22 |want|, 2^-148) + 2^-50 (|w| + |a v| + |b u|).  The first term is the bound of
    tests/test_gpu_lfpr_kernels.py (a handful of f64 operations leave an error far below an f32 half ulp: device and numpy can only land
    on opposite sides of a rounding boundary); the second covers the f64 rounding of the three terms where they cancel.
  Sums: 1e-12 (that file's SUM_REL) times the sum of the MAGNITUDES of the terms: both sides add the same doubles in different orders,
    n * 2^-53 relative to the sum of magnitudes at worst, 3e-11 at the largest size, in practice its square root.
  absmax: count * 2^-52 times max_i sum_c |basis delta|: the inner value is computed, not stored, so the maximum is not an exact
    selection -- each of its `count` multiply-adds rounds once on either side.
Two calls return equal bits; a declined or erroneous call leaves every output untouched; basis[:, col] equals out to the bit and the
other columns stay as they were.  262147 elements take 257 workgroups: the fold sees more partials than it has lanes."""
import ctypes as C

import numpy as np
import pytest

import krylov_common as kc

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1023, 1025, 4099, 262147]
REL, FLOOR, CANCEL, SUM_REL = 2.0 ** -22, 2.0 ** -148, 2.0 ** -50, 1e-12
SLABS = [None, (1, 0), (5, 0), (5, 4), (64, 0), (64, 63)]          # (slab width, col)
COUNTS = [1, 3, 4, 5, 17, 64]
PROBES = [1, 3, 4, 5, 63, 64]
DECLINED = 2
SENTINEL = -7.0


def _entries():
    from pygrank_amd import _lib as L
    close, residuals = L.entry("pgh_lanczos_close"), L.entry("pgh_krylov_residuals")
    assert close is not None and residuals is not None
    return close, residuals


def _doubles(values):
    return np.ascontiguousarray(values, dtype=np.float64)


def _ptr(array):
    return array.ctypes.data_as(C.POINTER(C.c_double))


def _slab(pg, n, width, seed):
    host = np.float32(np.random.default_rng(seed).random((n, width)) - 0.5)
    return host, pg.DeviceMatrix.from_host(host.astype(np.float64))


@pytest.mark.parametrize("n", SIZES)
def test_close(gpu_engine, n):
    pg = gpu_engine
    close, _ = _entries()
    rng = np.random.default_rng(77 * n)
    w, v, u = [np.float32(rng.random(n) - 0.5) for _ in range(3)]
    v[rng.random(n) < 0.1] = 0.0
    # a v close to w on a third of the elements: the difference cancels
    a, b = 0.7310585786300049, -0.2689414213699951
    near = rng.random(n) < 0.33
    w[near] = np.float32(a * v[near].astype(np.float64) * (1 + 1e-6 * rng.random(int(near.sum()))))
    dw, dv, du = [pg.DeviceVector.from_host(x.astype(np.float64)) for x in (w, v, u)]
    assert np.array_equal(dw.numpy(np.float32), w)
    slabs = {}
    for with_u in (False, True):
        want, scale = kc.close_reference(w, v, a, u if with_u else None, b)
        want32 = want.astype(np.float32).astype(np.float64)
        for shape in SLABS:
            what = (n, with_u, shape)
            results = []
            for _ in range(2):
                out = pg.DeviceVector.full(n, SENTINEL)
                sums = (C.c_double * 2)(SENTINEL, SENTINEL)
                basis = None
                if shape is not None:
                    if shape[0] not in slabs:
                        slabs[shape[0]] = _slab(pg, n, shape[0], n + shape[0])[0]
                    basis = pg.DeviceMatrix.from_host(slabs[shape[0]].astype(np.float64))
                assert close(dw._h, dv._h, a, du._h if with_u else None, b, out._h, None if basis is None else basis._h,
                             0 if shape is None else shape[1], sums) == 0, what
                results.append((out.numpy(np.float32), list(sums), None if basis is None else np.float32(basis.numpy())))
            got, got_sums, got_basis = results[0]
            excess = np.abs(got.astype(np.float64) - want32) - (np.maximum(REL * np.abs(want32), FLOOR) + CANCEL * scale)
            assert excess.max() <= 0, (what, int(np.argmax(excess)), float(excess.max()))
            stored = got.astype(np.float64)
            terms = [stored * stored, stored * v.astype(np.float64)]
            for k in range(2):
                assert abs(got_sums[k] - float(terms[k].sum())) <= SUM_REL * float(np.abs(terms[k]).sum()), (what, k, got_sums[k])
            assert np.array_equal(got, results[1][0]) and got_sums == results[1][1], what          # equal bits
            if shape is not None:
                width, col = shape
                assert np.array_equal(got_basis[:, col], got), what
                others = [c for c in range(width) if c != col]
                assert np.array_equal(got_basis[:, others], slabs[width][:, others]), what
                assert np.array_equal(got_basis, results[1][2]), what
    # the operands are read only
    for dev, host in ((dw, w), (dv, v), (du, u)):
        assert np.array_equal(dev.numpy(np.float32), host)


def test_close_refusals_leave_everything_untouched(gpu_engine):
    pg = gpu_engine
    close, _ = _entries()
    n = 1025
    rng = np.random.default_rng(5)
    w, v, u = [pg.DeviceVector.from_host(rng.random(n)) for _ in range(3)]
    short = pg.DeviceVector.from_host(rng.random(n - 1))
    host, _ = _slab(pg, n, 5, 9)
    shorter = pg.DeviceMatrix.from_host(host[:-1].astype(np.float64))
    calls = [
        ("nan a", DECLINED, lambda o, m, s: close(w._h, v._h, float("nan"), u._h, 0.5, o._h, m._h, 1, s)),
        ("inf b", DECLINED, lambda o, m, s: close(w._h, v._h, 0.5, u._h, float("inf"), o._h, m._h, 1, s)),
        ("inf b without u", DECLINED, lambda o, m, s: close(w._h, v._h, 0.5, None, float("-inf"), o._h, None, 0, s)),
        ("v length", None, lambda o, m, s: close(w._h, short._h, 0.5, u._h, 0.5, o._h, m._h, 1, s)),
        ("u length", None, lambda o, m, s: close(w._h, v._h, 0.5, short._h, 0.5, o._h, m._h, 1, s)),
        ("slab length", None, lambda o, m, s: close(w._h, v._h, 0.5, u._h, 0.5, o._h, shorter._h, 1, s)),
        ("col below", None, lambda o, m, s: close(w._h, v._h, 0.5, u._h, 0.5, o._h, m._h, -1, s)),
        ("col beyond", None, lambda o, m, s: close(w._h, v._h, 0.5, u._h, 0.5, o._h, m._h, 5, s)),
        ("out is w", None, lambda o, m, s: close(w._h, v._h, 0.5, u._h, 0.5, w._h, m._h, 1, s)),
        ("out is v", None, lambda o, m, s: close(w._h, v._h, 0.5, u._h, 0.5, v._h, m._h, 1, s)),
        ("out is u", None, lambda o, m, s: close(w._h, v._h, 0.5, u._h, 0.5, u._h, m._h, 1, s)),
        ("null w", None, lambda o, m, s: close(None, v._h, 0.5, u._h, 0.5, o._h, m._h, 1, s)),
        ("null v", None, lambda o, m, s: close(w._h, None, 0.5, u._h, 0.5, o._h, m._h, 1, s)),
        ("null out", None, lambda o, m, s: close(w._h, v._h, 0.5, u._h, 0.5, None, m._h, 1, s)),
        ("null sums", None, lambda o, m, s: close(w._h, v._h, 0.5, u._h, 0.5, o._h, m._h, 1, None)),
    ]
    before = [x.numpy(np.float32) for x in (w, v, u)]
    for what, status, call in calls:
        out = pg.DeviceVector.full(n, SENTINEL)
        slab = pg.DeviceMatrix.from_host(host.astype(np.float64))
        sums = (C.c_double * 2)(SENTINEL, SENTINEL)
        got = call(out, slab, sums)
        assert got == DECLINED if status == DECLINED else got not in (0, DECLINED), (what, got)
        assert np.all(out.numpy(np.float32) == np.float32(SENTINEL)), what
        assert np.array_equal(np.float32(slab.numpy()), host), what
        assert list(sums) == [SENTINEL, SENTINEL], what
        for x, kept in zip((w, v, u), before):
            assert np.array_equal(x.numpy(np.float32), kept), what


def test_close_of_nothing(gpu_engine):
    pg = gpu_engine
    close, _ = _entries()
    empty = [pg.DeviceVector.empty(0) for _ in range(3)]
    sums = (C.c_double * 2)(SENTINEL, SENTINEL)
    assert close(empty[0]._h, empty[1]._h, 0.5, None, 0.0, empty[2]._h, None, 0, sums) == 0
    assert list(sums) == [0.0, 0.0]


@pytest.mark.parametrize("n", SIZES)
def test_residuals(gpu_engine, n):
    pg = gpu_engine
    _, residuals = _entries()
    for at, count in enumerate(COUNTS):
        width = min(count + 3, 64)                          # a slab wider than count wherever the limit of 64 columns allows it
        host, slab = _slab(pg, n, width, 31 * n + count)
        # every pair of a count and a probe count; at the largest size (it only adds block partials) every count and every probe count twice
        for probes in (PROBES if n < 100000 else (PROBES[at], PROBES[-1 - at])):
            rng = np.random.default_rng(1000 * n + 64 * count + probes)
            deltas = _doubles((rng.random((count, probes)) - 0.5) * 10.0 ** rng.integers(-6, 1, (1, probes)))
            what = (n, count, probes)
            results = []
            for _ in range(2):
                sums, tops = np.full(probes, SENTINEL), np.full(probes, SENTINEL)
                assert residuals(slab._h, _ptr(deltas), count, probes, _ptr(sums), _ptr(tops)) == 0, what
                results.append((sums, tops))
            want_sum, want_max, mag_sum, mag_max = kc.residual_reference(host, deltas)
            sums, tops = results[0]
            assert np.all(np.abs(sums - want_sum) <= SUM_REL * mag_sum), (what, float(np.max(np.abs(sums - want_sum) / mag_sum)))
            assert np.all(np.abs(tops - want_max) <= count * 2.0 ** -52 * mag_max), (what, float(np.max(np.abs(tops - want_max) / mag_max)))
            assert np.array_equal(sums, results[1][0]) and np.array_equal(tops, results[1][1]), what      # equal bits
        assert np.array_equal(np.float32(slab.numpy()), host), (n, count)                                  # nothing of size n is written


def test_residuals_refusals_leave_everything_untouched(gpu_engine):
    pg = gpu_engine
    _, residuals = _entries()
    n = 1025
    host, slab = _slab(pg, n, 8, 3)
    _, wide = _slab(pg, 65, 65, 4)
    good = _doubles(np.random.default_rng(6).random((8, 64)))
    bad = good.copy()
    bad[3, 2] = float("nan")
    calls = [
        ("nan delta", DECLINED, lambda s, t: residuals(slab._h, _ptr(bad), 8, 64, s, t)),
        ("inf delta", DECLINED, lambda s, t: residuals(slab._h, _ptr(_doubles([[float("inf")]])), 1, 1, s, t)),
        ("count 0", None, lambda s, t: residuals(slab._h, _ptr(good), 0, 4, s, t)),
        ("count beyond the slab", None, lambda s, t: residuals(slab._h, _ptr(good), 9, 4, s, t)),
        ("probes 0", None, lambda s, t: residuals(slab._h, _ptr(good), 8, 0, s, t)),
        ("probes 65", None, lambda s, t: residuals(slab._h, _ptr(good), 1, 65, s, t)),
        ("slab of 65 columns", None, lambda s, t: residuals(wide._h, _ptr(good), 8, 4, s, t)),
        ("null slab", None, lambda s, t: residuals(None, _ptr(good), 8, 4, s, t)),
        ("null deltas", None, lambda s, t: residuals(slab._h, None, 8, 4, s, t)),
        ("null abssum", None, lambda s, t: residuals(slab._h, _ptr(good), 8, 4, None, t)),
        ("null absmax", None, lambda s, t: residuals(slab._h, _ptr(good), 8, 4, s, None)),
    ]
    for what, status, call in calls:
        sums, tops = np.full(64, SENTINEL), np.full(64, SENTINEL)
        got = call(_ptr(sums), _ptr(tops))
        assert got == DECLINED if status == DECLINED else got not in (0, DECLINED), (what, got)
        assert np.all(sums == SENTINEL) and np.all(tops == SENTINEL), what
    assert np.array_equal(np.float32(slab.numpy()), host)


def test_residuals_of_nothing(gpu_engine):
    pg = gpu_engine
    _, residuals = _entries()
    slab = pg.DeviceMatrix.empty(0, 5)
    sums, tops = np.full(4, SENTINEL), np.full(4, SENTINEL)
    deltas = _doubles(np.ones((3, 3)))
    assert residuals(slab._h, _ptr(deltas), 3, 3, _ptr(sums), _ptr(tops)) == 0
    assert list(sums) == [0.0, 0.0, 0.0, SENTINEL] and list(tops) == [0.0, 0.0, 0.0, SENTINEL]
