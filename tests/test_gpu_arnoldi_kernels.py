"""pgh_basis_dots and pgh_arnoldi_close (include/pgh_arnoldi.h) at the C-ABI on the GPU against numpy f64 evaluated from the downloaded
f32 operands.

Bounds, all derivable (those of tests/test_gpu_krylov_kernels.py).
  Stores: |got - f32(want)| <= max(2^-22 |want|, 2^-148) + 2^-50 (|w| + sum_j |c_j q_ij|).  A handful of f64 operations leave an error far
    below an f32 half ulp, so device and numpy can only land on opposite sides of a rounding boundary; the second term covers the f64
    rounding of the terms where they cancel (w is built to cancel against Q c on a third of the rows).
  Sums: 1e-12 times the sum of the MAGNITUDES of the terms: both sides add the same doubles in different orders.  The sums of the close
    are taken over the STORED out, so they are compared with sums over the downloaded out.
Two calls return equal bits; basis[:, col] equals out to the bit and the other columns stay as they were; a declined or erroneous call
leaves every output untouched.  Every count meets a slab wider than it (col first and last allowed) and, where that is a different
slab, one exactly as wide (col = -1).  At 262147 rows every count runs once with the width and column taken in turn."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1023, 1025, 4099, 262147]
COUNTS = [1, 3, 4, 5, 17, 63, 64]
REL, FLOOR, CANCEL, SUM_REL = 2.0 ** -22, 2.0 ** -148, 2.0 ** -50, 1e-12
DECLINED = 2
SENTINEL = -7.0


def _entries():
    from pygrank_amd import _lib as L
    dots, close = L.entry("pgh_basis_dots"), L.entry("pgh_arnoldi_close")
    assert dots is not None and close is not None
    return dots, close


def _ptr(array):
    return array.ctypes.data_as(C.POINTER(C.c_double))


def _shapes(count):
    """[(slab width, col)]: wider than count with the first and the last column allowed, and exactly count wide without a column."""
    width = min(count + 3, 64)
    shapes = [(count, -1)]
    if width > count:
        shapes += [(width, count)] + ([(width, width - 1)] if width - 1 > count else [])
    return shapes


def _operands(n, width, count, seed):
    rng = np.random.default_rng(seed)
    host = np.float32(rng.random((n, width)) - 0.5)
    host[rng.random(n) < 0.1] = 0.0
    coeffs = np.ascontiguousarray((rng.random(count) - 0.5) * 10.0 ** rng.integers(-3, 2, count))
    w = np.float32(rng.random(n) - 0.5)
    projection = host[:, :count].astype(np.float64) @ coeffs
    near = rng.random(n) < 0.33                             # w close to Q c on a third of the rows: the difference cancels
    w[near] = np.float32(projection[near] * (1 + 1e-6 * rng.random(int(near.sum()))))
    return host, coeffs, w


def _check_dots(what, got, host, count, values):
    values = values.astype(np.float64)
    for j in range(count + 1):
        terms = values * values if j == count else host[:, j].astype(np.float64) * values
        assert abs(got[j] - float(terms.sum())) <= SUM_REL * float(np.abs(terms).sum()), (what, j, got[j], float(terms.sum()))


def _run(pg, n, count, width, col):
    dots, close = _entries()
    what = (n, count, width, col)
    host, coeffs, w = _operands(n, width, count, 1000 * n + 64 * count + width)
    slab = pg.DeviceMatrix.from_host(host.astype(np.float64))
    dw = pg.DeviceVector.from_host(w.astype(np.float64))
    assert np.array_equal(dw.numpy(np.float32), w) and np.array_equal(np.float32(slab.numpy()), host)
    # ---- pgh_basis_dots
    results = []
    for _ in range(2):
        got = np.full(count + 2, SENTINEL)
        assert dots(slab._h, count, dw._h, _ptr(got)) == 0, what
        results.append(got)
    assert results[0][count + 1] == SENTINEL, what
    _check_dots(what, results[0], host, count, w)
    assert np.array_equal(results[0], results[1]), what                                        # equal bits
    assert np.array_equal(np.float32(slab.numpy()), host), what                               # the pass writes nothing of size n
    # ---- pgh_arnoldi_close
    terms = host[:, :count].astype(np.float64) * coeffs
    want32 = (w.astype(np.float64) - terms.sum(axis=1)).astype(np.float32).astype(np.float64)
    scale = np.abs(w.astype(np.float64)) + np.abs(terms).sum(axis=1)
    results = []
    for _ in range(2):            # (the second call finds column `col` holding what it is about to write: the columns read are others)
        out = pg.DeviceVector.full(n, SENTINEL)
        got = np.full(count + 2, SENTINEL)
        assert close(slab._h, count, dw._h, _ptr(coeffs), out._h, col, _ptr(got)) == 0, what
        results.append((out.numpy(np.float32), got, np.float32(slab.numpy())))
    out, got, after = results[0]
    excess = np.abs(out.astype(np.float64) - want32) - (np.maximum(REL * np.abs(want32), FLOOR) + CANCEL * scale)
    assert excess.max() <= 0, (what, int(np.argmax(excess)), float(excess.max()))
    assert got[count + 1] == SENTINEL, what
    _check_dots(what, got, host, count, out)
    assert np.array_equal(out, results[1][0]) and np.array_equal(got, results[1][1]) and np.array_equal(after, results[1][2]), what
    others = [c for c in range(width) if c != col]
    assert np.array_equal(after[:, others], host[:, others]), what
    if col >= 0:
        assert np.array_equal(after[:, col], out), what
    assert np.array_equal(dw.numpy(np.float32), w), what                                       # w is read only


@pytest.mark.parametrize("n", SIZES)
def test_dots_and_close(gpu_engine, n):
    for at, count in enumerate(COUNTS):
        shapes = _shapes(count)
        for width, col in (shapes if n < 100000 else [shapes[at % len(shapes)]]):
            _run(gpu_engine, n, count, width, col)


def test_refusals_leave_everything_untouched(gpu_engine):
    pg = gpu_engine
    dots, close = _entries()
    n = 1025
    rng = np.random.default_rng(5)
    host = np.float32(rng.random((n, 8)) - 0.5)
    w = pg.DeviceVector.from_host(rng.random(n))
    short = pg.DeviceVector.from_host(rng.random(n - 1))
    wide = pg.DeviceMatrix.from_host(rng.random((65, 65)))
    w65 = pg.DeviceVector.from_host(rng.random(65))
    good = np.ascontiguousarray(rng.random(8))
    nan, inf = good.copy(), good.copy()
    nan[3], inf[0] = float("nan"), float("-inf")
    calls = [
        ("nan coefficient", DECLINED, lambda m, o, d: close(m._h, 5, w._h, _ptr(nan), o._h, 6, d)),
        ("inf coefficient", DECLINED, lambda m, o, d: close(m._h, 5, w._h, _ptr(inf), o._h, -1, d)),
        ("w length", None, lambda m, o, d: close(m._h, 5, short._h, _ptr(good), o._h, 6, d)),
        ("out length", None, lambda m, o, d: close(m._h, 5, w._h, _ptr(good), short._h, 6, d)),
        ("count 0", None, lambda m, o, d: close(m._h, 0, w._h, _ptr(good), o._h, 6, d)),
        ("count beyond the slab", None, lambda m, o, d: close(m._h, 9, w._h, _ptr(good), o._h, -1, d)),
        ("col 0 is read", None, lambda m, o, d: close(m._h, 5, w._h, _ptr(good), o._h, 0, d)),
        ("col count - 1 is read", None, lambda m, o, d: close(m._h, 5, w._h, _ptr(good), o._h, 4, d)),
        ("col beyond", None, lambda m, o, d: close(m._h, 5, w._h, _ptr(good), o._h, 8, d)),
        ("out is w", None, lambda m, o, d: close(m._h, 5, w._h, _ptr(good), w._h, 6, d)),
        ("slab of 65 columns", None, lambda m, o, d: close(wide._h, 5, w65._h, _ptr(good), pg.DeviceVector.full(65, SENTINEL)._h, 6, d)),
        ("null slab", None, lambda m, o, d: close(None, 5, w._h, _ptr(good), o._h, 6, d)),
        ("null w", None, lambda m, o, d: close(m._h, 5, None, _ptr(good), o._h, 6, d)),
        ("null coefficients", None, lambda m, o, d: close(m._h, 5, w._h, None, o._h, 6, d)),
        ("null out", None, lambda m, o, d: close(m._h, 5, w._h, _ptr(good), None, 6, d)),
        ("null dots", None, lambda m, o, d: close(m._h, 5, w._h, _ptr(good), o._h, 6, None)),
        ("dots: w length", None, lambda m, o, d: dots(m._h, 5, short._h, d)),
        ("dots: count 0", None, lambda m, o, d: dots(m._h, 0, w._h, d)),
        ("dots: count beyond the slab", None, lambda m, o, d: dots(m._h, 9, w._h, d)),
        ("dots: slab of 65 columns", None, lambda m, o, d: dots(wide._h, 5, w65._h, d)),
        ("dots: null slab", None, lambda m, o, d: dots(None, 5, w._h, d)),
        ("dots: null w", None, lambda m, o, d: dots(m._h, 5, None, d)),
        ("dots: null dots", None, lambda m, o, d: dots(m._h, 5, w._h, None)),
    ]
    before = w.numpy(np.float32)
    for what, status, call in calls:
        slab = pg.DeviceMatrix.from_host(host.astype(np.float64))
        out = pg.DeviceVector.full(n, SENTINEL)
        sums = np.full(10, SENTINEL)
        got = call(slab, out, _ptr(sums))
        assert got == DECLINED if status == DECLINED else got not in (0, DECLINED), (what, got)
        assert np.all(out.numpy(np.float32) == np.float32(SENTINEL)), what
        assert np.array_equal(np.float32(slab.numpy()), host), what
        assert np.all(sums == SENTINEL), what
        assert np.array_equal(w.numpy(np.float32), before), what


def test_passes_over_nothing(gpu_engine):
    pg = gpu_engine
    dots, close = _entries()
    slab = pg.DeviceMatrix.empty(0, 5)
    w, out = pg.DeviceVector.empty(0), pg.DeviceVector.empty(0)
    sums = np.full(5, SENTINEL)
    assert dots(slab._h, 3, w._h, _ptr(sums)) == 0
    assert list(sums) == [0.0, 0.0, 0.0, 0.0, SENTINEL]
    sums = np.full(5, SENTINEL)
    assert close(slab._h, 3, w._h, _ptr(np.ones(3)), out._h, 4, _ptr(sums)) == 0
    assert list(sums) == [0.0, 0.0, 0.0, 0.0, SENTINEL]
