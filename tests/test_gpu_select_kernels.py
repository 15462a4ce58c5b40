"""The entries of include/pgh_select.h at the C-ABI on the GPU against numpy on the downloaded f32 operands, exactly: indices equal,
values equal as f32 bit patterns.

pgh_vec_select: n in (1, 63, 64, 65, 257, 4097, 70001) -- a lane, a wavefront and its neighbours, a quad tail, one workgroup stretch of 4096
rows plus one row, and 18 workgroups whose counts go through the scan -- in the three modes, with a capacity that is too small (only the
count comes back), exact, generous, and without `values`.  Vectors, by kind: random signed values with -0.0, +0.0, +-inf and denormals
planted; five distinct values; a constant; all zeros.  A NaN is planted only under PGH_SELECT_NONZERO, where it is selected.
pgh_mat_topk: the same n x b in (1, 3, 17, 64) with k in (1, 2, 63, 64, 65, min(n, 4096)) and k = n where n <= 4096, against
np.lexsort((np.arange(n), -x))[:k] per column; the columns cycle through the same kinds, so far more than k rows tie with the cut in the
five-valued, constant and all-zero ones.  A NaN in one column leaves the other columns as they were.
pgh_vec_gather / pgh_vec_scatter: a round trip, untouched entries keep their bits (a NaN payload and -0.0 among them), and an unsorted list,
a duplicate, -1 and n are refused with nothing written.
The two maps store the bits numpy's float32 operations give in the order the header names; pgh_mat_split_sums is compared with the f64 sum
of those f32 products within n * eps64 * sum |terms| (the orders of two f64 sums differ).
Two calls return equal bytes; a declined or erroneous call leaves every output untouched."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 4097, 70001)
WIDTHS = (1, 3, 17, 64)
NONZERO, GT, GE = 0, 1, 2
DECLINED = 2
SPECIALS = [-0.0, 0.0, np.inf, -np.inf, 1e-40, -3e-42, 1.4e-45, 0.5, 0.5, -0.0, 0.0, -0.5]
I32P, F64P = C.POINTER(C.c_int32), C.POINTER(C.c_double)


def _entry(name):
    from pygrank_amd import _lib as L
    fn = L.entry(name)
    assert fn is not None, name
    return fn


def _column(rng, n, kind):
    """f64 holding f32 values."""
    if kind == 0:
        x = rng.standard_normal(n).astype(np.float32).astype(np.float64)
        rows = rng.permutation(n)[:len(SPECIALS)]
        x[rows] = np.asarray(SPECIALS[:len(rows)], dtype=np.float32).astype(np.float64)
        return x
    if kind == 1:
        return rng.choice(np.asarray([-2.0, -0.0, 0.0, 0.75, 3.5]), size=n)
    if kind == 2:
        return np.full(n, np.float64(np.float32(0.3)))
    return np.zeros(n)


def _kind_of(n, j):
    return (SIZES.index(n) + j) % 4


def _bits(values):
    return np.asarray(values, dtype=np.float64).astype(np.float32).view(np.uint32)


def _i32(array):
    return array.ctypes.data_as(I32P)


def _select(x, mode, cut, capacity, with_values=True):
    """(status, count, positions, the values vector or None) of one pgh_vec_select call; unused places hold -7 / -77."""
    import pygrank_amd as pg
    positions = np.full(max(capacity, 1) + 1, -7, dtype=np.int32)
    values = pg.DeviceVector.full(capacity, -77.0) if with_values else None
    count = C.c_int64(-5)
    status = _entry("pgh_vec_select")(x._h, mode, cut, capacity, _i32(positions), values._h if with_values else None, C.byref(count))
    return status, count.value, positions, values


def _passing(host, mode, cut):
    with np.errstate(invalid="ignore"):
        if mode == NONZERO:
            return np.flatnonzero(host != 0)
        cut32 = np.float32(cut)
        return np.flatnonzero(host.astype(np.float32) > cut32 if mode == GT else host.astype(np.float32) >= cut32)


@pytest.mark.parametrize("kind", range(4))
@pytest.mark.parametrize("n", SIZES)
def test_select(gpu_engine, n, kind):
    pg = gpu_engine
    rng = np.random.default_rng(5 * n + kind)
    source = _column(rng, n, kind)
    x = pg.DeviceVector.from_host(source)
    host = x.numpy()
    for mode, cut in ((NONZERO, 123.0), (GT, 0.0), (GE, 0.0), (GT, 0.3), (GE, 0.3), (GE, -np.inf), (GT, np.inf), (GE, 1e-40)):
        want = _passing(host, mode, cut)
        m = len(want)
        status, count, positions, values = _select(x, mode, cut, m)            # exact capacity
        assert status == 0 and count == m
        assert np.array_equal(positions[:m], want) and np.all(positions[m:] == -7)
        assert np.array_equal(_bits(values.numpy()), _bits(host[want]))
        again = _select(x, mode, cut, m)
        assert np.array_equal(again[2], positions) and np.array_equal(_bits(again[3].numpy()), _bits(values.numpy()))
        status, count, positions, values = _select(x, mode, cut, min(n, m + 3))  # room to spare: the places behind the count stay
        assert status == 0 and count == m and np.array_equal(positions[:m], want) and np.all(positions[m:] == -7)
        stored = values.numpy()
        assert np.array_equal(_bits(stored[:m]), _bits(host[want])) and np.all(stored[m:] == -77.0)
        status, count, positions, _ = _select(x, mode, cut, m, with_values=False)
        assert status == 0 and count == m and np.array_equal(positions[:m], want)
        if m > 0:                                                               # too small: only the count comes back
            status, count, positions, values = _select(x, mode, cut, m - 1)
            assert status == 0 and count == m and np.all(positions == -7) and np.all(values.numpy() == -77.0)


@pytest.mark.parametrize("n", SIZES)
def test_select_takes_a_nan_for_non_zero(gpu_engine, n):
    pg = gpu_engine
    rng = np.random.default_rng(n)
    source = _column(rng, n, 0)
    source[rng.integers(0, n)] = np.nan
    source[n - 1] = np.nan
    x = pg.DeviceVector.from_host(source)
    host = x.numpy()
    want = np.flatnonzero(~(host == 0))
    status, count, positions, values = _select(x, NONZERO, 0.0, n)
    assert status == 0 and count == len(want) and np.array_equal(positions[:count], want)
    stored = values.numpy()[:count]
    assert np.array_equal(np.isnan(stored), np.isnan(host[want])) and np.isnan(stored[-1])
    keep = ~np.isnan(stored)
    assert np.array_equal(_bits(stored[keep]), _bits(host[want][keep]))


def test_select_refusals(gpu_engine):
    pg = gpu_engine
    x = pg.DeviceVector.from_host(np.arange(10.0))
    select = _entry("pgh_vec_select")
    positions = np.full(11, -7, dtype=np.int32)
    count = C.c_int64(-5)
    short = pg.DeviceVector.full(3, -77.0)
    for args in ((x._h, 3, 0.0, 10, _i32(positions), None, C.byref(count)),            # an unknown mode
                 (x._h, NONZERO, 0.0, -1, _i32(positions), None, C.byref(count)),       # a negative capacity
                 (x._h, NONZERO, 0.0, 10, _i32(positions), short._h, C.byref(count)),   # values shorter than the capacity
                 (x._h, NONZERO, 0.0, 10, _i32(positions), x._h, C.byref(count)),       # values is x
                 (None, NONZERO, 0.0, 10, _i32(positions), None, C.byref(count)),
                 (x._h, NONZERO, 0.0, 10, None, None, C.byref(count)),
                 (x._h, NONZERO, 0.0, 10, _i32(positions), None, None)):
        status = select(*args)
        assert status not in (0, DECLINED)
        assert count.value == -5 and np.all(positions == -7) and np.all(short.numpy() == -77.0)
    assert np.array_equal(x.numpy(), np.arange(10.0))
    empty = pg.DeviceVector.empty(0)
    assert select(empty._h, GE, 0.0, 0, _i32(positions), None, C.byref(count)) == 0 and count.value == 0


# ---------------------------------------------------------------- gather and scatter
def _odd_bits(n, seed):
    """n f32 bit patterns: random finite values with a NaN payload, -0.0 and a denormal among them."""
    rng = np.random.default_rng(seed)
    bits = rng.standard_normal(n).astype(np.float32).view(np.uint32).copy()
    for place, pattern in zip(rng.permutation(n)[:3], (0x7FC12345, 0x80000000, 0x00000007)):
        bits[place] = pattern
    return bits


def _upload_bits(pg, bits):
    return pg.DeviceVector.from_host(bits.view(np.float32))


@pytest.mark.parametrize("n", SIZES)
def test_gather_and_scatter_round_trip(gpu_engine, n):
    pg = gpu_engine
    gather, scatter = _entry("pgh_vec_gather"), _entry("pgh_vec_scatter")
    rng = np.random.default_rng(n)
    bits = _odd_bits(n, n)
    x = _upload_bits(pg, bits)
    for share in (1.0, 0.5, 0.01):
        m = max(1, int(share * n))
        idx = np.sort(rng.permutation(n)[:m]).astype(np.int32)
        out = pg.DeviceVector.full(m + 2, -77.0)
        assert gather(x._h, _i32(idx), m, out._h) == 0
        got = out.numpy(np.float32)
        assert np.array_equal(got[:m].view(np.uint32), bits[idx]) and np.all(got[m:] == -77.0)
        background = _odd_bits(n, n + 1)
        dst = _upload_bits(pg, background)
        assert scatter(dst._h, _i32(idx), m, out._h) == 0
        want = background.copy()
        want[idx] = bits[idx]
        assert np.array_equal(dst.numpy(np.float32).view(np.uint32), want)              # the other entries keep their bits
    assert np.array_equal(x.numpy(np.float32).view(np.uint32), bits)
    assert gather(x._h, None, 0, out._h) == 0 and scatter(x._h, None, 0, out._h) == 0   # an empty list moves nothing
    assert np.array_equal(x.numpy(np.float32).view(np.uint32), bits)


@pytest.mark.parametrize("bad", [[3, 2, 5], [1, 4, 4], [-1, 2, 3], [2, 3, 10], [0, 5, 2147483647]])
def test_gather_and_scatter_refuse_a_bad_list(gpu_engine, bad):
    pg = gpu_engine
    gather, scatter = _entry("pgh_vec_gather"), _entry("pgh_vec_scatter")
    bits = _odd_bits(10, 3)
    x = _upload_bits(pg, bits)
    idx = np.asarray(bad, dtype=np.int32)
    out = pg.DeviceVector.full(3, -77.0)
    status = gather(x._h, _i32(idx), 3, out._h)
    assert status not in (0, DECLINED) and np.all(out.numpy() == -77.0)
    assert b"pgh_vec_gather" in pg._lib.lib().pgh_last_error()
    status = scatter(x._h, _i32(idx), 3, out._h)
    assert status not in (0, DECLINED) and np.array_equal(x.numpy(np.float32).view(np.uint32), bits)
    good = np.asarray([1, 2, 3, 4], dtype=np.int32)
    assert gather(x._h, _i32(good), 4, out._h) not in (0, DECLINED)                    # more than out holds
    assert scatter(x._h, _i32(good), 4, out._h) not in (0, DECLINED)                   # more than src holds
    assert gather(x._h, _i32(good), -1, out._h) not in (0, DECLINED)
    assert gather(x._h, _i32(good), 3, x._h) not in (0, DECLINED)                      # out is x
    assert np.all(out.numpy() == -77.0) and np.array_equal(x.numpy(np.float32).view(np.uint32), bits)


# ---------------------------------------------------------------- the top k
def _slab(n, b):
    rng = np.random.default_rng(13 * n + b)
    return np.stack([_column(rng, n, _kind_of(n, j)) for j in range(b)], axis=1)


def _topk(M, k, slots=None):
    slots = k * M.b if slots is None else slots
    rows = np.full(slots + 1, -7, dtype=np.int32)
    values = np.full(slots + 1, -77.0)
    status = _entry("pgh_mat_topk")(M._h, k, _i32(rows), values.ctypes.data_as(F64P))
    return status, rows, values


def _ks(n):
    return sorted({k for k in (1, 2, 63, 64, 65, min(n, 4096), n) if 1 <= k <= min(n, 4096)})


@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_topk(gpu_engine, n, b):
    pg = gpu_engine
    M = pg.DeviceMatrix.from_host(_slab(n, b))
    host = M.numpy()
    places = np.arange(n)
    order = np.stack([np.lexsort((places, -host[:, j])) for j in range(b)], axis=1)
    for k in _ks(n):
        status, rows, values = _topk(M, k)
        assert status == 0 and rows[k * b] == -7 and values[k * b] == -77.0
        rows, values = rows[:k * b].reshape(k, b), values[:k * b].reshape(k, b)
        assert np.array_equal(rows, order[:k]), k
        assert np.array_equal(_bits(values), _bits(np.take_along_axis(host, order[:k], axis=0))), k
    again = _topk(M, _ks(n)[-1])
    assert np.array_equal(again[1][:-1].reshape(-1, b), rows) and np.array_equal(again[2][:-1].reshape(-1, b).view(np.int64), values.view(np.int64))
    got_rows, got_values = M.top(_ks(n)[-1])                                            # the Python surface hands the same lists on
    assert got_rows.dtype == np.int32 and np.array_equal(got_rows, rows) and np.array_equal(got_values.view(np.int64), values.view(np.int64))


@pytest.mark.parametrize("n,b", [(65, 3), (4097, 17), (70001, 64)])
def test_topk_a_nan_stays_in_its_column(gpu_engine, n, b):
    pg = gpu_engine
    clean = _slab(n, b)
    dirty = clean.copy()
    dirty[n // 2, 1] = np.nan
    dirty[n - 1, 1] = np.nan
    k = min(n, 64)
    status, want_rows, want_values = _topk(pg.DeviceMatrix.from_host(clean), k)
    assert status == 0
    status, rows, values = _topk(pg.DeviceMatrix.from_host(dirty), k)
    assert status == 0
    others = [j for j in range(b) if j != 1]
    rows, want_rows = rows[:-1].reshape(k, b), want_rows[:-1].reshape(k, b)
    values, want_values = values[:-1].reshape(k, b), want_values[:-1].reshape(k, b)
    assert np.array_equal(rows[:, others], want_rows[:, others])
    assert np.array_equal(values[:, others].view(np.int64), want_values[:, others].view(np.int64))
    assert np.all((rows[:, 1] >= 0) & (rows[:, 1] < n))


def test_topk_declines_and_refuses(gpu_engine):
    pg = gpu_engine
    rng = np.random.default_rng(2)
    M = pg.DeviceMatrix.from_host(rng.standard_normal((4100, 2)))
    status, rows, values = _topk(M, 4097)
    assert status == DECLINED and np.all(rows == -7) and np.all(values == -77.0)
    assert b"declined" in pg._lib.lib().pgh_last_error()
    status, rows, values = _topk(M, 4096)
    assert status == 0
    for k in (0, -3, 4101):
        status, rows, values = _topk(M, k, slots=16)
        assert status not in (0, DECLINED) and np.all(rows == -7) and np.all(values == -77.0)
    wide = pg.DeviceMatrix.from_host(rng.standard_normal((70, 65)))
    status, rows, values = _topk(wide, 5)
    assert status == DECLINED and np.all(rows == -7) and np.all(values == -77.0)
    got_rows, got_values = wide.top(5)                                                  # the Python surface cuts the slab into chunks
    host = wide.numpy()
    order = np.stack([np.lexsort((np.arange(70), -host[:, j])) for j in range(65)], axis=1)[:5]
    assert np.array_equal(got_rows, order) and np.array_equal(got_values, np.take_along_axis(host, order, axis=0))
    topk = _entry("pgh_mat_topk")
    assert topk(M._h, 5, None, values.ctypes.data_as(F64P)) not in (0, DECLINED)
    assert topk(M._h, 5, _i32(rows), None) not in (0, DECLINED)
    assert topk(None, 5, _i32(rows), values.ctypes.data_as(F64P)) not in (0, DECLINED)
    assert np.all(rows == -7) and np.all(values == -77.0)


# ---------------------------------------------------------------- the slab passes of MabsMaintain and SeparateNormalization
MAP_SHAPES = [(n, b) for n in (1, 63, 65, 1025) for b in (1, 3, 5, 64)] + [(70001, 17)]


def _doubles(values):
    return np.ascontiguousarray(values, dtype=np.float64)


@pytest.mark.parametrize("n,b", MAP_SHAPES)
def test_col_scale_and_split_passes(gpu_engine, n, b):
    pg = gpu_engine
    rng = np.random.default_rng(3 * n + b)
    M = pg.DeviceMatrix.from_host(_slab(n, b) if n in SIZES and b in WIDTHS else rng.standard_normal((n, b)))
    host = M.numpy().astype(np.float32)
    factors = _doubles(rng.uniform(0.1, 3.0, b) * rng.choice([-1.0, 1.0], b))
    out = pg.DeviceMatrix.from_host(np.full((n, b), -77.0))
    assert _entry("pgh_mat_col_scale")(M._h, factors.ctypes.data_as(F64P), out._h) == 0
    with np.errstate(invalid="ignore", over="ignore"):
        want = host * factors.astype(np.float32)[None, :]
    assert np.array_equal(out.numpy().astype(np.float32).view(np.uint32), want.view(np.uint32))
    fraction = rng.random(n) if n % 2 else (rng.random(n) < 0.4).astype(np.float64)
    s = pg.DeviceVector.from_host(fraction)
    s32 = s.numpy(np.float32)
    finite = np.where(np.isfinite(host), host, np.float32(1.5))                         # (the sums are compared on finite slabs)
    F = pg.DeviceMatrix.from_host(finite.astype(np.float64))
    first, second = finite * s32[:, None], finite * (np.float32(1.0) - s32)[:, None]
    sums = np.full(2 * b + 1, -77.0)
    assert _entry("pgh_mat_split_sums")(F._h, s._h, sums.ctypes.data_as(F64P)) == 0
    assert sums[2 * b] == -77.0
    got = sums[:2 * b].reshape(b, 2)
    for j in range(b):
        for side, terms in enumerate((first[:, j], second[:, j])):
            exact = float(np.sum(terms.astype(np.float64)))
            bar = n * float(np.finfo(np.float64).eps) * float(np.sum(np.abs(terms.astype(np.float64))))
            assert abs(got[j, side] - exact) <= bar, (j, side, got[j, side], exact, bar)
    again = np.full(2 * b + 1, -77.0)
    assert _entry("pgh_mat_split_sums")(F._h, s._h, again.ctypes.data_as(F64P)) == 0 and np.array_equal(again, sums)
    a, d = _doubles(rng.uniform(0.1, 3.0, b)), _doubles(rng.uniform(0.1, 3.0, b))
    assert _entry("pgh_mat_split_blend")(F._h, s._h, a.ctypes.data_as(F64P), d.ctypes.data_as(F64P), out._h) == 0
    want = first * a.astype(np.float32)[None, :] + second * d.astype(np.float32)[None, :]
    assert np.array_equal(out.numpy().astype(np.float32).view(np.uint32), want.view(np.uint32))


def test_map_refusals(gpu_engine):
    pg = gpu_engine
    rng = np.random.default_rng(4)
    wide, narrow = pg.DeviceMatrix.from_host(rng.standard_normal((9, 65))), pg.DeviceMatrix.from_host(rng.standard_normal((9, 3)))
    wide_out, narrow_out = pg.DeviceMatrix.from_host(np.full((9, 65), -77.0)), pg.DeviceMatrix.from_host(np.full((9, 3), -77.0))
    s, short = pg.DeviceVector.from_host(rng.random(9)), pg.DeviceVector.from_host(rng.random(8))
    ones = _doubles(np.ones(65)).ctypes.data_as(F64P)
    sums = np.full(131, -77.0)
    assert _entry("pgh_mat_col_scale")(wide._h, ones, wide_out._h) == DECLINED
    assert _entry("pgh_mat_split_blend")(wide._h, s._h, ones, ones, wide_out._h) == DECLINED
    assert _entry("pgh_mat_split_sums")(wide._h, s._h, sums.ctypes.data_as(F64P)) == DECLINED
    assert _entry("pgh_mat_col_scale")(narrow._h, ones, wide_out._h) not in (0, DECLINED)       # shapes differ
    assert _entry("pgh_mat_col_scale")(narrow._h, ones, narrow._h) not in (0, DECLINED)         # out is m
    assert _entry("pgh_mat_split_blend")(narrow._h, short._h, ones, ones, narrow_out._h) not in (0, DECLINED)
    assert _entry("pgh_mat_split_sums")(narrow._h, short._h, sums.ctypes.data_as(F64P)) not in (0, DECLINED)
    assert np.all(sums == -77.0) and np.all(wide_out.numpy() == -77.0) and np.all(narrow_out.numpy() == -77.0)
