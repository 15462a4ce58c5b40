"""The five entries of include/pgh_post.h at the C-ABI on the GPU against numpy on the downloaded f32 operands.

Bounds.  The select, the compare and the ordinals are selections, 0 / 1 and positions: exact (== for the select, where -0.0 and +0.0
tie), and equal to pgh_vec_kth_largest / pgh_ewise_vs / pgh_vec_ordinals on every column.  Affine and row_op: rtol = 2 * eps32 against
the same formula in numpy float32 (the bar of pgh_mat_div_cols in kernel_checks.py), and exactly the bits the vector primitives
(pgh_ewise_vs, pgh_ewise_vv) store for the column.
Shapes: n in (1, 63, 64, 65, 1025, 4099) x b in (1, 3, 64) and (262147, 3): lane and quad tails, every column a lane can meet (b = 3
makes 63 wide columns of the select's 64 lanes), several grid periods.
Columns, by kind: normal values with -0.0, +0.0, +-inf, denormals, negatives and a planted tie; all equal; two values; keys that differ
only in the lowest byte; keys that differ only in the top byte.  A slab of fewer than five columns starts at kind n % 5.
Two calls return equal bits; a declined or erroneous call leaves every output untouched."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(n, b) for n in (1, 63, 64, 65, 1025, 4099) for b in (1, 3, 64)] + [(262147, 3)]
EPS32 = float(np.finfo(np.float32).eps)
SENTINEL = -77.0


def _entry(name):
    from pygrank_amd import _lib as L
    fn = L.entry(name)
    assert fn is not None, name
    return fn


def _bits(values):
    return np.asarray(values, dtype=np.uint32).view(np.float32).astype(np.float64)


def _column(rng, n, kind):
    if kind == 0:
        x = rng.standard_normal(n).astype(np.float32).astype(np.float64)
        specials = [-0.0, 0.0, np.inf, -np.inf, 1e-40, -3e-42, 1.4e-45, 0.5, 0.5, 0.5, -0.0, 0.0]
        rows = rng.permutation(n)[:len(specials)]
        x[rows] = np.asarray(specials[:len(rows)], dtype=np.float32).astype(np.float64)
        return x
    if kind == 1:
        return np.full(n, np.float64(np.float32(0.3)))
    if kind == 2:
        return np.where(rng.random(n) < 0.5, -1.5, 2.25)
    if kind == 3:
        return _bits(0x3F800000 | rng.integers(0, 256, n, dtype=np.uint32))
    return _bits((rng.integers(0, 256, n, dtype=np.uint32) << 24) | 0x00123456)      # exponent bit 23 is 0: finite, some denormal


def _slab(n, b):
    rng = np.random.default_rng(11 * n + b)
    first = n % 5 if b < 5 else 0
    return np.stack([_column(rng, n, (first + j) % 5) for j in range(b)], axis=1)


def _doubles(k):
    return (C.c_double * k)(*([SENTINEL] * k))


def _ks(n, column):
    """1, 2, n // 2, n - 1, n and a k on each side of both ends of the longest tie of `column` in descending order."""
    ks = {1, 2, n // 2, n - 1, n}
    order = np.sort(column)[::-1]
    starts = np.flatnonzero(np.r_[True, order[1:] != order[:-1]])
    ends = np.r_[starts[1:], n]
    longest = int(np.argmax(ends - starts))
    s, e = int(starts[longest]), int(ends[longest])             # positions s .. e - 1 (0-based) tie
    ks |= {s, s + 1, e, e + 1}
    return sorted(k for k in ks if 1 <= k <= n)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("n,b", SHAPES)
def test_kth_largest(gpu_engine, n, b):
    pg = gpu_engine
    select = _entry("pgh_post_kth_largest")
    M = pg.DeviceMatrix.from_host(_slab(n, b))
    host = M.numpy()
    columns = M.columns()
    descending = np.sort(host, axis=0)[::-1]
    for k in _ks(n, host[:, 0]):
        values = _doubles(b + 1)
        assert select(M._h, k, values) == 0
        assert values[b] == SENTINEL
        got = np.array(values[:b])
        assert np.all(got == descending[k - 1]), (n, b, k, np.flatnonzero(got != descending[k - 1])[:4])
        alone = np.array([column.kth_largest(k) for column in columns])
        assert np.all(got == alone), (n, b, k)
        again = _doubles(b)
        assert select(M._h, k, again) == 0
        assert _same_bits(got, np.array(again[:]))
    for k in (0, n + 1, -3):
        values = _doubles(b)
        status = select(M._h, k, values)
        assert status not in (0, 2) and list(values) == [SENTINEL] * b, (n, b, k, status)


def test_kth_largest_declines_65_columns_and_keeps_a_nan_to_its_column(gpu_engine):
    pg = gpu_engine
    from pygrank_amd import _lib as L
    select = _entry("pgh_post_kth_largest")
    wide = pg.DeviceMatrix.from_host(np.ones((5, 65)))
    values = _doubles(65)
    assert select(wide._h, 1, values) == L.DECLINED and list(values) == [SENTINEL] * 65
    assert select(None, 1, values) not in (0, L.DECLINED)
    for n in (1, 65, 4099):
        S = _slab(n, 64)[:, :3].copy()
        S[n // 2, 1] = np.nan
        M = pg.DeviceMatrix.from_host(S)
        host = M.numpy()
        for k in sorted({1, (n + 1) // 2, n}):
            values = _doubles(3)
            assert select(M._h, k, values) == 0
            for j in (0, 2):
                assert values[j] == np.sort(host[:, j])[::-1][k - 1], (n, k, j)


def _refusals(call, pg, L, n=5):
    """call(m, out) -> status: 65 columns decline, other shapes and out == m are errors; the output keeps its sentinel."""
    wide, wide_out = pg.DeviceMatrix.from_host(np.ones((n, 65))), pg.DeviceMatrix.from_host(np.full((n, 65), SENTINEL))
    assert call(wide, wide_out) == L.DECLINED
    assert np.all(wide_out.numpy() == SENTINEL)
    m, other = pg.DeviceMatrix.from_host(np.ones((n, 3))), pg.DeviceMatrix.from_host(np.full((n, 2), SENTINEL))
    assert call(m, other) not in (0, L.DECLINED) and np.all(other.numpy() == SENTINEL)
    assert call(m, m) not in (0, L.DECLINED) and np.all(m.numpy() == 1.0)


def _sentinel_slab(pg, n, b):
    return pg.DeviceMatrix.from_host(np.full((n, b), SENTINEL))


@pytest.mark.parametrize("n,b", SHAPES)
def test_col_threshold(gpu_engine, n, b):
    pg = gpu_engine
    from pygrank_amd import _lib as L
    threshold = _entry("pgh_post_col_threshold")
    M = pg.DeviceMatrix.from_host(_slab(n, b))
    host = M.numpy()
    rng = np.random.default_rng(n + b)
    stored = host[rng.integers(0, n, b), np.arange(b)]              # a stored value of every column: ties at the cut
    stored = np.where(np.isfinite(stored), stored, 0.0)
    cuts = stored * (1.0 + 1e-12)                                   # not f32 values: the entry rounds them, to the stored ones
    cuts32 = cuts.astype(np.float32)
    assert np.array_equal(cuts32.astype(np.float64), stored)
    host32 = host.astype(np.float32)
    for inclusive in (0, 1):
        out = _sentinel_slab(pg, n, b)
        assert threshold(M._h, (C.c_double * b)(*cuts), inclusive, out._h) == 0
        got = out.numpy()
        want = (host32 >= cuts32[None, :]) if inclusive else (host32 > cuts32[None, :])
        assert np.array_equal(got, want.astype(np.float64)), (n, b, inclusive)
        for j, column in enumerate(M.columns()):
            alone = pg.DeviceVector.empty(n)
            L.check(L.lib().pgh_ewise_vs(L.GE if inclusive else L.GT, column._h, float(cuts[j]), 0, alone._h))
            assert np.array_equal(got[:, j], alone.numpy()), (n, b, inclusive, j)
        again = _sentinel_slab(pg, n, b)
        assert threshold(M._h, (C.c_double * b)(*cuts), inclusive, again._h) == 0
        assert _same_bits(got, again.numpy())


@pytest.mark.parametrize("n,b", SHAPES)
def test_col_affine(gpu_engine, n, b):
    pg = gpu_engine
    from pygrank_amd import _lib as L
    affine = _entry("pgh_post_col_affine")
    M = pg.DeviceMatrix.from_host(_slab(n, b))
    host = M.numpy()
    rng = np.random.default_rng(3 * n + b)
    sub, div = rng.standard_normal(b), rng.random(b) + 0.5
    div[rng.random(b) < 0.3] *= -1.0
    div[b // 2] = 0.0                                               # this column is copied, whatever its `sub`
    out = _sentinel_slab(pg, n, b)
    assert affine(M._h, (C.c_double * b)(*sub), (C.c_double * b)(*div), out._h) == 0
    got = out.numpy()
    host32 = host.astype(np.float32)
    with np.errstate(all="ignore"):
        want = ((host32 - sub.astype(np.float32)[None, :]) / div.astype(np.float32)[None, :]).astype(np.float64)
    want[:, b // 2] = host[:, b // 2]
    with np.errstate(invalid="ignore"):                             # (inf - inf where both hold the same infinity)
        near = (got == want) | (np.abs(got - want) <= 2 * EPS32 * np.abs(want))
    assert np.all(near), (n, b, np.argwhere(~near)[:4])
    assert _same_bits(got[:, b // 2], host[:, b // 2])              # -0.0 stays -0.0
    for j, column in enumerate(M.columns()):
        if j == b // 2:
            continue
        shifted, alone = pg.DeviceVector.empty(n), pg.DeviceVector.empty(n)
        L.check(L.lib().pgh_ewise_vs(L.SUB, column._h, float(sub[j]), 0, shifted._h))
        L.check(L.lib().pgh_ewise_vs(L.DIV, shifted._h, float(div[j]), 0, alone._h))
        assert _same_bits(got[:, j], alone.numpy()), (n, b, j)
    again = _sentinel_slab(pg, n, b)
    assert affine(M._h, (C.c_double * b)(*sub), (C.c_double * b)(*div), again._h) == 0
    assert _same_bits(got, again.numpy())


@pytest.mark.parametrize("n,b", SHAPES)
def test_row_op(gpu_engine, n, b):
    pg = gpu_engine
    from pygrank_amd import _lib as L
    row_op = _entry("pgh_post_row_op")
    M = pg.DeviceMatrix.from_host(_slab(n, b))
    host32 = M.numpy().astype(np.float32)
    rng = np.random.default_rng(5 * n + b)
    v = pg.DeviceVector.from_host(np.abs(rng.standard_normal(n)) + 0.125)
    v32 = v.numpy().astype(np.float32)
    offset = 1e-3 * (1.0 + 1e-12)
    for op in (L.POST_ROW_SUB, L.POST_ROW_SWEEP):
        out = _sentinel_slab(pg, n, b)
        assert row_op(M._h, v._h, op, offset, out._h) == 0
        got = out.numpy()
        with np.errstate(all="ignore"):
            want = host32 - v32[:, None] if op == L.POST_ROW_SUB else host32 / (v32 + np.float32(offset))[:, None]
        want = want.astype(np.float64)
        with np.errstate(invalid="ignore"):
            near = (got == want) | (np.abs(got - want) <= 2 * EPS32 * np.abs(want))
        assert np.all(near), (n, b, op, np.argwhere(~near)[:4])
        under = pg.DeviceVector.empty(n)
        L.check(L.lib().pgh_ewise_vs(L.ADD, v._h, offset, 0, under._h))
        for j, column in enumerate(M.columns()):
            alone = pg.DeviceVector.empty(n)
            if op == L.POST_ROW_SUB:
                L.check(L.lib().pgh_ewise_vv(L.SUB, column._h, v._h, alone._h))
            else:
                L.check(L.lib().pgh_ewise_vv(L.DIV, column._h, under._h, alone._h))
            assert _same_bits(got[:, j], alone.numpy()), (n, b, op, j)
        again = _sentinel_slab(pg, n, b)
        assert row_op(M._h, v._h, op, offset, again._h) == 0
        assert _same_bits(got, again.numpy())


@pytest.mark.parametrize("n,b", SHAPES)
def test_ordinals(gpu_engine, n, b):
    pg = gpu_engine
    ordinals = _entry("pgh_post_ordinals")
    M = pg.DeviceMatrix.from_host(_slab(n, b))
    host = M.numpy()
    out = _sentinel_slab(pg, n, b)
    assert ordinals(M._h, out._h) == 0
    got = out.numpy()
    for j, column in enumerate(M.columns()):
        assert np.array_equal(got[:, j], column.ordinals().numpy()), (n, b, j)
        want = np.empty(n)
        want[np.argsort(-host[:, j], kind="stable")] = np.arange(1, n + 1)      # descending, ties in ascending row order
        assert np.array_equal(got[:, j], want), (n, b, j)
    again = _sentinel_slab(pg, n, b)
    assert ordinals(M._h, again._h) == 0
    assert _same_bits(got, again.numpy())


def test_refusals_leave_the_output_untouched(gpu_engine):
    pg = gpu_engine
    from pygrank_amd import _lib as L
    some = (C.c_double * 65)(*([0.5] * 65))
    v = pg.DeviceVector.from_host(np.ones(5))
    short = pg.DeviceVector.from_host(np.ones(4))
    _refusals(lambda m, out: _entry("pgh_post_col_threshold")(m._h, some, 1, out._h), pg, L)
    _refusals(lambda m, out: _entry("pgh_post_col_affine")(m._h, some, some, out._h), pg, L)
    _refusals(lambda m, out: _entry("pgh_post_row_op")(m._h, v._h, L.POST_ROW_SWEEP, 0.0, out._h), pg, L)
    _refusals(lambda m, out: _entry("pgh_post_ordinals")(m._h, out._h), pg, L)
    m, out = pg.DeviceMatrix.from_host(np.ones((5, 3))), _sentinel_slab(pg, 5, 3)
    assert _entry("pgh_post_row_op")(m._h, v._h, 7, 0.0, out._h) not in (0, L.DECLINED)            # an unknown op
    assert _entry("pgh_post_row_op")(m._h, short._h, L.POST_ROW_SUB, 0.0, out._h) not in (0, L.DECLINED)
    assert _entry("pgh_post_col_threshold")(m._h, None, 1, out._h) not in (0, L.DECLINED)
    assert np.all(out.numpy() == SENTINEL)
