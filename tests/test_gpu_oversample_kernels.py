"""The four entries of include/pgh_oversample.h at the C-ABI on the GPU against numpy f64 evaluated from the downloaded f32 operands
(oversampling_common.seed_floor / seed_resample / boost_forms / boost_update).

Bounds.  Floors, counts and resampled slabs are selections and integers: exact.  Update stores: relative 2^-22 per element, absolute floor
2^-148 (the store bound of tests/test_gpu_lfpr_kernels.py: one f64 product and sum leave an error far below an f32 half ulp, device and
numpy can only land on opposite sides of a rounding boundary); the floor the update returns is then compared with the minimum over the
DOWNLOADED new total, exactly.  Forms: 1e-12 relative to numpy's f64 sums (the same doubles added in another order; fresh and total
are positive here, so no sum cancels).
The slabs hold seed values 0.5 and 2 that must not count, a column without seeds, ties at the floor, negative ranks and -0.0.
Two calls return equal bits; a declined or erroneous call leaves every output untouched.  262147 rows x 3 columns are 196611 quads in 769
parts with a last quad of one element; 4099 x 64 uses every column a lane can meet."""
import ctypes as C

import numpy as np
import pytest

import oversampling_common as oc

pytestmark = pytest.mark.gpu

SHAPES = [(n, b) for n in (1, 63, 64, 65, 1025, 4099) for b in (1, 3, 64)] + [(262147, 1), (262147, 3)]
REL, FLOOR, SUM_REL = 2.0 ** -22, 2.0 ** -148, 1e-12
SENTINEL = -77.0


def _entry(name):
    from pygrank_amd import _lib as L
    fn = L.entry(name)
    assert fn is not None, name
    return fn


def _operands(n, b, positive=False):
    """(ranks, seeds) as f32-valued f64 arrays: column 1 of a slab of three or more has no seed, every other column ties at its floor
    wherever it has two seeds or more."""
    rng = np.random.default_rng(7 * n + b)
    ranks = rng.random((n, b)) + 0.25 if positive else rng.standard_normal((n, b))
    ranks = ranks.astype(np.float32).astype(np.float64)
    if not positive and n > 2:
        ranks[rng.integers(0, n, max(1, n // 16)), :] = -0.0
        ranks[rng.integers(0, n, max(1, n // 16)), :] = 0.0
    seeds = (rng.random((n, b)) < 0.3).astype(np.float64)
    seeds[rng.random((n, b)) < 0.1] = 0.5                       # must not count
    seeds[rng.random((n, b)) < 0.1] = 2.0
    if b >= 3:
        seeds[:, 1] = np.where(seeds[:, 1] == 1.0, 0.5, seeds[:, 1])
    for c in range(b):
        rows = np.flatnonzero(seeds[:, c] == 1.0)
        if len(rows) >= 2:                                      # the lowest seed rank twice: a tie at the floor
            lowest = rows[np.argmin(ranks[rows, c])]
            other = rows[0] if rows[0] != lowest else rows[1]
            ranks[other, c] = ranks[lowest, c]
    return ranks, seeds


def _counts(b):
    return (C.c_int64 * b)(*([int(SENTINEL)] * b))


def _doubles(k):
    return (C.c_double * k)(*([SENTINEL] * k))


@pytest.mark.parametrize("n,b", SHAPES)
def test_seed_floor(gpu_engine, n, b):
    pg = gpu_engine
    floor = _entry("pgh_seed_floor")
    ranks, seeds = _operands(n, b)
    R, S = pg.DeviceMatrix.from_host(ranks), pg.DeviceMatrix.from_host(seeds)
    want_floor, want_count = oc.seed_floor(R.numpy(), S.numpy())
    got = []
    for _ in range(2):
        floors, counts = _doubles(b), _counts(b)
        assert floor(R._h, S._h, floors, counts) == 0
        got.append((list(floors), list(counts)))
    print(n, b, "floors", got[0][0][:3], "counts", got[0][1][:3])
    assert got[0][1] == list(want_count)
    assert got[0][0] == list(want_floor)                        # +inf == +inf for the column without seeds
    if b >= 3:
        assert got[0][1][1] == 0 and got[0][0][1] == np.inf
    assert np.array_equal(np.array(got[0][0]).view(np.int64), np.array(got[1][0]).view(np.int64)) and got[0][1] == got[1][1]


@pytest.mark.parametrize("n,b", SHAPES)
def test_seed_resample(gpu_engine, n, b):
    pg = gpu_engine
    resample = _entry("pgh_seed_resample")
    ranks, seeds = _operands(n, b)
    R = pg.DeviceMatrix.from_host(ranks)
    floors, _ = oc.seed_floor(ranks, seeds)
    floors = np.where(np.isfinite(floors), floors, 0.25)         # the column without seeds gets a threshold of its own
    for strict in (0, 1):
        for keep_mode in ("none", "apart", "in place"):
            keep = None if keep_mode == "none" else pg.DeviceMatrix.from_host(seeds)
            out = keep if keep_mode == "in place" else pg.DeviceMatrix.from_host(np.full((n, b), SENTINEL))
            counts = _counts(b)
            fl = (C.c_double * b)(*floors)
            assert resample(R._h, fl, strict, None if keep is None else keep._h, out._h, counts) == 0
            want, want_count = oc.seed_resample(ranks, floors, strict, None if keep is None else seeds)
            got = out.numpy()
            what = (n, b, strict, keep_mode)
            assert np.array_equal(got, want), (what, int(np.sum(got != want)))
            assert list(counts) == list(want_count), what
            if not strict:                                        # the ties at the floor are in
                assert np.all(got[ranks == floors[None, :]] == 1.0)
            if keep_mode == "apart":
                again, counts2 = pg.DeviceMatrix.from_host(np.full((n, b), SENTINEL)), _counts(b)
                assert resample(R._h, fl, strict, keep._h, again._h, counts2) == 0
                assert np.array_equal(again.numpy(), got) and list(counts2) == list(counts)


@pytest.mark.parametrize("n,b", SHAPES)
def test_boost_forms(gpu_engine, n, b):
    pg = gpu_engine
    forms = _entry("pgh_boost_forms")
    fresh, seeds = _operands(n, b, positive=True)
    total = _operands(n + 1, b, positive=True)[0][:n] * 3.0
    S, R, T = (pg.DeviceMatrix.from_host(v) for v in (seeds, fresh, total))
    want = oc.boost_forms(S.numpy(), R.numpy(), T.numpy())
    got = []
    for _ in range(2):
        out = _doubles(3 * b)
        assert forms(S._h, R._h, T._h, out) == 0
        got.append(np.array(list(out)).reshape(b, 3))
    worst = float(np.max(np.abs(got[0] - want) / np.maximum(np.abs(want), 1e-300)))
    print(n, b, "forms worst relative deviation", worst)
    assert np.all(np.abs(got[0] - want) <= SUM_REL * np.abs(want)), (n, b, worst)
    assert np.array_equal(got[0].view(np.int64), got[1].view(np.int64))


@pytest.mark.parametrize("n,b", SHAPES)
def test_boost_update(gpu_engine, n, b):
    pg = gpu_engine
    update = _entry("pgh_boost_update")
    total, mask = _operands(n, b)
    fresh = _operands(n + 2, b)[0][:n]
    weights = np.linspace(-0.4, 0.9, b) if b > 1 else np.array([0.37])
    got = []
    for _ in range(2):
        T, R, M = (pg.DeviceMatrix.from_host(v) for v in (total, fresh, mask))
        floors, counts = _doubles(b), _counts(b)
        assert update(T._h, R._h, (C.c_double * b)(*weights), M._h, floors, counts) == 0
        got.append((T.numpy(), list(floors), list(counts)))
    want, _, _ = oc.boost_update(total, fresh, weights, mask)
    want32 = want.astype(np.float32).astype(np.float64)
    excess = np.abs(got[0][0] - want32) - np.maximum(REL * np.abs(want32), FLOOR)
    print(n, b, "update worst excess over the store bound", float(excess.max()))
    assert excess.max() <= 0, (n, b, float(excess.max()))
    stored_floor, stored_count = oc.seed_floor(got[0][0], mask)   # what pgh_seed_floor would return on the stored total
    assert got[0][1] == list(stored_floor) and got[0][2] == list(stored_count)
    assert np.array_equal(got[0][0].view(np.int64), got[1][0].view(np.int64))
    assert np.array_equal(np.array(got[0][1]).view(np.int64), np.array(got[1][1]).view(np.int64)) and got[0][2] == got[1][2]


def test_update_then_floor_agree(gpu_engine):
    """The update's second result is pgh_seed_floor of its first."""
    pg = gpu_engine
    n, b = 4099, 3
    total, mask = _operands(n, b)
    fresh = _operands(n + 2, b)[0][:n]
    T, R, M = (pg.DeviceMatrix.from_host(v) for v in (total, fresh, mask))
    floors, counts, floors2, counts2 = _doubles(b), _counts(b), _doubles(b), _counts(b)
    assert _entry("pgh_boost_update")(T._h, R._h, (C.c_double * b)(0.3, -0.2, 0.7), M._h, floors, counts) == 0
    assert _entry("pgh_seed_floor")(T._h, M._h, floors2, counts2) == 0
    assert list(floors) == list(floors2) and list(counts) == list(counts2)


def test_declined_and_erroneous_calls_write_nothing(gpu_engine):
    pg = gpu_engine
    from pygrank_amd import _lib as L
    DECLINED = L.DECLINED
    floor, resample, forms, update = (_entry(name) for name in ("pgh_seed_floor", "pgh_seed_resample", "pgh_boost_forms", "pgh_boost_update"))
    n = 65

    def slab(b, value=SENTINEL, rows=n):
        return pg.DeviceMatrix.from_host(np.full((rows, b), value))

    def untouched(*things):
        for thing in things:
            values = thing.numpy() if isinstance(thing, pg.DeviceMatrix) else np.array(list(thing), dtype=np.float64)
            assert np.all(values == SENTINEL), values

    # more than 64 columns: declined
    wide = [slab(65) for _ in range(4)]
    f, c, s3 = _doubles(65), _counts(65), _doubles(195)
    finite = (C.c_double * 65)(*([0.5] * 65))
    assert floor(wide[0]._h, wide[1]._h, f, c) == DECLINED
    assert resample(wide[0]._h, finite, 0, None, wide[1]._h, c) == DECLINED
    assert forms(wide[0]._h, wide[1]._h, wide[2]._h, s3) == DECLINED
    assert update(wide[0]._h, wide[1]._h, finite, wide[2]._h, f, c) == DECLINED
    untouched(f, c, s3, *wide)
    # a non-finite host argument: declined
    a, b_, m = slab(3), slab(3), slab(3)
    f, c = _doubles(3), _counts(3)
    for bad in (np.nan, np.inf, -np.inf):
        assert resample(a._h, (C.c_double * 3)(0.1, bad, 0.2), 0, None, b_._h, c) == DECLINED
        assert update(a._h, b_._h, (C.c_double * 3)(0.1, 0.2, bad), m._h, f, c) == DECLINED
    untouched(f, c, a, b_, m)
    # shape mismatches, forbidden aliasing and null arguments: errors
    other, short = slab(2), slab(3, rows=n - 1)
    for status in (floor(a._h, other._h, f, c), floor(a._h, short._h, f, c), floor(a._h, None, f, c), floor(a._h, b_._h, None, c),
                   resample(a._h, (C.c_double * 3)(0.1, 0.1, 0.1), 0, None, a._h, c),
                   resample(a._h, (C.c_double * 3)(0.1, 0.1, 0.1), 0, other._h, b_._h, c),
                   resample(a._h, None, 0, None, b_._h, c),
                   forms(a._h, b_._h, short._h, _doubles(9)), forms(a._h, None, m._h, _doubles(9)),
                   update(a._h, a._h, (C.c_double * 3)(0.1, 0.1, 0.1), m._h, f, c),
                   update(a._h, b_._h, (C.c_double * 3)(0.1, 0.1, 0.1), a._h, f, c),
                   update(a._h, b_._h, (C.c_double * 3)(0.1, 0.1, 0.1), other._h, f, c)):
        assert status not in (0, DECLINED)
    untouched(f, c, a, b_, m, other, short)
