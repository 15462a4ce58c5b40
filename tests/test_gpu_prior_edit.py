"""pgh_prior_edit (include/pgh_fair.h) at the C-ABI on the GPU: every shape x probes x buckets x skew, each with all four kinds of
operands (personalization sparse 0/1 or dense positive, sensitive binary or fractional), against the formula in numpy f64 from the
downloaded f32 operands, rounded once to f32.

Bound: relative 2^-22 per element (two f32 ulps).  An f64 exp and about ten f64 operations leave an error far below an f32 half ulp, so
the device and numpy can only differ by landing on opposite sides of a rounding boundary: one ulp, up to 2 * 2^-23 relative at the
bottom of a binade.  Values in the subnormal range get the absolute floor 2 * 2^-149.  Two calls return equal bits; the refusals leave
`out` untouched."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 257, 4099]
PROBES = [1, 3, 10, 63, 64]
BUCKETS = [0, 1, 2, 4]
REL, FLOOR = 2.0 ** -22, 2.0 ** -148


def _params(rng, probes, buckets):
    """Candidates from the optimiser's box, its corners included: a in {0, 1}, b = +-5, last parameter 0 and 1."""
    P = np.empty((probes, 4 * buckets + 1))
    for t in range(buckets):
        P[:, 4 * t:4 * t + 2] = rng.random((probes, 2))
        P[:, 4 * t + 2:4 * t + 4] = rng.uniform(-5, 5, (probes, 2))
    P[:, -1] = rng.random(probes)
    corners = rng.random(P.shape) < 0.25
    low = np.tile(np.array([0, 0, -5, -5] * buckets + [0], dtype=np.float64), (probes, 1))
    high = np.tile(np.array([1, 1, 5, 5] * buckets + [1], dtype=np.float64), (probes, 1))
    P = np.where(corners, np.where(rng.random(P.shape) < 0.5, low, high), P)
    P[0, -1] = 0.0
    P[-1, -1] = 1.0 if probes > 1 else P[-1, -1]
    return np.ascontiguousarray(P)


def _operands(pg, rng, n, variant):
    pers = (rng.random(n) < 0.1).astype(np.float64) if variant & 1 else rng.random(n) + 0.01
    sens = (rng.random(n) < 0.2).astype(np.float64) if variant & 2 else rng.random(n)
    ranks = rng.random(n) ** 4 + 1e-6
    return [pg.DeviceVector.from_host(v) for v in (pers, sens, ranks)]


def _expected(pers, sens, ranks, rank_max, P, buckets, skew):
    p, s = np.asarray(pers, dtype=np.float64)[:, None], np.asarray(sens, dtype=np.float64)[:, None]
    r = np.asarray(ranks, dtype=np.float64)[:, None] / rank_max
    d = r - p if skew else np.abs(r - p)
    res = r * np.ones((1, P.shape[0])) if buckets == 0 else 0
    for t in range(buckets):
        a = s * (P[:, 4 * t] - P[:, 4 * t + 1]) + P[:, 4 * t + 1]
        b = s * (P[:, 4 * t + 2] - P[:, 4 * t + 3]) + P[:, 4 * t + 3]
        res = res + (1 - a) * np.exp(b * d) + a * np.exp(-b * d)
    return ((1.0 - P[:, -1]) * res + p * P[:, -1]).astype(np.float32).astype(np.float64)


def _call(vectors, rank_max, P, buckets, probes, skew, out):
    from pygrank_amd import _lib as L
    entry = L.entry("pgh_prior_edit")
    assert entry is not None
    return entry(vectors[0]._h, vectors[1]._h, vectors[2]._h, float(rank_max), P.ctypes.data_as(C.c_void_p), buckets, probes, skew, out._h)


@pytest.mark.parametrize("n", SIZES)
def test_formula_on_every_shape(gpu_engine, n):
    pg = gpu_engine
    worst, case = 0.0, 0
    for probes in PROBES:
        for buckets in BUCKETS:
            for skew in (0, 1):
                for variant in range(4):
                    rng = np.random.default_rng(10000 * n + 1000 * probes + 100 * buckets + 10 * skew + variant)
                    vectors = _operands(pg, rng, n, variant)
                    case += 1
                    rank_max = float(vectors[2].max())
                    P = _params(rng, probes, buckets)
                    out, again = pg.DeviceMatrix.empty(n, probes), pg.DeviceMatrix.empty(n, probes)
                    assert _call(vectors, rank_max, P, buckets, probes, skew, out) == 0
                    assert _call(vectors, rank_max, P, buckets, probes, skew, again) == 0
                    got = out.numpy()
                    assert np.array_equal(got.view(np.int64), again.numpy().view(np.int64))         # repeatability: equal bits
                    want = _expected(*vectors, rank_max, P, buckets, skew)
                    assert want.shape == got.shape and np.all(np.isfinite(want))
                    excess = np.abs(got - want) / (REL * np.abs(want) + FLOOR)
                    worst = max(worst, float(excess.max()))
                    assert excess.max() <= 1.0, (n, probes, buckets, skew, variant, np.unravel_index(excess.argmax(), excess.shape))
    print(f"n {n}: largest error {worst:.3f} of the bound over {case} cases")


def test_refusals_write_nothing(gpu_engine):
    pg = gpu_engine
    from pygrank_amd import _lib as L
    rng = np.random.default_rng(7)
    n = 257
    vectors = _operands(pg, rng, n, 0)
    sentinel = -123.5

    def filled(rows, cols):
        return pg.DeviceMatrix.from_host(np.full((rows, cols), sentinel))

    def untouched(out):
        return bool(np.all(out.numpy() == sentinel))

    good = _params(rng, 10, 1)
    nan = good.copy()
    nan[3, 2] = np.nan
    declined = [(_params(rng, 65, 1), 1, 65, 1.0, filled(n, 65)), (_params(rng, 10, 5), 5, 10, 1.0, filled(n, 10)),
                (nan, 1, 10, 1.0, filled(n, 10)), (good, 1, 10, 0.0, filled(n, 10)), (good, 1, 10, float("inf"), filled(n, 10))]
    for P, buckets, probes, rank_max, out in declined:
        assert _call(vectors, rank_max, P, buckets, probes, 0, out) == L.DECLINED, (buckets, probes, rank_max)
        assert b"declined" in L.lib().pgh_last_error()
        assert untouched(out)
    short = pg.DeviceVector.from_host(np.ones(n - 1))
    errors = [([vectors[0], short, vectors[2]], filled(n, 10)), (vectors, filled(n - 1, 10)), (vectors, filled(n, 9))]
    for operands, out in errors:
        status = _call(operands, 1.0, good, 1, 10, 0, out)
        assert status not in (0, L.DECLINED)
        assert untouched(out)
    out = filled(n, 10)
    assert _call(vectors, 1.0, good, 1, 10, 0, out) == 0 and not untouched(out)
