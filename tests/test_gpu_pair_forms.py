"""pgh_pair_forms (include/pgh_supervised.h) on the GPU against numpy in f64 on the SAME f32 inputs.

Every sum is held to 1e-12 * sum |term| (f64 accumulation of terms formed in f64 from f32 values: the bound tests/test_gpu_cut_forms.py
holds such sums to; the device's and numpy's log differ by a few ulp of f64, far inside it), the count and the three maxima exactly,
and two calls to the same bits.  Scores lie in [0, 1) and the known scores in [0.1, 1) so that every logarithm is finite; one extra
case with scores and known scores of exactly 0 and 1 checks that the non-finite slots agree with numpy in kind.

Shapes: n = 1, 3 (below one workgroup), 257 (just past 256), 1024, 20 037 (odd, many parts); b = 1, 3, 5, 33 (a column per thread),
32, 64 (16-byte row loads).  Column j % 5 == 1 is all zero, column j % 5 == 2 equals the known scores."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
SLOTS = 20
SUM_TOL = 1e-12
MAXIMA = (8, 9, 10)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _handle(x):
    return None if x is None else x._h


def _call(L, scores, known_vec, known_mat, exclude_vec, exclude_mat, factors, eps, groups, b=None):
    b = scores.b if b is None else b
    out = np.full(SLOTS * b + 4, SENTINEL)
    status = L.entry("pgh_pair_forms")(_handle(scores), _handle(known_vec), _handle(known_mat), _handle(exclude_vec),
                                       _handle(exclude_mat), _ptr(factors), float(eps), groups, _ptr(out))
    return status, out


def _reference(S, K, E, factors, eps, logs):
    """(slots [b, 20], sum of |term| [b, 20]) in f64; K and E are [n] or [n, b] (E may be None)."""
    n, b = S.shape
    want, scale = np.zeros((b, SLOTS)), np.zeros((b, SLOTS))
    with np.errstate(all="ignore"):
        for j in range(b):
            k = (K if K.ndim == 1 else K[:, j]).astype(np.float64)
            keep = np.ones(n, dtype=bool) if E is None else ((E if E.ndim == 1 else E[:, j]) == 0)
            s = S[:, j].astype(np.float64) * (1.0 if factors is None else factors[j])
            s, k = s[keep], k[keep]
            terms = {0: np.ones_like(s), 1: s, 2: s * s, 3: k, 4: k * k, 5: k * s, 6: np.abs(k - s), 7: (k - s) ** 2, 11: np.abs(k)}
            if logs:
                terms.update({12: k * np.log(s + eps), 13: (1 - k) * np.log(1 - s + eps), 14: (s + eps) * np.log(s + eps),
                              15: (s + eps) * np.log(k + eps), 16: s * np.log(k)})
            for f, t in terms.items():
                want[j, f], scale[j, f] = t.sum(), np.abs(t).sum()
            for f, t in ((8, np.abs(k - s)), (9, s), (10, k)):
                want[j, f] = t.max() if len(t) else -np.inf
    return want, scale


def _check(got, want, scale, label):
    finite = np.isfinite(want)
    finite[:, MAXIMA] = False
    diff = np.abs(got[finite] - want[finite])
    err = diff / np.maximum(scale[finite], 1e-300)
    print(f"{label}: largest error over sum |term| {err.max() if err.size else 0.0:.3e} (bound {SUM_TOL:.0e})")
    assert np.array_equal(got[:, 0], want[:, 0]), label                                   # the count
    assert np.array_equal(got[:, MAXIMA], want[:, MAXIMA]), label                         # the maxima
    assert np.all(diff <= SUM_TOL * scale[finite]), (label, float(err.max()))
    other = ~finite
    other[:, MAXIMA] = False
    assert np.array_equal(np.isnan(got[other]), np.isnan(want[other])), label
    assert np.array_equal(got[other][~np.isnan(want[other])], want[other][~np.isnan(want[other])]), label    # the same infinity


def _inputs(n, b, seed):
    rng = np.random.default_rng(seed)
    K = (0.1 + 0.9 * rng.random((n, b))).astype(np.float32)
    k = (0.1 + 0.9 * rng.random(n)).astype(np.float32)
    S = (rng.random((n, b)) * 0.999).astype(np.float32)
    factors = 0.5 + 0.5 * rng.random(b)
    patterns = {"nothing": np.zeros(n), "third": (np.arange(n) % 3 == 0).astype(np.float64) * 2.5, "everything": np.ones(n)}
    E = np.stack([np.roll(patterns["third"], j) for j in range(b)], axis=1)
    return S, k, K, factors, patterns, E


SHAPES = [(n, b) for n in (1, 3, 257, 1024, 20037) for b in (1, 3, 5, 32, 33, 64)]


@pytest.mark.parametrize("n,b", SHAPES)
def test_pair_forms_against_numpy(gpu_engine, n, b):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix, DeviceVector
    assert L.entry("pgh_pair_forms") is not None
    S0, k, K, factors, patterns, E = _inputs(n, b, seed=7000 + 64 * n + b)
    eps = float(np.finfo(np.float32).eps)
    dk, dK = DeviceVector.from_host(k), DeviceMatrix.from_host(K)
    excludes = [("none", None, None, None)]
    excludes += [("vec/" + name, DeviceVector.from_host(p), None, p.astype(np.float32)) for name, p in patterns.items()]
    excludes += [("mat/third", None, DeviceMatrix.from_host(E), E.astype(np.float32)),
                 ("mat/everything", None, DeviceMatrix.from_host(np.ones((n, b))), np.ones((n, b), dtype=np.float32))]
    variant = 0
    for known_is_mat in (False, True):
        known = K if known_is_mat else k
        S = S0.copy()
        for j in range(b):
            if j % 5 == 1:
                S[:, j] = 0
            if j % 5 == 2:
                S[:, j] = known[:, j] if known_is_mat else known
        mat = DeviceMatrix.from_host(S)
        assert np.array_equal(mat.numpy().astype(np.float32), S)
        for name, ev, em, E_host in excludes:
            variant += 1
            use_factors = None if variant % 2 else factors.copy()
            if use_factors is not None:
                use_factors[[j for j in range(b) if j % 5 == 2]] = 1.0        # the columns equal to the known scores stay equal
            for groups in (L.PAIR_MOMENTS, L.PAIR_LOGS):
                label = f"n={n} b={b} known={'mat' if known_is_mat else 'vec'} exclude={name} factors={use_factors is not None} groups={groups}"
                args = (mat, None if known_is_mat else dk, dK if known_is_mat else None, ev, em, use_factors, eps, groups)
                status, out = _call(L, *args)
                assert status == 0, (label, L.lib().pgh_last_error())
                assert np.all(out[SLOTS * b:] == SENTINEL), label
                got = out[:SLOTS * b].reshape(b, SLOTS)
                want, scale = _reference(S, known, E_host, use_factors, eps, groups == L.PAIR_LOGS)
                assert np.all(got[:, 17:] == 0), label
                if groups == L.PAIR_MOMENTS:
                    assert np.all(got[:, 12:] == 0), label
                _check(got, want, scale, label)
                if name.endswith("everything"):
                    assert np.all(got[:, 0] == 0) and np.all(got[:, MAXIMA] == -np.inf), label
                    sums = [f for f in range(SLOTS) if f not in MAXIMA]
                    assert np.all(got[:, sums] == 0), label
                for j in range(b):
                    if j % 5 == 1:                # an all-zero column: max s is 0 over its kept rows, -inf where none is kept (n = 1, "third")
                        assert got[j, 1] == 0 and got[j, 2] == 0 and got[j, 5] == 0, label
                        assert got[j, 9] == (0 if want[j, 0] > 0 else -np.inf), label
                    if j % 5 == 2:
                        assert got[j, 6] == 0 and got[j, 7] == 0 and got[j, 8] in (0, -np.inf), label
                status, again = _call(L, *args)
                assert status == 0 and np.array_equal(out, again), label              # bit for bit


def test_pair_forms_non_finite_slots_agree_with_numpy_in_kind(gpu_engine):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix, DeviceVector
    assert L.entry("pgh_pair_forms") is not None
    n, eps = 1000, float(np.finfo(np.float32).eps)
    rng = np.random.default_rng(31)
    k = (rng.random(n) < 0.3).astype(np.float32)                      # 0 / 1 labels: log(k) is -inf or 0
    for b in (4, 5):
        S = rng.random((n, b)).astype(np.float32)
        S[::7, 0] = 1.0
        S[::5, 0] = 0.0                                               # 0 * log(0): nan
        S[:, 1] = k                                                   # s == k: 0 * -inf and 1 * 0
        S[:, 2] = 1.0
        S[:, 3] = np.where(k != 0, S[:, 3], 0)                        # s == 0 wherever k == 0
        status, out = _call(L, DeviceMatrix.from_host(S), DeviceVector.from_host(k), None, None, None, None, eps, L.PAIR_LOGS)
        assert status == 0, L.lib().pgh_last_error()
        got = out[:SLOTS * b].reshape(b, SLOTS)
        want, scale = _reference(S, k, None, None, eps, True)
        assert np.isnan(want[0, 16]) and np.isnan(want[1, 16]) and np.isnan(want[3, 16]) and want[2, 16] == -np.inf
        assert np.all(np.isfinite(want[:, 12:16]))
        _check(got, want, scale, f"non-finite b={b}")


def test_pair_forms_refusals_leave_the_output_alone(gpu_engine):
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix, DeviceVector
    assert L.entry("pgh_pair_forms") is not None
    n, eps = 300, float(np.finfo(np.float32).eps)
    rng = np.random.default_rng(5)

    def untouched(status, out, declined=True):
        assert (status == L.DECLINED) if declined else (status not in (0, L.DECLINED)), status
        assert np.all(out == SENTINEL)
    k, K = DeviceVector.from_host(rng.random(n)), DeviceMatrix.from_host(rng.random((n, 4)))
    mat = DeviceMatrix.from_host(rng.random((n, 4)))
    wide = DeviceMatrix.from_host(rng.random((n, 65)))
    # declined: more than 64 columns, a non-finite factor or eps
    untouched(*_call(L, wide, k, None, None, None, None, eps, L.PAIR_MOMENTS))
    untouched(*_call(L, wide, k, None, None, None, None, eps, L.PAIR_LOGS))
    untouched(*_call(L, mat, k, None, None, None, np.array([1.0, np.nan, 1.0, 1.0]), eps, L.PAIR_MOMENTS))
    untouched(*_call(L, mat, k, None, None, None, np.array([1.0, 1.0, np.inf, 1.0]), eps, L.PAIR_LOGS))
    untouched(*_call(L, mat, k, None, None, None, None, float("nan"), L.PAIR_LOGS))
    untouched(*_call(L, mat, k, None, None, None, None, float("inf"), L.PAIR_MOMENTS))
    # errors: shapes, both or neither known, both excludes, a null output, unknown groups
    short, narrow = DeviceVector.from_host(rng.random(n - 1)), DeviceMatrix.from_host(rng.random((n, 3)))
    untouched(*_call(L, mat, short, None, None, None, None, eps, L.PAIR_MOMENTS), declined=False)
    untouched(*_call(L, mat, None, narrow, None, None, None, eps, L.PAIR_MOMENTS), declined=False)
    untouched(*_call(L, mat, k, None, short, None, None, eps, L.PAIR_MOMENTS), declined=False)
    untouched(*_call(L, mat, k, None, None, narrow, None, eps, L.PAIR_MOMENTS), declined=False)
    untouched(*_call(L, mat, None, DeviceMatrix.from_host(rng.random((n + 1, 4))), None, None, None, eps, L.PAIR_LOGS), declined=False)
    untouched(*_call(L, mat, k, K, None, None, None, eps, L.PAIR_MOMENTS), declined=False)
    untouched(*_call(L, mat, None, None, None, None, None, eps, L.PAIR_MOMENTS), declined=False)
    untouched(*_call(L, mat, k, None, k, K, None, eps, L.PAIR_MOMENTS), declined=False)
    untouched(*_call(L, mat, k, None, None, None, None, eps, 7), declined=False)
    status = L.entry("pgh_pair_forms")(mat._h, k._h, None, None, None, None, eps, L.PAIR_MOMENTS, None)
    assert status not in (0, L.DECLINED)
    # and the entry still serves the next request
    status, out = _call(L, mat, k, None, None, None, None, eps, L.PAIR_LOGS)
    assert status == 0 and np.all(out[:12] != SENTINEL)
