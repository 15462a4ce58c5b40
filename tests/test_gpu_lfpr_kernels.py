"""pgh_lfpr_setup and pgh_lfpr_close (include/pgh_lfpr.h) at the C-ABI on the GPU against numpy f64 evaluated from the downloaded f32
operands (lfpr_common.setup_reference / close_sums).

Bounds.  Stores: relative 2^-22 per element, absolute floor 2 * 2^-149 for subnormals -- the bound tests/test_gpu_prior_edit.py derives
(a handful of f64 operations leave an error far below an f32 half ulp: device and numpy can only land on opposite sides of a rounding
boundary).  Sums: 1e-12 relative to numpy's f64 sum over the STORED values (both sides add the same doubles in different orders: n * 2^-53
relative to the sum of magnitudes at worst, 3e-11 at the largest size, in practice its square root; the operands are drawn so that no
sum cancels to a small fraction of its terms).  The maximum of kind LINF is a selection, not a sum: exact.
Two calls return equal bits; a declined or erroneous call leaves every output untouched.  262147 elements take 257 workgroups: the fold
sees more partials than it has lanes."""
import ctypes as C

import numpy as np
import pytest

import lfpr_common as lc

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1023, 1025, 4099, 262147]
REL, FLOOR, SUM_REL = 2.0 ** -22, 2.0 ** -148, 1e-12
PHIS = [0.0, 0.2, 1.0]
MABS, L1, LINF, ITERS = range(4)


def _entries():
    from pygrank_amd import _lib as L
    setup, close = L.entry("pgh_lfpr_setup"), L.entry("pgh_lfpr_close")
    assert setup is not None and close is not None
    return setup, close


def _stores_agree(got, want, what):
    want32 = np.asarray(want, dtype=np.float64).astype(np.float32).astype(np.float64)
    excess = np.abs(np.asarray(got, dtype=np.float64) - want32) - np.maximum(REL * np.abs(want32), FLOOR)
    assert excess.max() <= 0, (what, int(np.argmax(excess)), float(excess.max()))


def _sums_agree(got, want, what, exact=()):
    for k, (a, b) in enumerate(zip(got, want)):
        if k in exact:
            assert a == b, (what, k, a, b)
        else:
            assert abs(a - b) <= SUM_REL * abs(b), (what, k, a, b)


def _setup_operands(rng, n, binary, integral, phi):
    s = (rng.random(n) < 0.2).astype(np.float64) if binary else rng.random(n)
    if integral:
        R, B = rng.integers(0, 6, n).astype(np.float64), rng.integers(0, 12, n).astype(np.float64)
    else:
        R, B = rng.random(n) * 3, rng.random(n) * 9
        R[rng.random(n) < 0.15] = 0.0
        B[rng.random(n) < 0.15] = 0.0
    # rows exactly on the edge R == phi (R + B): phi = 0.2 -> B = 4 R (0.2 * 5 R rounds to R for these R)
    edge = rng.random(n) < 0.1
    edge[0] = True
    if 0 < phi < 1:
        R[edge] = np.round(R[edge]) + 1
        B[edge] = R[edge] * round((1 - phi) / phi)
    o = rng.random(n) + 0.05
    return [np.float32(v) for v in (s, R, B, o)]


@pytest.mark.parametrize("n", SIZES)
def test_setup(gpu_engine, n):
    pg = gpu_engine
    setup, _ = _entries()
    for phi in PHIS:
        for binary in (True, False):
            for integral in (True, False):
                for with_original in (False, True):
                    rng = np.random.default_rng(1000 * n + int(10 * phi) + 100 * binary + 200 * integral + 400 * with_original)
                    host = _setup_operands(rng, n, binary, integral, phi)
                    s, R, B, o = [pg.DeviceVector.from_host(v) for v in host]
                    outs, again = [pg.DeviceVector.full(n, -7.0) for _ in range(5)], [pg.DeviceVector.full(n, -7.0) for _ in range(5)]
                    sums, sums2 = (C.c_double * 2)(), (C.c_double * 2)()
                    what = (n, phi, binary, integral, with_original)
                    assert setup(s._h, R._h, B._h, o._h if with_original else None, phi, *[v._h for v in outs], sums) == 0, what
                    assert setup(s._h, R._h, B._h, o._h if with_original else None, phi, *[v._h for v in again], sums2) == 0, what
                    want = lc.setup_reference(host[0], host[1], host[2], host[3] if with_original else None, phi)
                    got = [v.numpy(np.float32) for v in outs]
                    for name, a, b in zip(("d", "dR", "dB", "xR", "xB"), got, want):
                        _stores_agree(a, b, what + (name,))
                    if 0 < phi < 1:
                        on_edge = host[1].astype(np.float64) == phi * (host[1].astype(np.float64) + host[2])
                        assert on_edge[0]
                        assert np.all(got[1][on_edge & (host[1] != 0)] == 0)         # case 2 there: dR is an exact zero
                    _sums_agree(list(sums), [float(got[3].astype(np.float64).sum()), float(got[4].astype(np.float64).sum())], what)
                    assert list(sums) == list(sums2)
                    for a, b in zip(got, again):
                        assert np.array_equal(a, b.numpy(np.float32))


def _close_operands(rng, n, negative):
    y0 = rng.random(n) * 1e-3 + 1e-5
    if negative:
        y0[rng.random(n) < 0.2] *= -1.0
    x = y0 * (1 + 0.3 * (rng.random(n) - 0.35))           # most residual terms share a sign: the signed sum does not cancel
    xR, xB = (rng.random(n) < 0.2) * rng.random(n), rng.random(n)
    d, dR, dB = rng.random(n) * 2, rng.random(n) * 0.3, rng.random(n) * 0.8
    d[rng.random(n) < 0.1] = 0.0
    return [np.float32(v) for v in (y0, x, xR, xB, d, dR, dB)]


@pytest.mark.parametrize("n", SIZES)
def test_close(gpu_engine, n):
    pg = gpu_engine
    _, close = _entries()
    for kind in (MABS, L1, LINF):
        for alias in (False, True):
            for cR, cB in ((3e-4, 7e-4), (0.0, 7e-4), (3e-4, 0.0), (0.0, 0.0)):
                for negative in (False, True):
                    rng = np.random.default_rng(1000 * n + 10 * kind + alias + 100 * negative + int(1e6 * (cR + 2 * cB)))
                    host = _close_operands(rng, n, negative)
                    x_scale, y_scale = 1.25, 1.0 / 0.93
                    what = (n, kind, alias, cR, cB, negative)
                    results = []
                    for _ in range(2):
                        dev = [pg.DeviceVector.from_host(v) for v in host]
                        y = dev[0] if alias else pg.DeviceVector.full(n, -7.0)
                        u = pg.DeviceVector.full(n, -7.0)
                        sums = (C.c_double * 5)()
                        assert close(dev[0]._h, dev[1]._h, x_scale, *[v._h for v in dev[2:]], cR, cB, y_scale, kind, y._h, u._h, sums) == 0, what
                        results.append((y.numpy(np.float32), u.numpy(np.float32), list(sums)))
                        if not alias:
                            assert np.array_equal(dev[0].numpy(np.float32), host[0])
                    (got_y, got_u, got_sums), second = results
                    f = lambda v: v.astype(np.float64)                                   # noqa: E731
                    _stores_agree(got_y, f(host[0]) + cR * f(host[2]) + cB * f(host[3]), what + ("y",))
                    _stores_agree(got_u, f(got_y) * f(host[4]), what + ("u",))
                    want = lc.close_sums(got_y, host[1], x_scale, host[4], host[5], host[6], y_scale, kind == LINF)
                    _sums_agree(got_sums, want, what, exact=(3,) if kind == LINF else ())
                    assert np.array_equal(got_y, second[0]) and np.array_equal(got_u, second[1]) and got_sums == second[2]


def test_refusals_leave_the_outputs_untouched(gpu_engine):
    pg = gpu_engine
    from pygrank_amd import _lib as L
    setup, close = _entries()
    n = 1025
    rng = np.random.default_rng(5)
    s, R, B, o = [pg.DeviceVector.from_host(v) for v in _setup_operands(rng, n, True, True, 0.2)]
    outs = [pg.DeviceVector.full(n, -7.0) for _ in range(5)]
    short = pg.DeviceVector.full(n - 1, -7.0)
    sums = (C.c_double * 2)(-1.0, -1.0)
    handles = [v._h for v in outs]

    def untouched():
        return all(np.all(v.numpy(np.float32) == -7.0) for v in outs) and np.all(short.numpy(np.float32) == -7.0)
    for phi in (float("nan"), float("inf")):
        assert setup(s._h, R._h, B._h, None, phi, *handles, sums) == L.DECLINED and untouched()
    for bad in ((s._h, R._h, B._h, None, 0.2, short._h, *handles[1:], sums),              # a length mismatch
                (s._h, R._h, short._h, None, 0.2, *handles, sums),
                (s._h, R._h, B._h, short._h, 0.2, *handles, sums),
                (s._h, R._h, B._h, None, 0.2, handles[0], handles[0], *handles[2:], sums),    # two outputs share their memory
                (s._h, R._h, B._h, None, 0.2, s._h, *handles[1:], sums),                     # an output is an input
                (None, R._h, B._h, None, 0.2, *handles, sums),                                # null arguments
                (s._h, R._h, B._h, None, 0.2, *handles[:4], None, sums),
                (s._h, R._h, B._h, None, 0.2, *handles, None)):
        status = setup(*bad)
        assert status not in (0, L.DECLINED) and untouched(), bad
    assert list(sums) == [-1.0, -1.0]
    assert np.array_equal(s.numpy(np.float32) != 0, s.numpy(np.float32) == 1)           # the input an output was aliased with

    host = _close_operands(rng, n, False)
    dev = [pg.DeviceVector.from_host(v) for v in host]
    y, u = pg.DeviceVector.full(n, -7.0), pg.DeviceVector.full(n, -7.0)
    sums = (C.c_double * 5)(*[-1.0] * 5)
    ins = [v._h for v in dev]

    def call(y0=ins[0], x=ins[1], x_scale=1.0, rest=tuple(ins[2:]), cR=1e-4, cB=1e-4, y_scale=1.0, kind=L1, y_=y._h, u_=u._h, sums_=sums):
        return close(y0, x, x_scale, *rest, cR, cB, y_scale, kind, y_, u_, sums_)

    def untouched2():
        return np.all(y.numpy(np.float32) == -7.0) and np.all(u.numpy(np.float32) == -7.0) and \
            all(np.array_equal(v.numpy(np.float32), h) for v, h in zip(dev, host)) and np.all(short.numpy(np.float32) == -7.0)
    for declined in (dict(cR=float("nan")), dict(cB=float("inf")), dict(x_scale=float("nan")), dict(y_scale=float("-inf")),
                     dict(kind=ITERS), dict(kind=-1), dict(kind=7)):
        assert call(**declined) == L.DECLINED and untouched2(), declined
    for bad in (dict(u_=short._h), dict(y_=short._h), dict(x=short._h), dict(rest=(short._h, *ins[3:])),
                dict(u_=y._h), dict(u_=ins[0]), dict(u_=ins[1]), dict(u_=ins[4]), dict(y_=ins[1]), dict(y_=ins[5]),
                dict(y0=None), dict(y_=None), dict(u_=None), dict(sums_=None), dict(rest=(None, *ins[3:]))):
        status = call(**bad)
        assert status not in (0, L.DECLINED) and untouched2(), bad
    assert list(sums) == [-1.0] * 5
    assert call() == 0 and not untouched2()                                               # the same arguments, nothing refused


def _shifted(pg, values):
    """`values` in device memory that is NOT 16-byte aligned: a view one element into a buffer of len(values) + 1."""
    whole = pg.DeviceVector.from_host(np.concatenate([np.float32([-7.0]), np.float32(values)]))
    return pg.DeviceVector.wrap(whole.ptr + 4, len(values), keepalive=whole)


@pytest.mark.parametrize("n", [65, 4099])
def test_operands_that_are_not_16_byte_aligned(gpu_engine, n):
    """One misaligned operand or output sends every element down the one-per-lane path: the same stores, bit for bit, as the 16-byte
    path gives on aligned copies, and sums within the bound (another order of addition)."""
    pg = gpu_engine
    setup, close = _entries()
    rng = np.random.default_rng(77 + n)
    host = _setup_operands(rng, n, False, False, 0.2)
    aligned = [pg.DeviceVector.from_host(v) for v in host]
    outs = [pg.DeviceVector.full(n, -7.0) for _ in range(5)]
    sums = (C.c_double * 2)()
    assert setup(*[v._h for v in aligned], 0.2, *[v._h for v in outs], sums) == 0
    want = [v.numpy(np.float32) for v in outs]
    for which in ("input", "output", "all"):
        ins = [_shifted(pg, v) if which == "all" or (which == "input" and k == 1) else pg.DeviceVector.from_host(v) for k, v in enumerate(host)]
        made = [_shifted(pg, np.full(n, -7.0)) if which == "all" or (which == "output" and k == 2) else pg.DeviceVector.full(n, -7.0)
                for k in range(5)]
        assert which == "input" or made[2].ptr % 16 != 0
        sums2 = (C.c_double * 2)()
        assert setup(*[v._h for v in ins], 0.2, *[v._h for v in made], sums2) == 0, which
        for a, b in zip(want, made):
            assert np.array_equal(a, b.numpy(np.float32)), which
        _sums_agree(list(sums2), list(sums), which)
        for v in made:
            if v._keepalive is not None:
                assert v._keepalive.numpy(np.float32)[0] == -7.0          # the element in front of the view
    host = _close_operands(rng, n, True)
    dev = [pg.DeviceVector.from_host(v) for v in host]
    y, u = pg.DeviceVector.full(n, -7.0), pg.DeviceVector.full(n, -7.0)
    sums = (C.c_double * 5)()
    assert close(dev[0]._h, dev[1]._h, 1.25, *[v._h for v in dev[2:]], 3e-4, 7e-4, 1.07, L1, y._h, u._h, sums) == 0
    for which in ("input", "output", "all"):
        ins = [_shifted(pg, v) if which == "all" or (which == "input" and k == 4) else pg.DeviceVector.from_host(v) for k, v in enumerate(host)]
        y2 = _shifted(pg, np.full(n, -7.0)) if which != "input" else pg.DeviceVector.full(n, -7.0)
        u2 = _shifted(pg, np.full(n, -7.0)) if which == "all" else pg.DeviceVector.full(n, -7.0)
        sums2 = (C.c_double * 5)()
        assert close(ins[0]._h, ins[1]._h, 1.25, *[v._h for v in ins[2:]], 3e-4, 7e-4, 1.07, L1, y2._h, u2._h, sums2) == 0, which
        assert np.array_equal(y.numpy(np.float32), y2.numpy(np.float32)) and np.array_equal(u.numpy(np.float32), u2.numpy(np.float32)), which
        _sums_agree(list(sums2), list(sums), which)
