"""The bounds of tests/f64_common.py bite: deliberately wrong "engine outputs", made in numpy, are rejected by the check they belong
to, and correct f64 results summed in other orders are accepted -- the bound belongs to the arithmetic, not to one summation order.
No engine is involved."""
import numpy as np
import pytest
import scipy.sparse as sp

import f64_common as fc

ALPHA = 0.85


@pytest.fixture(scope="module")
def setting():
    """The two-sided value-free image of the 3 001-node graph with multiplicities (its effective entries right_i * m * left_j are no
    f32 numbers), a positive warm start and the probe's personalization."""
    rng = np.random.default_rng(3)
    W, iso = fc.small_graph(rng, "mult")
    out_w, in_w = np.asarray(W.sum(axis=1)).ravel(), np.asarray(W.sum(axis=0)).ravel()
    op = fc.effective_matrix(W, fc.f32_inverse(out_w, 0.5), fc.f32_inverse(in_w, 0.5))
    ins = fc.inputs(rng, op.n)
    x = ins["positive"]
    p = fc.cancellation_probe(op, x, ALPHA)
    return dict(op=op, iso=iso, x=x, p=p, decades=ins["decades"])


def _probe_output(row_sums, p):
    """The step's f32 output from f64 row sums."""
    return (ALPHA * np.asarray(row_sums, dtype=np.float64) + (1.0 - ALPHA) * p.astype(np.float64)).astype(fc.F32).astype(np.float64)


def _probe_ratio(setting, got, cold):
    ref = fc.recursive_reference(setting["op"], setting["p"], setting["x"], 1, alpha=ALPHA, cold=cold)
    return ref["out"].verdict(got)[1]


def _ordered_row_sums(op, x, order):
    MT, x = op.MT, np.asarray(x, dtype=np.float64)
    out = np.zeros(op.n)
    for i in range(op.n):
        lo, hi = MT.indptr[i], MT.indptr[i + 1]
        prods = MT.data[lo:hi] * x[MT.indices[lo:hi]]
        if hi == lo:
            continue
        if order == "forward":
            out[i] = np.cumsum(prods)[-1]                   # strictly sequential
        elif order == "reversed":
            out[i] = np.cumsum(prods[::-1])[-1]
        else:
            out[i] = np.add.reduce(prods)                    # numpy's pairwise blocks
    return out


@pytest.mark.parametrize("order", ["forward", "reversed", "pairwise"])
def test_probe_accepts_f64_sums_in_any_order(setting, order):
    got = _probe_output(_ordered_row_sums(setting["op"], setting["x"], order), setting["p"])
    ratio = _probe_ratio(setting, got, cold=False)          # the stricter bound: no fixed-point term
    assert ratio.max() <= 1.0, (order, float(ratio.max()))


def test_probe_rejects_row_sums_accumulated_in_f32(setting):
    op = setting["op"]
    sums32 = sp.csr_array(op.MT.astype(fc.F32)) @ setting["x"].astype(fc.F32)
    assert sums32.dtype == fc.F32
    ratio = _probe_ratio(setting, _probe_output(sums32, setting["p"]), cold=True)
    live = np.diff(op.MT.indptr) > 0
    assert np.count_nonzero(ratio[live] > 1.0) > 0.9 * np.count_nonzero(live), float(np.median(ratio[live]))


def test_probe_rejects_one_entry_rounded_to_f32(setting):
    op = setting["op"]
    MT = op.MT.copy()
    counts = np.diff(MT.indptr)
    row = int(np.flatnonzero(counts >= 3)[7])
    at = MT.indptr[row] + 1
    assert not fc.is_f32(MT.data[at])
    MT.data[at] = float(fc.F32(MT.data[at]))
    sums = fc.matvec_ld(MT, setting["x"]).astype(np.float64)
    ratio = _probe_ratio(setting, _probe_output(sums, setting["p"]), cold=True)
    assert ratio[row] > 1.0 and np.all(np.delete(ratio, row) <= 1.0), float(ratio[row])


def test_probe_rejects_a_dropped_smallest_cold_entry(setting):
    op = setting["op"]
    MT = op.MT.copy()
    row = int(np.argmax(np.diff(MT.indptr)))                # a hub row: ~1 000 entries, nearly all of them cold under PGH_HOT64=32
    lo, hi = MT.indptr[row], MT.indptr[row + 1]
    share = np.abs(MT.data[lo:hi] * setting["x"][MT.indices[lo:hi]])
    MT.data[lo + int(np.argmin(share))] = 0.0
    assert share.min() < 2e-3 * share.sum()
    sums = fc.matvec_ld(MT, setting["x"]).astype(np.float64)
    ratio = _probe_ratio(setting, _probe_output(sums, setting["p"]), cold=True)
    assert ratio[row] > 1.0 and np.all(np.delete(ratio, row) <= 1.0), float(ratio[row])


def test_probe_accepts_the_fixed_point_sums_of_the_cold_image(setting):
    op = setting["op"]
    sums = fc.fixed_point_rows(op, setting["x"], op.fixed_point_bits())
    ratio = _probe_ratio(setting, _probe_output(sums, setting["p"]), cold=True)
    assert ratio.max() <= 1.0, float(ratio.max())


def test_decades_product_tells_40_fixed_point_bits_from_51(setting):
    """T_2 of the input spread over 30 decades: rows far below the largest product see the quantum."""
    op, p = setting["op"], setting["decades"]
    want = fc.step(op, fc.Vec(p.astype(np.float64)), 1.0, cold=True)
    assert op.fixed_point_bits() == 51
    good = fc.fixed_point_rows(op, p, 51).astype(fc.F32).astype(np.float64)
    assert want.verdict(good)[1].max() <= 1.0
    bad = fc.fixed_point_rows(op, p, 40).astype(fc.F32).astype(np.float64)
    ratio = want.verdict(bad)[1]
    assert np.count_nonzero(ratio > 1.0) > 100, int(np.count_nonzero(ratio > 1.0))


def test_isolated_check_rejects_a_kept_warm_start(setting):
    iso = setting["iso"]
    got = np.zeros(setting["op"].n)
    assert fc.rows_exactly_zero(got, iso)
    got[iso[len(iso) // 2]] = 3.0
    assert not fc.rows_exactly_zero(got, iso)
    got[iso[len(iso) // 2]] = -0.0
    assert not fc.rows_exactly_zero(got, iso)
