"""The entries of include/pgh_link.h at the C-ABI on the GPU against the numpy restatement of tests/link_common.py.

Nothing here has a tolerance.  The scores are f32 values, so a product of two and a square of one are exact in f64; the row sums are
added in column order on both sides; division and square root are IEEE on both sides: the PREDICTIONS are compared bit for bit (a device
divide or square root that was not correctly rounded would show here).  The pair counts are integers: the AUC is compared with `==`
against two_wins / (2.0 * P * N).  pgh_link_factors is compared bit for bit after its one rounding to f32.

Shapes: rows 2 .. 70001 (one lane, one row tile, more than one tile, a grid-stride tail), columns 1, 2, 3 (a padded row tile), 63, 64,
65 and 130 (no 64-column limit, more than one column chunk, a chunk of 2), pairs 1 .. 2^20 + 1 (one lane, one workgroup, more than one
sort tile).  The largest case is 70001 rows x 130 columns with 2^20 + 1 pairs."""
import ctypes as C

import numpy as np
import pytest

import link_common as lc

pytestmark = pytest.mark.gpu

COS, DOT, DECLINED = 0, 1, 2
SIMILARITIES = [("cos", COS), ("dot", DOT)]
ROWS = [2, 63, 64, 65, 257, 4097, 70001]
COLUMNS = [1, 2, 3, 63, 64, 65, 130]
PAIRS = [1, 2, 255, 256, 257, 65537, 2 ** 20 + 1]
# every value of the three lists at least once, every column count on more than one row tile, and the largest of each together
SHAPES = [(2, 1, 1), (2, 2, 2), (63, 3, 255), (64, 63, 256), (65, 64, 257), (257, 65, 65537), (4097, 130, 255), (4097, 2, 2 ** 20 + 1),
          (70001, 3, 65537), (70001, 130, 2 ** 20 + 1)] + [(257, b, 257) for b in COLUMNS] + [(n, 3, 256) for n in ROWS]
SENTINEL = -7.0


def _entries():
    from pygrank_amd import _lib as L
    names = ["pgh_link_plan_create", "pgh_link_plan_info", "pgh_link_plan_destroy", "pgh_link_auc", "pgh_link_predictions", "pgh_link_factors"]
    entries = [L.entry(name) for name in names]
    assert all(entry is not None for entry in entries)
    return entries


def test_the_shapes_cover_every_listed_size():
    assert {s[0] for s in SHAPES} == set(ROWS) and {s[1] for s in SHAPES} == set(COLUMNS) and {s[2] for s in SHAPES} == set(PAIRS)
    assert (70001, 130, 2 ** 20 + 1) in SHAPES


def _scores(n, b, seed):
    rng = np.random.default_rng(seed)
    S = (rng.random((n, b)) - 0.5).astype(np.float32)
    S[rng.random((n, b)) < 0.25] = 0.0
    S[n // 2] = 0.0                                         # an all-zero row: safe_div
    return S


def _pairs(n, count, seed):
    rng = np.random.default_rng(seed)
    first = rng.integers(0, n, count).astype(np.int32)
    second = rng.integers(0, n, count).astype(np.int32)
    label = (rng.random(count) < 0.3).astype(np.uint8)
    if count >= 2:
        label[0], label[1] = 1, 0
    return first, second, label


class Plan:
    def __init__(self, n, first, second, label):
        create, _, self._destroy, _, _, _ = _entries()
        self.keep = [np.ascontiguousarray(first, dtype=np.int32), np.ascontiguousarray(second, dtype=np.int32),
                     np.ascontiguousarray(label, dtype=np.uint8)]
        self.h = C.c_void_p()
        status = create(n, len(self.keep[0]), self.keep[0].ctypes.data_as(C.POINTER(C.c_int32)), self.keep[1].ctypes.data_as(C.POINTER(C.c_int32)),
                        self.keep[2].ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(self.h))
        assert status == 0, status

    def close(self):
        assert self._destroy(self.h) == 0
        self.h = None


def _auc(matrix, plan, similarity):
    auc_fn = _entries()[3]
    auc, positive, negative = C.c_double(SENTINEL), C.c_int64(-1), C.c_int64(-1)
    status = auc_fn(matrix._h, plan.h, similarity, C.byref(auc), C.byref(positive), C.byref(negative))
    return status, auc.value, positive.value, negative.value


def _predictions(matrix, plan, similarity, first, count):
    out = np.full(count, SENTINEL, dtype=np.float64)
    status = _entries()[4](matrix._h, plan.h, similarity, first, count, out.ctypes.data_as(C.POINTER(C.c_double)))
    return status, out


def _free_bytes():
    from pygrank_amd import _lib as L
    free, total = C.c_int64(), C.c_int64()
    assert L.lib().pgh_mem_info(C.byref(free), C.byref(total)) == 0
    return free.value


def _bits(values):
    return np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n,b,count", SHAPES)
def test_predictions_auc_and_factors(gpu_engine, n, b, count):
    pg = gpu_engine
    S = _scores(n, b, 31 * n + b)
    matrix = pg.DeviceMatrix.from_host(S.astype(np.float64))
    assert np.array_equal(matrix.numpy(), S.astype(np.float64))
    first, second, label = _pairs(n, count, count + n)
    plan = Plan(n, first, second, label)
    info = [C.c_int64(), C.c_int64(), C.c_int64()]
    assert _entries()[1](plan.h, *[C.byref(v) for v in info]) == 0
    assert [v.value for v in info] == [n, count, int(label.sum())]
    for name, similarity in SIMILARITIES:
        want = lc.predictions(S.astype(np.float64), first, second, name)
        status, got = _predictions(matrix, plan, similarity, 0, count)
        assert status == 0
        different = np.flatnonzero(_bits(got) != _bits(want))
        print(f"n {n} b {b} pairs {count} {name}: predictions that differ in a bit: {len(different)}")
        assert len(different) == 0, (name, different[:5], got[different[:5]], want[different[:5]])
        if count > 3:                                       # a range inside the plan
            status, part = _predictions(matrix, plan, similarity, 1, count - 3)
            assert status == 0 and np.array_equal(_bits(part), _bits(want[1:count - 2]))
        wins, P, N = lc.two_wins(want, label)
        status, auc, positive, negative = _auc(matrix, plan, similarity)
        assert status == 0 and (positive, negative) == (P, N)
        if P == 0 or N == 0:
            assert auc != auc                               # the counts returned, no AUC
            continue
        assert auc == wins / (2.0 * P * N), (name, auc, wins, P, N)
        free = _free_bytes()
        again = _auc(matrix, plan, similarity)
        assert again == (0, auc, P, N)                      # the same bits ...
        assert _free_bytes() == free                        # ... and nothing allocated
        # the factors, rounded once to f32
        t = pg.DeviceVector.full(n, SENTINEL)
        assert _entries()[5](matrix._h, similarity, t._h) == 0
        assert np.array_equal(t.numpy(np.float32).view(np.uint32), lc.factors(S.astype(np.float64), name).astype(np.float32).view(np.uint32))
    plan.close()


def test_ties(gpu_engine):
    pg = gpu_engine
    n, count = 300, 1000
    first, second, label = _pairs(n, count, 5)
    plan = Plan(n, first, second, label)
    zeros = pg.DeviceMatrix.from_host(np.zeros((n, 4)))
    constant = pg.DeviceMatrix.from_host(np.full((n, 1), 0.5))          # one group: cos is 1 for every pair up to rounding, dot 0.25
    for _, similarity in SIMILARITIES:
        assert _auc(zeros, plan, similarity)[:2] == (0, 0.5)            # a slab of zeros: every prediction 0
        status, auc, _, _ = _auc(constant, plan, similarity)
        assert status == 0 and auc == 0.5                               # all predictions equal
    plan.close()
    # -0.0 against +0.0: (-1) * 0 and 1 * 0 under "dot" are one score
    signed = pg.DeviceMatrix.from_host(np.array([[-1.0], [1.0], [0.0]]))
    plan = Plan(3, [0, 1], [2, 2], [1, 0])
    status, got = _predictions(signed, plan, DOT, 0, 2)
    assert status == 0 and np.array_equal(_bits(got), _bits([-0.0, 0.0]))
    assert _auc(signed, plan, DOT)[:2] == (0, 0.5)
    plan.close()
    plan = Plan(3, [0, 1], [2, 2], [0, 1])
    assert _auc(signed, plan, DOT)[:2] == (0, 0.5)
    plan.close()
    # a strict order, both ways round
    ordered = pg.DeviceMatrix.from_host(np.array([[1.0], [2.0], [3.0]]))
    plan = Plan(3, [0, 1], [2, 2], [0, 1])                                # predictions 3 (negative) < 6 (positive)
    assert _auc(ordered, plan, DOT)[:2] == (0, 1.0)
    plan.close()
    plan = Plan(3, [0, 1], [2, 2], [1, 0])
    assert _auc(ordered, plan, DOT)[:2] == (0, 0.0)
    plan.close()


def test_edge_inputs(gpu_engine):
    pg = gpu_engine
    n = 100
    S = _scores(n, 3, 1)
    matrix = pg.DeviceMatrix.from_host(S.astype(np.float64))
    first, second, _ = _pairs(n, 50, 2)
    for label, counts in ((np.ones(50, dtype=np.uint8), (50, 0)), (np.zeros(50, dtype=np.uint8), (0, 50))):
        plan = Plan(n, first, second, label)
        status, auc, positive, negative = _auc(matrix, plan, COS)
        assert status == 0 and auc != auc and (positive, negative) == counts
        plan.close()
    plan = Plan(n, [], [], [])                                           # no pairs at all
    assert _auc(matrix, plan, COS)[0] == 0 and _auc(matrix, plan, COS)[2:] == (0, 0)
    assert _predictions(matrix, plan, COS, 0, 0)[0] == 0
    plan.close()
    # an infinite score in the last column: inf / inf under "cos", whatever the partner holds
    S[5, 2] = np.inf
    first[0], second[0] = 5, 6
    label = np.arange(50, dtype=np.uint8) % 2
    plan = Plan(n, first, second, label)
    infinite = pg.DeviceMatrix.from_host(S.astype(np.float64))
    status, auc, positive, negative = _auc(infinite, plan, COS)
    assert status == 0 and auc != auc and (positive, negative) == (25, 25)
    status, got = _predictions(infinite, plan, COS, 0, 50)
    assert status == 0 and np.isnan(got[0])
    assert np.array_equal(np.isnan(got), np.isnan(lc.predictions(S.astype(np.float64), first, second, "cos")))
    plan.close()


def test_refusals_write_nothing(gpu_engine):
    from pygrank_amd import _lib as L
    pg = gpu_engine
    create = _entries()[0]
    n = 64
    matrix = pg.DeviceMatrix.from_host(_scores(n, 3, 3).astype(np.float64))
    first, second, label = _pairs(n, 10, 4)
    plan = Plan(n, first, second, label)
    other = pg.DeviceMatrix.from_host(_scores(n + 1, 3, 3).astype(np.float64))
    status, auc, positive, negative = _auc(other, plan, COS)              # a slab with the wrong row count
    assert status not in (0, DECLINED) and (auc, positive, negative) == (SENTINEL, -1, -1)
    assert b"rows" in L.lib().pgh_last_error()
    status, got = _predictions(other, plan, COS, 0, 10)
    assert status not in (0, DECLINED) and np.all(got == SENTINEL)
    assert _auc(matrix, plan, 2)[0] not in (0, DECLINED)                  # an unknown similarity
    assert _predictions(matrix, plan, COS, 5, 6)[0] not in (0, DECLINED)  # a range that leaves the plan
    short = pg.DeviceVector.full(n - 1, SENTINEL)
    assert _entries()[5](matrix._h, COS, short._h) not in (0, DECLINED) and np.all(short.numpy() == SENTINEL)
    plan.close()

    def refused(rows, count, a, b, c):
        handle = C.c_void_p(12345)
        a, b, c = np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.int32), np.asarray(c, dtype=np.uint8)
        status = create(rows, count, a.ctypes.data_as(C.POINTER(C.c_int32)), b.ctypes.data_as(C.POINTER(C.c_int32)),
                        c.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(handle))
        assert status not in (0, DECLINED) and handle.value == 12345
        return L.lib().pgh_last_error()
    assert b"outside" in refused(n, 2, [0, n], [1, 1], [1, 0])            # a pair id >= n
    assert b"outside" in refused(n, 2, [0, 1], [1, -1], [1, 0])
    # 2^27 + 1 pairs: refused by the argument check alone, before a single element is read (the arrays hold two)
    free = _free_bytes()
    assert b"PGH_LINK_MAX_PAIRS" in refused(n, 2 ** 27 + 1, [0, 1], [1, 0], [1, 0])
    assert _free_bytes() == free
