"""include/pgh_rank.h on the GPU against a numpy f64 restatement written in tests/rank_common.py (stable order from np.lexsort, mid-ranks
from tie-group counts, -0.0 canonicalised): pgh_ndcg on its streaming and its sorted route, pgh_spearman, and the vector entries.

The bounds are those of rank_common's docstring: DCG relative max(T, 4) * 2^-50 with T = min(k, relevant rows) terms, rho absolute
n' * 2^-50.  The shapes are the smallest at which the kernels can go wrong: sizes around the wavefront (63, 64, 65), more than one
workgroup (257, 4097), more rows than one pass of the fixed parts holds (70 001 > 256 * 256), 1, 2, 63 and 64 columns, the two sides
of the LDS threshold of the streaming kernel (8 * b * relevant <= 61 440 bytes: 120 and 121 relevant rows at 64 columns) and of its
limit (8192 and 8193 relevant rows)."""
import numpy as np
import pytest

import rank_common as rc

pytestmark = pytest.mark.gpu


def _graded(rng, n, share):
    """Known scores in {0, 0.25, 0.5, 1}: about `share` of the rows relevant, with ties."""
    return np.where(rng.random(n) < share, rng.choice([0.25, 0.5, 1.0], n), 0.0)


def _scores(rng, n, b):
    """f32 scores: continuous columns, columns on a grid of eighths (many ties), and a constant one."""
    host = rc.f32(rng.random((n, b)))
    host[:, ::3] = np.round(host[:, ::3] * 8) / 8
    if b > 2:
        host[:, 2] = 0.5
    return host


def _ks(n, kept, relevant):
    return sorted({k for k in (1, kept, kept + 1, n, relevant) if k >= 1})


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 4097, 70001])
def test_ndcg_and_spearman_shapes(gpu_engine, n):
    rng = np.random.default_rng(n)
    known = _graded(rng, n, 0.1)
    known[rng.integers(n)] = 1.0
    exclude = (rng.random(n) < 0.2).astype(np.float64)
    exclude[int(np.flatnonzero(known)[0])] = 0                   # at least one relevant row is kept
    for b in (1, 2, 63, 64):
        host = _scores(rng, n, b)
        for ex in (None, exclude):
            keep = rc.kept_rows(n, ex)
            ks = _ks(n, int(keep.sum()), int((known[keep] != 0).sum()))
            rc.check_ndcg(gpu_engine, host, known, ex, ks if b in (1, 64) else ks[:2], label="shapes")
            rc.check_spearman(gpu_engine, host, known, ex, label="shapes")


def test_kept_rows_none_one_all(gpu_engine):
    pg = gpu_engine
    n = 257
    rng = np.random.default_rng(5)
    known, host = _graded(rng, n, 0.3), _scores(rng, n, 5)
    # nothing kept: every sum is empty
    plan = rc.Plan(pg, known, np.ones(n))
    assert (plan.kept, plan.relevant) == (0, 0)
    slab = pg.DeviceMatrix.from_host(host)
    for route in (rc.AUTO, rc.STREAMING, rc.SORTED):
        assert plan.ndcg(slab, 3, route) == (0, [0.0] * 5, 0.0)
    assert all(np.isnan(plan.spearman(slab)))
    # one kept row, relevant or not
    for row in (int(np.flatnonzero(known)[0]), int(np.flatnonzero(known == 0)[0])):
        only = np.ones(n)
        only[row] = 0
        rc.check_ndcg(pg, host, known, only, [1, 2, n], label="one kept")
        assert all(np.isnan(rc.check_spearman(pg, host, known, only, label="one kept")))
    rc.check_ndcg(pg, host, known, np.zeros(n), [1, n], label="all kept")
    rc.check_ndcg(pg, host, known, None, [1, n], label="no exclude")


@pytest.mark.parametrize("relevant", [0, 1, 120, 121, 8192, 8193])
def test_relevant_row_counts(gpu_engine, relevant):
    pg = gpu_engine
    n, b = 70001, 64
    rng = np.random.default_rng(relevant)
    rows = rng.choice(np.arange(1, n - 1), max(relevant - 2, 0), replace=False)
    known = np.zeros(n)
    known[rows] = rng.choice([0.25, 0.5, 1.0], len(rows))
    if relevant >= 1:
        known[0] = 0.5                                            # a relevant row first ...
    if relevant >= 2:
        known[n - 1] = 1.0                                        # ... and last in row order
    exclude = (rng.random(n) < 0.1).astype(np.float64)
    exclude[known != 0] = 0
    extra = rng.choice(np.flatnonzero(known == 0), 50, replace=False)
    known_more = known.copy()
    known_more[extra] = 1.0                                       # relevant rows that are excluded do not count
    exclude[extra] = 1
    host = _scores(rng, n, b)
    ks = [1, 10, max(relevant, 1), n]
    if relevant <= rc.MAX_RELEVANT:
        plan = rc.check_ndcg(pg, host, known_more, exclude, ks, label="relevant")
        assert plan.relevant == relevant
        return
    plan = rc.check_ndcg(pg, host, known_more, exclude, ks, routes=(rc.SORTED, rc.AUTO), label="relevant")
    assert plan.relevant == relevant
    slab = pg.DeviceMatrix.from_host(host)
    status, values, ideal = plan.ndcg(slab, 10, rc.STREAMING)
    assert status == rc.DECLINED and values == [-7.0] * b and ideal == -7.0       # nothing written
    assert plan.ndcg(slab, 10, rc.AUTO) == plan.ndcg(slab, 10, rc.SORTED)


def test_ties_and_special_scores(gpu_engine):
    pg = gpu_engine
    n = 4097
    rng = np.random.default_rng(11)
    known = _graded(rng, n, 0.05)
    relevant = np.flatnonzero(known)
    tiny = float(np.float32(1e-45))                               # the smallest f32 denormal
    columns = []
    columns.append(np.full(n, 0.25))                              # all scores equal: the order is the row order
    straddle = rc.f32(rng.random(n))
    straddle[rng.choice(n, n // 2, replace=False)] = 0.75         # a tie group of n / 2 rows: position k falls inside it for the ks below
    columns.append(straddle)
    tied = np.round(rc.f32(rng.random(n)) * 4) / 4                # five values: relevant rows tie with each other and with their
    columns.append(tied)                                          # neighbours on both sides in row order
    zeros = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    zeros[relevant[::2]] = -0.0
    zeros[relevant[1::2]] = 0.0
    columns.append(zeros)                                         # -0.0 and +0.0 are ONE tie group
    mixed = zeros.copy()
    mixed[rng.choice(n, n // 3, replace=False)] = 1.0
    mixed[rng.choice(n, n // 3, replace=False)] = -1.0
    columns.append(mixed)
    columns.append(-rc.f32(rng.random(n)))                        # negative scores
    columns.append(rng.choice([0.0, tiny, 2 * tiny, -tiny, 1e-38], n))     # denormals
    columns.append(rng.choice([-np.inf, np.inf, 0.0, 1.0, -1.0], n))       # infinities are ordinary scores
    host = rc.f32(np.stack(columns, axis=1))
    assert np.signbit(host[:, 3]).any() and not np.signbit(host[:, 3]).all() and (np.abs(host[:, 6]) == tiny).any()
    exclude = (rng.random(n) < 0.2).astype(np.float64)
    for ex in (None, exclude):
        keep = rc.kept_rows(n, ex)
        kept, rel = int(keep.sum()), int((known[keep] != 0).sum())
        rc.check_ndcg(pg, host, known, ex, [1, rel, n // 3, kept, kept + 1, n], label="ties")
        rc.check_spearman(pg, host, known, ex, label="ties")


def test_one_nan_spoils_one_column(gpu_engine):
    pg = gpu_engine
    n, b = 257, 5
    rng = np.random.default_rng(13)
    known, host = _graded(rng, n, 0.2), _scores(rng, n, b)
    exclude = np.zeros(n)
    exclude[7] = 1
    host[100, 3] = np.nan
    host[7, 1] = np.nan                                           # in an excluded row: not a score of the column
    rc.check_ndcg(pg, host, known, exclude, [1, 10, n], label="nan")
    got = rc.check_spearman(pg, host, known, exclude, label="nan")
    assert [bool(np.isnan(v)) for v in got] == [False, False, True, True, False]       # column 2 is constant, column 3 holds the NaN
    status, values, _ = rc.Plan(pg, known, exclude).ndcg(pg.DeviceMatrix.from_host(host), 10, rc.STREAMING)
    assert status == 0 and [bool(np.isnan(v)) for v in values] == [False, False, False, True, False]


def test_negative_known_score(gpu_engine):
    pg = gpu_engine
    n, b = 4097, 3
    rng = np.random.default_rng(17)
    known, host = _graded(rng, n, 0.1), _scores(rng, n, b)
    known[rng.choice(n, 20, replace=False)] = -0.5
    plan = rc.check_ndcg(pg, host, known, None, [1, 10, n], routes=(rc.SORTED, rc.AUTO), label="negative")
    assert plan.negative == 1
    status, values, ideal = plan.ndcg(pg.DeviceMatrix.from_host(host), 10, rc.STREAMING)
    assert status == rc.DECLINED and values == [-7.0] * b and ideal == -7.0
    # an excluded negative known score does not count
    exclude = (known < 0).astype(np.float64)
    assert rc.check_ndcg(pg, host, known, exclude, [10], label="negative excluded").negative == 0


def test_vector_entries_are_the_one_column_case(gpu_engine):
    pg = gpu_engine
    n = 4097
    rng = np.random.default_rng(19)
    known, host = _graded(rng, n, 0.1), _scores(rng, n, 4)
    exclude = (rng.random(n) < 0.2).astype(np.float64)
    plan = rc.Plan(pg, known, exclude)
    slab = pg.DeviceMatrix.from_host(host)
    many = plan.spearman(slab)
    for route in (rc.STREAMING, rc.SORTED):
        status, wide, ideal = plan.ndcg(slab, 25, route)
        assert status == 0
        for j in range(4):
            vector = pg.DeviceVector.from_host(host[:, j])
            assert plan.ndcg(vector, 25, route) == (0, [wide[j]], ideal)
            assert plan.ndcg(pg.DeviceMatrix.from_host(host[:, j:j + 1]), 25, route) == (0, [wide[j]], ideal)
            assert rc.same(plan.spearman(vector)[0], many[j])


def test_spearman_special_cases(gpu_engine):
    pg = gpu_engine
    n = 4097
    rng = np.random.default_rng(23)
    known = rc.f32(rng.random(n))                                 # distinct with overwhelming probability; ties are handled anyway
    exclude = (rng.random(n) < 0.2).astype(np.float64)
    heavy = np.round(known * 3) / 3
    host = rc.f32(np.stack([np.full(n, 2.0), known * 0.5, -known, np.round(rc.f32(rng.random(n)) * 2) / 2, rc.f32(rng.random(n))], axis=1))
    for ex in (None, exclude):
        got = rc.check_spearman(pg, host, known, ex, label="special")
        kept = int(rc.kept_rows(n, ex).sum())
        assert np.isnan(got[0])                                   # a constant column
        assert abs(got[1] - 1) <= rc.rho_bound(kept) and abs(got[2] + 1) <= rc.rho_bound(kept)      # monotone: +-1
        assert all(np.isnan(rc.check_spearman(pg, host, np.full(n, 0.5), ex, label="constant known")))
        rc.check_spearman(pg, host, heavy, ex, label="heavy ties")


def test_bad_arguments(gpu_engine):
    pg = gpu_engine
    from pygrank_amd import _lib as L
    plan = rc.Plan(pg, np.ones(10))
    slab = pg.DeviceMatrix.from_host(np.ones((10, 2)))
    for k, route in ((0, rc.AUTO), (3, 5)):
        with pytest.raises(L.EngineError):
            plan.ndcg(slab, k, route)
    with pytest.raises(L.EngineError, match="rows differ"):
        plan.ndcg(pg.DeviceMatrix.from_host(np.ones((9, 2))), 3, rc.AUTO)
    wide = pg.DeviceMatrix.from_host(np.ones((10, 65)))
    assert plan.ndcg(wide, 3, rc.AUTO)[0] == rc.DECLINED
    with pytest.raises(L.EngineError, match="differ in length"):
        rc.Plan(pg, np.ones(10), np.ones(9))
