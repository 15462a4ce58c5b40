"""The fairness postprocessors on the GPU, on the graphs of tests/golden/golden_fairness.json: FairPersonalizer's two routes against
each other and against the reference's recorded losses, a full run, and AdHocFairness("B").

Bounds (tests/fairness_common.py, no new constant): the ranks of a batch column against its single-vector run, and of an engine run
against the reference, are held to 1e-6 relative L-inf (tests/test_gpu_batch_edges.py BOUND, tests/parity_common.py REL_TOL); pRule and
Mabs to 16 * 2^-24 relative against recorded values and to twice that between the slab and the columns route
(tests/supervised_common.py TOL, tests/test_gpu_supervised.py).  fairness_common.loss_bound carries the rank bound through the two
measures and scales the two terms by the loss's weights.

The generator drops the descent case of er10k (see tests/test_fairness_host.py); the full run is checked on weighted300 and rmat10_dir."""
import pytest

import fairness_common as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return fc.fixture()


@pytest.fixture(scope="module")
def all_cases(gpu_engine, fx):
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = fc.Case(gpu_engine, fx, key)
        return cache[key]
    return get


@pytest.mark.parametrize("key", fc.GRAPHS)
def test_routes_agree(gpu_engine, fx, all_cases, key):
    from pygrank_amd import _lib as L
    assert L.entry("pgh_prior_edit") is not None
    case = all_cases(key)
    largest = 0.0
    for buckets, skew in ((1, False), (2, True)):
        personalizer = case.personalizer(fx, parameter_buckets=buckets, error_skewing=skew, max_residual=1)
        loss = case.open(personalizer)
        try:
            steps = fc.first_steps(buckets, 1)
            for step in steps:
                many = loss.many(step)
                singles = [loss(w) for w in step]
                for w, a, b in zip(step, many, singles):
                    bound, host = fc.loss_bound(loss, w, 2 * fc.sc.TOL)
                    largest = max(largest, abs(a - b))
                    assert abs(a - b) <= bound, (key, w, a, b, bound)
                    assert abs(a - host) <= bound and abs(b - host) <= bound, (key, w, a, b, host, bound)
        finally:
            loss.close()
        fit = personalizer.last_fit
        assert fit["batched_steps"] == fit["edit_kernel_steps"] == len(steps) and fit["single_steps"] == 10 * len(steps)
    print(f"{key}: largest |many - loss| {largest!r}")


@pytest.mark.parametrize("key", fc.GRAPHS)
def test_points_against_the_reference(gpu_engine, fx, all_cases, key):
    worst = fc.check_points(all_cases(key), fx)
    print(f"{key}: largest difference from the reference {worst:.3f} of its bound")


@pytest.mark.parametrize("key", fc.DESCENTS)
def test_full_run(gpu_engine, fx, all_cases, key):
    case = all_cases(key)
    personalizer = case.personalizer(fx)
    fc.check_descent(case, fx, personalizer)
    fit = personalizer.last_fit
    assert fit["batched_steps"] > 0 and fit["edit_kernel_steps"] == fit["batched_steps"]


@pytest.mark.parametrize("key", fc.GRAPHS)
def test_adhoc_b(gpu_engine, fx, all_cases, key):
    fc.check_adhoc(all_cases(key))
