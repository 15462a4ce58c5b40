"""The fairness postprocessors on the host test double (no GPU) against the reference's recorded behaviour
(tests/golden/golden_fairness.json).  The double lacks include/pgh_fair.h, so FairPersonalizer's `many` builds its columns one candidate
at a time here and still ranks and scores them together.

The end-to-end condition is checked on weighted300 and rmat10_dir.  The fixture's generator drops the descent case of er10k: the
reference's own descent improves its loss by 0.0075 there on each of the 8 sensitive draws tried, short of the 0.05 a case needs."""
import pytest

import fairness_common as fc


@pytest.fixture(scope="module")
def fx():
    return fc.fixture()


def test_many_without_the_entry_equals_the_loop(host_engine, fx):
    from pygrank_amd import _lib as L
    assert L.entry("pgh_prior_edit") is None
    case = fc.Case(host_engine, fx, "weighted300")
    personalizer = case.personalizer(fx, max_residual=1)
    loss = case.open(personalizer)
    try:
        assert callable(getattr(loss, "many", None))
        for step in fc.first_steps(1, 1):
            many = loss.many(step)
            singles = [loss(w) for w in step]
            for w, a, b in zip(step, many, singles):
                bound, host = fc.loss_bound(loss, w, 2 * fc.sc.TOL)
                assert abs(a - b) <= bound and abs(a - host) <= bound, (w, a, b, host, bound)
    finally:
        loss.close()
    assert personalizer.last_fit["edit_kernel_steps"] == 0 and personalizer.last_fit["batched_steps"] == 5
    off = case.personalizer(fx, batch=False)
    loss = case.open(off)
    try:
        assert not hasattr(loss, "many")
    finally:
        loss.close()


def test_points_against_the_reference(host_engine, fx):
    fc.check_points(fc.Case(host_engine, fx, "weighted300"), fx)


@pytest.mark.parametrize("batch", [True, False])
@pytest.mark.parametrize("key", fc.DESCENTS)
def test_descent_meets_the_end_to_end_condition(host_engine, fx, key, batch):
    case = fc.Case(host_engine, fx, key)
    personalizer = case.personalizer(fx, batch=batch)
    ranks = fc.check_descent(case, fx, personalizer)
    assert isinstance(ranks, host_engine.GraphSignal)
    fit = personalizer.last_fit
    assert fit["edit_kernel_steps"] == 0
    assert (fit["batched_steps"] > 0) == batch and (fit["single_steps"] > 1) == (not batch)


def test_convergence_manager_comes_back(host_engine, fx):
    pg = host_engine
    case = fc.Case(pg, fx, "weighted300")

    class Failing(pg.Postprocessor):
        """Passes everything to the wrapped ranker and raises on the third rank()."""
        calls = 0

        def rank(self, *args, **kwargs):
            self.calls += 1
            if self.calls == 3:
                raise RuntimeError("third call")
            return self.ranker.rank(*args, **kwargs)

    for batch in (True, False):
        inner = pg.PageRank(**fx["pagerank"])
        manager = inner.convergence
        failing = Failing(inner)
        personalizer = pg.FairPersonalizer(failing, verbose=False, batch=batch, **fx["fair"])
        with pytest.raises(RuntimeError, match="third call"):
            personalizer.rank(case.graph, case.seeds, case.sensitive)
        assert failing.calls == 3 and inner.convergence is manager
    healthy = case.personalizer(fx)
    manager = healthy.ranker.convergence
    healthy.rank(case.graph, case.seeds, case.sensitive)
    assert healthy.ranker.convergence is manager


def test_refusals(host_engine, fx):
    pg = host_engine
    case = fc.Case(pg, fx, "weighted300")
    for parity in ("TPR", "TNR", "mistreatment"):
        with pytest.raises(NotImplementedError, match="Mistreatment"):
            pg.FairPersonalizer(pg.PageRank(), parity_type=parity).rank(case.graph, case.seeds, case.sensitive)
    with pytest.raises(Exception, match="Invalid parity type"):
        pg.FairPersonalizer(pg.PageRank(), parity_type="parity").rank(case.graph, case.seeds, case.sensitive)
    ranks = pg.PageRank().rank(case.graph, case.seeds)
    for method in ("O", "LFPRO"):
        with pytest.raises(NotImplementedError):
            pg.AdHocFairness(method).transform(ranks, sensitive=case.sensitive)
    with pytest.raises(Exception, match="Invalid fairness postprocessing method") as caught:
        pg.AdHocFairness("X").transform(ranks, sensitive=case.sensitive)
    assert not isinstance(caught.value, NotImplementedError)
    u = pg.FairPersonalizer(pg.PageRank(**fx["pagerank"]), parity_type="U", verbose=False, **fx["fair"])
    loss = case.open(u)
    try:
        assert isinstance(loss.fairness_measure, pg.MannWhitneyParity)
        import math
        got = loss.many(fc.first_steps(1, 0)[2])
        assert len(got) == 10 and all(math.isfinite(value) for value in got)
    finally:
        loss.close()


def test_adhoc_argument_swap(host_engine):
    pg = host_engine
    ranker = pg.PageRank()
    for built in (pg.AdHocFairness(ranker, "B"), pg.AdHocFairness("B", ranker)):
        assert built.ranker is ranker and built.method == "B"
    alone = pg.AdHocFairness("mult")
    assert isinstance(alone.ranker, pg.Tautology) and alone.method == "mult"
    default = pg.AdHocFairness()
    assert isinstance(default.ranker, pg.Tautology) and default.method == "B"
    swapped = pg.AdHocFairness("mult", "B")              # neither is a ranker: fairness.py:168-171 swaps, then drops the non-ranker
    assert isinstance(swapped.ranker, pg.Tautology) and swapped.method == "mult"


@pytest.mark.parametrize("key", fc.GRAPHS)
def test_adhoc_b_matches_the_fixture(host_engine, fx, key):
    fc.check_adhoc(fc.Case(host_engine, fx, key))
