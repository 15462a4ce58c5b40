"""The references and bounds of tests/f64_common.py exercised against the host double (oracle/host_abi.cpp iterates in double over the
stored f32 matrix): items 1 to 9 of tests/test_gpu_f64_kernels.py without a GPU.  The layout switches are inert here and format() has
no premise to check; the reference matrix is download_transposed()."""
import numpy as np
import pytest
import scipy.sparse as sp

import f64_common as fc


@pytest.fixture()
def calls(host_engine):
    return fc.Calls(host_engine)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    fc.print_report("f64 step checks on the host double: worst |error| / bound")


@pytest.mark.parametrize("weights,kind", [("unit", "col"), ("mult", "two-sided"), ("real", "valued"), ("mult", "col")])
def test_host_double_full_battery(calls, weights, kind):
    W, iso = fc.small_graph(np.random.default_rng(3), weights)
    g, _ = fc.upload(calls.pg, W, kind)
    fc.full_battery(calls, g, fc.stored_operator(g), "host %s %s" % (weights, kind), False, iso, 17)


@pytest.mark.parametrize("weights", ["unit", "mult"])
def test_host_double_exact_integers(calls, weights):
    W, _ = fc.small_graph(np.random.default_rng(3), weights)
    g, op = fc.upload(calls.pg, W, "none")
    stored = fc.stored_operator(g)
    assert np.array_equal(stored.MT.toarray(), op.MT.toarray())
    fc.check_exact(calls, g, op, "host none " + weights, np.random.default_rng(5))


def test_host_double_chain_graph(calls):
    W, iso = fc.chain_graph(np.random.default_rng(9))
    g, _ = fc.upload(calls.pg, W, "col")
    op = fc.stored_operator(g)
    rng = np.random.default_rng(21)
    fc.check_products(calls, g, op, "host chain", False, rng)
    fc.check_probe(calls, g, op, "host chain", False, rng)
    fc.check_isolated(calls, g, op, "host chain", iso, rng)


def test_host_double_isolated_tail_graph(calls):
    W, iso = fc.iso_tail_graph(np.random.default_rng(13))
    g, _ = fc.upload(calls.pg, W, "col")
    op = fc.stored_operator(g)
    rng = np.random.default_rng(23)
    fc.check_products(calls, g, op, "host isolated tail", False, rng)
    fc.check_isolated(calls, g, op, "host isolated tail", iso, rng)


@pytest.mark.parametrize("name", ["loop1", "edge2", "ring65"])
def test_host_double_tiny_graphs(calls, name):
    W = fc.tiny_graphs()[name]
    g, _ = fc.upload(calls.pg, W, "col")
    op = fc.stored_operator(g)
    rng = np.random.default_rng(2)
    fc.check_products(calls, g, op, "host " + name, False, rng)
    fc.check_probe(calls, g, op, "host " + name, False, rng)
    fc.check_loop(calls, g, op, "host " + name, False, rng)


def test_host_double_refusals(calls):
    fc.check_refusals(calls)
