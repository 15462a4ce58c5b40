"""The f64 image's step kernels (pygrank_amd/csrc/pgh_bsf64.hip) held to f64, row by row, on graphs small enough to reason about:
the blocked stream (k_bsf64_partial in its six shapes, k_bsf64_fixup with both chain paths, k_bsf64_combine), the cold image
(k_pb64_gather / k_pb64_finish: fixed-point bins, hub bins, rows left in the stream), the narrowed stream, the way in and out and the
isolated-row watch -- reached through pgh_poly_terms, pgh_ppr_run_f64 / pgh_absorb_run_f64 / pgh_sarw_run_f64 and pgh_poly_run.

References, bounds and graphs: tests/f64_common.py (every term of a row's bound is derived there; tests/test_f64_bounds_host.py
shows that the bounds reject f32 accumulation, a matrix entry rounded once too often, a dropped cold entry, too few fixed-point bits
and a stale isolated row).  The layout of the f64 image is fixed when it is first built, so every case sets its switches in a block
that restores them, builds a fresh graph, makes its first f64 call inside the block, and asserts its premise from format(): a case
that fell back to another layout fails.  The worst |error| / bound of every check is kept in f64_common.F64_REPORT and printed when
the module is done (pytest -s)."""
import re

import numpy as np
import pytest

import f64_common as fc

pytestmark = pytest.mark.gpu

IMAGE = dict(PGH_PB="1", PGH_PB_FORCE="1")
# name -> (switches, column blocks, cold image, heavy rows left in the stream).  n = 3 001 > PGH_HOT64: eight blocks unless forced.
LAYOUTS = {
    "hot": (dict(), 1, False, False),
    "hot256 gathers": (dict(PGH_HOT64="256", PGH_PB64="0"), 8, False, False),
    "hot32 gathers": (dict(PGH_HOT64="32", PGH_PB64="0"), 8, False, False),
    "hot256 image": (dict(PGH_HOT64="256", **IMAGE), 8, True, False),
    "hot32 image": (dict(PGH_HOT64="32", **IMAGE), 8, True, False),
    # the two hub rows (~1 000 entries): one hub bin each; or, split into pieces of <= 300 entries -- more pieces than the image has
    # source chunks (one) -- left in the stream (pb_plan_layout)
    "hot32 hub bins": (dict(PGH_HOT64="32", PGH_PB_HEAVY="256", PGH_PB_HUBMAX="2000", **IMAGE), 8, True, False),
    "hot32 heavy rows": (dict(PGH_HOT64="32", PGH_PB_HEAVY="256", PGH_PB_HUBMAX="300", **IMAGE), 8, True, True),
    "hot32 image 4-byte": (dict(PGH_HOT64="32", PGH_STREAM16="0", **IMAGE), 8, True, False),
    "1 block image": (dict(PGH_HOT64="32", PGH_BLOCKS64="1", **IMAGE), 1, True, False),
    "1 block gathers": (dict(PGH_HOT64="32", PGH_BLOCKS64="1", PGH_PB64="0"), 1, False, False),
    "8 blocks forced": (dict(PGH_HOT64="32", PGH_BLOCKS64="8", **IMAGE), 8, True, False),
    "8 blocks all hot": (dict(PGH_BLOCKS64="8", **IMAGE), 8, False, False),     # no cold source: nothing for an image to hold
    "16 blocks": (dict(PGH_HOT64="32", PGH_BLOCKS64="16", **IMAGE), 16, False, False),
    "32 blocks": (dict(PGH_HOT64="32", PGH_BLOCKS64="32", **IMAGE), 32, False, False),
    "64 blocks": (dict(PGH_HOT64="32", PGH_BLOCKS64="64", **IMAGE), 64, False, False),
}
# (layout, upload route, weights): every route on the layouts that differ in kernels, one route each on the others
CASES = [(layout, kind, weights)
         for layout in ("hot", "hot32 gathers", "hot32 image", "hot32 heavy rows", "1 block image", "16 blocks")
         for kind, weights in (("col", "mult"), ("two-sided", "unit"), ("valued", "real"))]
CASES += [("hot256 gathers", "two-sided", "mult"), ("hot256 image", "valued", "real"), ("hot32 hub bins", "two-sided", "mult"),
          ("hot32 hub bins", "valued", "real"), ("hot32 image 4-byte", "col", "unit"), ("hot32 image 4-byte", "valued", "real"),
          ("1 block gathers", "col", "unit"), ("8 blocks forced", "col", "unit"), ("8 blocks all hot", "valued", "real"),
          ("32 blocks", "two-sided", "mult"), ("64 blocks", "valued", "real"), ("64 blocks", "col", "mult")]


@pytest.fixture(scope="module")
def calls(gpu_engine):
    return fc.Calls(gpu_engine)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    fc.print_report("f64 step kernels: worst |error| / bound per case")


_GRAPHS = {}


def _small(weights):
    if weights not in _GRAPHS:
        _GRAPHS[weights] = fc.small_graph(np.random.default_rng(3), weights)
    return _GRAPHS[weights]


def _chain():
    if "chain" not in _GRAPHS:
        _GRAPHS["chain"] = fc.chain_graph(np.random.default_rng(9))
    return _GRAPHS["chain"]


def assert_premise(g, op, blocks, image, heavy, narrow=None, case=None):
    """The layout the case is about, from format() once the f64 image exists."""
    fmt = g.format()
    if case is not None:
        fc.F64_FORMATS[case] = fmt
    assert "f64 image: %d column blocks" % blocks in fmt, fmt
    tail = fmt.split("f64 image")[1]
    found = re.search(r"f64 propagation-blocking image of (\d+) entries", tail)
    assert (found is not None and int(found.group(1)) > 0) == image, fmt
    assert ("heavy rows stay in the stream" in tail) == heavy, fmt
    if narrow is None:
        narrow = image and not heavy                          # bsf64_ensure: hot-only streams are narrowed unless PGH_STREAM16=0
    assert "(%d B/entry)" % ((4 if op.valued else 0) + (2 if narrow else 4)) in tail, fmt
    return int(found.group(1)) if found else 0


def _first_call(calls, g, op):
    calls.terms(g, np.ones(op.n, dtype=fc.F32), 1, 1)       # builds the f64 image under the block's switches


@pytest.mark.parametrize("layout,kind,weights", CASES)
def test_f64_steps_row_by_row(calls, layout, kind, weights):
    """Items 1, 2, 4, 5, 6, 7 and 8 of f64_common on one layout of the 3 001-node graph."""
    env, blocks, image, heavy = LAYOUTS[layout]
    W, iso = _small(weights)
    with fc.layout_env(**env):
        g, op = fc.upload(calls.pg, W, kind)
        _first_call(calls, g, op)
        case = "%s / %s %s" % (layout, kind, weights)
        assert_premise(g, op, blocks, image, heavy, False if "PGH_STREAM16" in env else None, case)
        fc.full_battery(calls, g, op, case, image, iso, 17)


@pytest.mark.parametrize("layout,weights", [("hot", "mult"), ("hot32 gathers", "unit"), ("hot32 image", "mult"), ("hot32 heavy rows", "unit"),
                                            ("16 blocks", "mult")])
def test_f64_integer_terms_are_exact(calls, layout, weights):
    """Item 3: integer weights, no normalisation, integer inputs: T_2 .. T_6 to the bit."""
    env, blocks, image, heavy = LAYOUTS[layout]
    W, _ = _small(weights)
    with fc.layout_env(**env):
        g, op = fc.upload(calls.pg, W, "none")
        _first_call(calls, g, op)
        assert_premise(g, op, blocks, image, heavy)
        fc.check_exact(calls, g, op, "%s / none %s" % (layout, weights), np.random.default_rng(5))


# the 20 000-node graph in one column block.  "pieces": two source chunks (17 500 - 512 cold sources > 16 384), so the 17 000-entry
# row -- at least 16 488 of its entries cold, more than PGH_PB_HEAVY -- is split into ceil(c / 9 000) = 2 hub pieces; had the image
# one chunk only, the row would stay in the stream and the premise (no heavy rows) would fail
CHAIN_LAYOUTS = {
    "hot only": (dict(PGH_BLOCKS64="1"), False, "col"),
    "hub bins": (dict(PGH_BLOCKS64="1", PGH_HOT64="2048", PGH_PB_HEAVY="4096", **IMAGE), True, "two-sided"),
    "hub pieces": (dict(PGH_BLOCKS64="1", PGH_HOT64="512", PGH_PB_HEAVY="4096", PGH_PB_HUBMAX="9000", **IMAGE), True, "col"),
}


@pytest.mark.parametrize("layout", list(CHAIN_LAYOUTS))
def test_f64_long_chains(calls, layout):
    """Rows of 17 000 and 8 000 entries and of every length up to 1 100 in ONE block: the whole-wavefront chain of the fix-up (32 or
    more tiles), the short chains, segment ends on every alignment; with a small hot cache the long rows are hub bins and pieces."""
    env, image, kind = CHAIN_LAYOUTS[layout]
    W, iso = _chain()
    case = "chain %s / %s" % (layout, kind)
    with fc.layout_env(**env):
        g, op = fc.upload(calls.pg, W, kind)
        _first_call(calls, g, op)
        entries = assert_premise(g, op, 1, image, False, case=case)
        if layout == "hub pieces":
            assert entries >= 17000 - 512, entries
        rng = np.random.default_rng(21)
        fc.check_products(calls, g, op, case, image, rng)
        fc.check_probe(calls, g, op, case, image, rng)
        fc.check_chains(calls, g, op, case, image, rng)
        fc.check_poly(calls, g, op, case, image, rng)
        fc.check_isolated(calls, g, op, case, iso, rng)


def test_f64_isolated_items_of_the_cold_image(calls):
    """Item 8 where the finishing pass of the cold image has isolated ITEMS to pass over: on the graphs above one bin spans every row,
    the isolated ones included, and they are summed like any other.  Here 20 000 isolated rows follow 4 000 live ones in one block:
    the image's one bin holds at most 16 384 rows, so at least 7 616 isolated rows lie behind it."""
    W, iso = fc.iso_tail_graph(np.random.default_rng(13))
    case = "isolated tail / col"
    with fc.layout_env(PGH_BLOCKS64="1", PGH_HOT64="32", **IMAGE):
        g, op = fc.upload(calls.pg, W, "col")
        _first_call(calls, g, op)
        assert_premise(g, op, 1, True, False, case=case)
        assert "in 1 chunks x 1 bins" in g.format() and len(iso) > 16384, g.format()
        rng = np.random.default_rng(23)
        fc.check_products(calls, g, op, case, True, rng)
        fc.check_probe(calls, g, op, case, True, rng)
        fc.check_isolated(calls, g, op, case, iso, rng)


@pytest.mark.parametrize("name", ["loop1", "edge2", "ring65"])
def test_f64_tiny_graphs(calls, name):
    W = fc.tiny_graphs()[name]
    case = "tiny " + name
    with fc.layout_env():
        g, op = fc.upload(calls.pg, W, "col")
        _first_call(calls, g, op)
        assert_premise(g, op, 1, False, False)
        rng = np.random.default_rng(2)
        fc.check_products(calls, g, op, case, False, rng)
        fc.check_probe(calls, g, op, case, False, rng)
        fc.check_loop(calls, g, op, case, False, rng)


def test_f64_entries_refuse_graphs_without_an_image(calls):
    """Item 9: rectangular graphs and graphs without an entry."""
    with fc.layout_env():
        fc.check_refusals(calls)
