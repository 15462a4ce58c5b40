"""Postprocessor.propagate on the GPU: the comparison of tests/test_postprocess_host.py on the "slab" route -- one inner batch, the
entries of include/pgh_post.h counted -- at the same bounds: exact for Top, Threshold, Ordinals, Sweep, LinearSweep and the chain,
4 * 2^-24 relative for Normalize and Transformer (postprocess_common.REL).  `fused=False` (the inner batch kept, the columns through
backend primitives) is held to the same bounds against `fused=True`."""
import numpy as np
import pytest

import oversampling_common as oc
import postprocess_common as pc

pytestmark = pytest.mark.gpu

CALLS = {
    "Top": {"pgh_post_kth_largest": 1, "pgh_post_col_threshold": 1},
    "TopShare": {"pgh_post_kth_largest": 1, "pgh_post_col_threshold": 1},
    "Threshold": {"pgh_post_col_threshold": 1},
    "Ordinals": {"pgh_post_ordinals": 1},
    "Sweep": {"pgh_post_row_op": 1},
    "LinearSweep": {"pgh_post_row_op": 1},
    "NormalizeMax": {"pgh_mat_col_stats": 1, "pgh_post_col_affine": 1},
    "NormalizeSum": {"pgh_mat_col_stats": 1, "pgh_post_col_affine": 1},
    "NormalizeL2": {"pgh_mat_col_stats": 1, "pgh_post_col_affine": 1},
    "NormalizeRange": {"pgh_mat_col_stats": 1, "pgh_post_col_affine": 1},
    "Transformer": {"pgh_ewise_unary": 1},
}


@pytest.mark.parametrize("name", sorted(pc.EXACT))
@pytest.mark.parametrize("width", pc.WIDTHS)
@pytest.mark.parametrize("key", pc.GRAPHS)
def test_propagate_takes_the_slab_route(gpu_engine, key, width, name):
    pg = gpu_engine
    _, steps, _, fused = pc.check_propagate(pg, key, width, name, "slab")
    chunks = [min(64, width - first) for first in range(0, width, 64)]
    for step in steps:
        assert step.last_propagate["chunks"] == chunks
        calls = dict(step.last_propagate["calls"])
        if name == "ThresholdGap":
            assert calls == {"pgh_mat_get_col": width, "pgh_vec_gap_threshold": width, "pgh_post_col_threshold": len(chunks)}
        elif name != "Chain":
            assert calls == {entry: times * len(chunks) for entry, times in CALLS[name].items()}
    # the inner batch kept, the columns through backend primitives: the same values at the same bounds
    _, _, _, unfused = pc.check_propagate(pg, key, width, name, "columns", fused=False)
    for j in range(width):
        assert pc.within(fused[:, j], unfused[:, j], pc.EXACT[name]), (key, width, name, j)


def test_top_of_64_columns_is_one_select_one_compare_and_one_inner_batch(gpu_engine):
    pg = gpu_engine
    case = oc.Case(pg, "rmat12_sym")
    F = pc.features(case.n, 64)
    ranker = case.ranker()
    post = pg.Top(ranker, 10)
    got = post.propagate(case.graph, F).numpy()
    assert post.last_propagate == dict(route="slab", chunks=[64], calls={"pgh_post_kth_largest": 1, "pgh_post_col_threshold": 1})
    assert [len(batch) for batch in ranker.last_batches] == [64]
    inner = case.ranker().propagate(case.graph, F).numpy()
    for j in range(64):
        cut = np.sort(inner[:, j])[::-1][9]
        assert np.array_equal(got[:, j], (inner[:, j] >= cut).astype(np.float64)), j
    # a keep outside [1, n] leaves the cut 0, as rank does: no select
    everything = pg.Top(case.ranker(), case.n + 1)
    assert np.all(everything.propagate(case.graph, F).numpy() == 1.0)
    assert dict(everything.last_propagate["calls"]) == {"pgh_post_col_threshold": 1}


def test_batch_false_is_the_column_loop_bit_for_bit(gpu_engine):
    pg = gpu_engine
    case = oc.Case(pg, "weighted300")
    F = pc.features(case.n, 3)
    post, _ = pc.build(pg, "Chain", case.ranker(), case.n)
    post.batch = False
    got = post.propagate(case.graph, F).numpy()
    assert post.last_propagate["route"] == "ranks"
    again, _ = pc.build(pg, "Chain", case.ranker(), case.n)
    assert np.array_equal(got, pg.NodeRanking.propagate(again, case.graph, F).numpy())


def test_zero_and_constant_columns_stay(gpu_engine):
    pg = gpu_engine
    case = oc.Case(pg, "weighted300")
    G = np.abs(np.random.default_rng(3).normal(size=(case.n, 4)))
    G[:, 1] = 0.0
    G[:, 2] = 0.25
    for method in ("max", "sum", "L2", "range"):
        post = pg.Normalize(method=method)
        got = post.propagate(case.graph, G).numpy()
        assert post.last_propagate["route"] == "slab"
        assert not got[:, 1].any()
        for j in range(4):
            ranks = pg.Normalize(method=method).rank(case.graph, pg.to_signal(case.graph, G[:, j].copy()))
            assert pc.within(got[:, j], np.asarray(ranks.np, dtype=np.float64), False), (method, j)
        if method == "range":
            assert np.array_equal(got[:, 2], np.full(case.n, 0.25))


def test_sweep_inside_seed_oversampling_batches(gpu_engine):
    pg = gpu_engine
    case = oc.Case(pg, "rmat10_dir")
    F = pc.features(case.n, 8)
    ranker = case.ranker()
    swept = pg.create_many_variation_types()["SweepO"](ranker)
    got = swept.propagate(case.graph, F).numpy()
    assert swept.ranker.last_propagate["route"] == "slab" and [len(batch) for batch in ranker.last_batches] == [8]
    for j in range(8):
        alone = pg.create_many_variation_types()["SweepO"](case.ranker()).rank(case.graph, F[:, j].copy())
        assert oc.rel_linf(got[:, j], np.asarray(alone.np, dtype=np.float64)) <= oc.BAR
