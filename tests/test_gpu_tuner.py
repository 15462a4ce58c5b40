"""ParameterTuner on the GPU: the fixture's recorded steps through the fused route (pgh_probe_auc) and through the unfused one, the
end-to-end run, the engine's decline behind the tuner, and the timing tool at a small scale."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tuner_common as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return tc.fixture()


def test_replay_takes_the_fused_route_and_equals_the_unfused_one(gpu_engine, fx):
    pg = gpu_engine
    _, seeds, _ = tc.planted(pg, fx)
    fused_tuner = tc.tuner_for(pg, fx)
    fused = tc.replay(fx, tc.tuner_loss(pg, fused_tuner, seeds))
    assert fused_tuner.last_tune == dict(fused_steps=len(fx["tuner"]["steps"]), unfused_steps=0)
    plain_tuner = tc.tuner_for(pg, fx, fuse=False)
    plain = tc.replay(fx, tc.tuner_loss(pg, plain_tuner, seeds))
    assert plain_tuner.last_tune == dict(fused_steps=0, unfused_steps=len(fx["tuner"]["steps"]))
    assert fused == plain


def test_end_to_end_on_the_fused_route(gpu_engine, fx):
    pg = gpu_engine
    tuner = tc.tuner_for(pg, fx)
    graph, seeds, ranks = tc.end_to_end(pg, fx, tuner)
    assert tuner.last_tune["fused_steps"] > 0 and tuner.last_tune["unfused_steps"] == 0
    plain = tc.tuner_for(pg, fx, fuse=False)
    assert np.array_equal(np.asarray(plain(graph, seeds).np, dtype=np.float64), ranks) and plain.last_params == tuner.last_params
    ppr = pg.ParameterTuner(lambda params: pg.PageRank(alpha=params[0]), measure=pg.AUC, deviation_tol=0.01, max_vals=[0.99],
                            min_vals=[0.5], verbose=False)
    assert isinstance(ppr(graph, seeds), pg.GraphSignal) and 0.5 <= ppr.last_params[0] <= 0.99
    cos = pg.ParameterTuner(measure=pg.Cos, verbose=False, **fx["tuner_args"])
    assert isinstance(cos(graph, seeds), pg.GraphSignal) and cos.last_tune == dict(fused_steps=0, unfused_steps=0)


def test_a_declined_step_takes_the_unfused_route(gpu_engine, fx):
    """70 hop weights and a tolerance no step meets: more than 64 terms, which pgh_probe_auc declines."""
    pg = gpu_engine
    _, seeds, _ = tc.planted(pg, fx)
    args = dict(max_vals=[1] * 70, min_vals=[1] + [0] * 69, fraction_of_training=0.5, tol=1e-30, error_type=pg.L1)
    candidates = [[1.0] + [0.5 + 0.1 * k] * 69 for k in range(4)]
    tuner = pg.ParameterTuner(verbose=False, **args)
    got = tc.tuner_loss(pg, tuner, seeds).many(candidates)
    assert tuner.last_tune == dict(fused_steps=0, unfused_steps=1)
    plain = pg.ParameterTuner(verbose=False, fuse=False, **args)
    assert got == tc.tuner_loss(pg, plain, seeds).many(candidates)
    assert all(-1.0 <= v <= 0.0 for v in got)


def test_tune_bench_runs_at_scale_20(gpu_engine):
    out = subprocess.run([sys.executable, os.path.join(tc.ROOT, "tools", "tune_bench.py"), "--scale", "20", "--steps", "8", "--reps", "3"],
                         capture_output=True, text=True, timeout=420)
    assert out.returncode == 0, out.stderr[-2000:]
    report = json.loads(out.stdout.strip().splitlines()[-1])
    print(report)
    assert report["fused"]["samples"] == report["sequential"]["samples"] == 24
    assert report["routes"]["unfused_steps"] == 0 and report["fused"]["median_ms"] > 0 and report["sequential"]["median_ms"] > 0
