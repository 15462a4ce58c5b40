"""The fused single-vector loops under the switches the engine reads once per process: PGH_POLL, PGH_DEFER_CLOSE, PGH_FUSED_RES,
PGH_FIRST_PRED and PGH_PUBLISHED_STATE.  Each set runs tests/loop_switch_worker.py as a child of its own, one after
the other: four graphs (the one-workgroup tail, the general sequence, a cold image, the row-major branch), every loop route on each
against oracle/ref_loops.py -- rel-Linf <= 1e-6, equal iteration counts, two runs with equal bits (see the worker's docstring)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("PGH_POLL", "PGH_DEFER_CLOSE", "PGH_FUSED_RES", "PGH_FIRST_PRED", "PGH_PUBLISHED_STATE", "PGH_CHEB_F32", "PGH_WINDOW",
            "PGH_SEED_PUSH", "PGH_SEED_PUSH2", "PGH_SMALL_TAIL", "PGH_PB", "PGH_PB_FORCE", "PGH_FORMAT", "PGH_BLOCKS")
SETS = [("defaults", {}),
        ("poll0", dict(PGH_POLL="0")),
        ("defer_close0", dict(PGH_DEFER_CLOSE="0")),
        ("fused_res0", dict(PGH_FUSED_RES="0")),
        ("first_pred0", dict(PGH_FIRST_PRED="0")),
        ("published_state0", dict(PGH_PUBLISHED_STATE="0")),
        ("poll0_defer_close0_fused_res0", dict(PGH_POLL="0", PGH_DEFER_CLOSE="0", PGH_FUSED_RES="0"))]
# a child took about one second when this was written (uploads, the scale-16 image and the first child's oracle runs included): the
# limit leaves room for a loaded machine, no more
TIMEOUT = 120


@pytest.fixture(scope="module")
def oracle_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("loop_switch_oracle"))


@pytest.mark.parametrize("label,switches", SETS, ids=[s[0] for s in SETS])
def test_loops_under_switch_set(oracle_cache, label, switches):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "loop_switch_worker.py"), oracle_cache, label],
                         capture_output=True, text=True, timeout=TIMEOUT, env=env, cwd=ROOT)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-6000:] + res.stderr[-3000:]
    assert f"{label}: 0 failed checks" in res.stdout, res.stdout[-3000:]
