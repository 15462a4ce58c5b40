"""tools/benchkit.py on the host: the sampler's order and what it keeps, the summary, the disjoint-spreads rule, the record's line and
file, the seed draws against the loop the tools wrote out, and the bring-up's message.  No engine: a fake timer returns scripted
milliseconds and records its calls."""
import json
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import benchkit  # noqa: E402


class ScriptedTimer:
    def __init__(self, script):
        self.script, self.calls = list(script), []

    def time(self, fn):
        value = fn()
        self.calls.append(value[0])
        return self.script.pop(0), value


def test_alternate_runs_the_routes_in_turn_and_drops_the_first_round():
    timer = ScriptedTimer([100.0, 200.0, 300.0, 1.0, 2.0, 3.0, 1.5, 2.5, 3.5])
    runs = {name: 0 for name in ("r1", "r2", "r3")}

    def route(name):
        def once():
            runs[name] += 1
            return name, runs[name]
        return once
    seen = []
    got, last = benchkit.alternate(timer, {name: route(name) for name in runs}, 2, lambda name, value: seen.append((name, value)))
    assert timer.calls == ["r1", "r2", "r3"] * 3
    assert list(got) == ["r1", "r2", "r3"]
    assert got["r1"] == dict(median_ms=1.25, min_ms=1.0, max_ms=1.5, samples=2)
    assert got["r2"] == dict(median_ms=2.25, min_ms=2.0, max_ms=2.5, samples=2)
    assert got["r3"] == dict(median_ms=3.25, min_ms=3.0, max_ms=3.5, samples=2)
    assert last == dict(r1=("r1", 3), r2=("r2", 3), r3=("r3", 3))
    assert seen == [(name, (name, rep)) for rep in (1, 2, 3) for name in ("r1", "r2", "r3")]


def test_sample_hands_out_the_milliseconds_themselves():
    timer = ScriptedTimer([9.0, 8.0, 1.0, 2.0, 3.0, 4.0])
    samples, last = benchkit.sample(timer, dict(a=lambda: ("a",), b=lambda: ("b",)), 2)
    assert samples == dict(a=[1.0, 3.0], b=[2.0, 4.0]) and last == dict(a=("a",), b=("b",))


def test_keep_false_lets_a_value_go_once_the_next_run_has_ended():
    import weakref

    class Value:
        pass
    alive = []

    def route():
        alive[:] = [ref for ref in alive if ref() is not None]
        value = Value()
        alive.append(weakref.ref(value))
        return len(alive), value                                     # how many values live while this run makes its own
    timer = ScriptedTimer([1.0] * 6)
    seen = []
    _, last = benchkit.sample(timer, dict(a=route, b=route), 2, lambda name, value: seen.append(value[0]), keep=False)
    assert seen == [1, 2, 2, 2, 2, 2] and list(last) == ["b"]
    timer, alive[:], seen[:] = ScriptedTimer([1.0] * 6), [], []
    _, last = benchkit.sample(timer, dict(a=route, b=route), 2, lambda name, value: seen.append(value[0]))
    assert seen == [1, 2, 3, 3, 3, 3] and list(last) == ["a", "b"]


def test_summary_rounds_to_four_places_in_its_key_order():
    got = benchkit.summary([1.00004, 3.0, 2.00006])
    assert list(got.items()) == [("median_ms", 2.0001), ("min_ms", 1.0), ("max_ms", 3.0), ("samples", 3)]


def test_disjoint_wants_a_gap_and_honours_the_keys_it_is_given():
    a, b = dict(min_ms=1.0, max_ms=2.0), dict(min_ms=2.0, max_ms=3.0)
    assert benchkit.disjoint(a, b) is False and benchkit.disjoint(b, a) is False           # touching intervals overlap
    assert benchkit.disjoint(a, dict(min_ms=2.5, max_ms=3.0)) is True and benchkit.disjoint(dict(min_ms=2.5, max_ms=3.0), a) is True
    assert benchkit.disjoint(a, dict(min_ms=np.float64(1.5), max_ms=np.float64(3.0))) is False
    keys = dict(lo="min_ms_per_column", hi="max_ms_per_column")
    wide = dict(min_ms=1.0, max_ms=9.0, min_ms_per_column=0.1, max_ms_per_column=0.2)
    narrow = dict(min_ms=2.0, max_ms=3.0, min_ms_per_column=0.3, max_ms_per_column=0.4)
    assert benchkit.disjoint(wide, narrow) is False and benchkit.disjoint(wide, narrow, **keys) is True


def test_over_is_the_ratio_of_the_medians():
    a, b = dict(median_ms=1.0), dict(median_ms=3.0)
    assert benchkit.over(a, b) == 0.3333 and benchkit.over(a, b, 5) == 0.33333 and benchkit.over(b, a) == 3.0


def test_emit_prints_one_line_and_writes_it_where_asked(tmp_path, capsys):
    record = dict(tool="x", nested=dict(b=1, a=[1, 2]), ratio=0.5)
    benchkit.emit(record)
    assert capsys.readouterr().out == json.dumps(record) + "\n"
    assert list(tmp_path.iterdir()) == []
    path = tmp_path / "missing" / "deeper" / "x.log"
    benchkit.emit(record, str(path))
    assert capsys.readouterr().out == json.dumps(record) + "\n"
    assert path.read_text() == json.dumps(record) + "\n"
    assert list(json.loads(path.read_text())) == ["tool", "nested", "ratio"]


class HostVector:
    def __init__(self, values):
        self.values = values

    @classmethod
    def from_host(cls, values):
        return cls(np.array(values))


HOST_PG = types.SimpleNamespace(DeviceVector=HostVector)


def test_seed_columns_draw_what_the_written_out_loop_drew():
    n, width, seeds = 50, 3, 5
    nodes = np.sort(np.random.default_rng(7).choice(n, size=37, replace=False))
    rng = np.random.default_rng(1)
    columns = []
    for _ in range(width):
        p = np.zeros(n)
        p[rng.choice(nodes, size=min(seeds, len(nodes)), replace=False)] = 1.0
        columns.append(HOST_PG.DeviceVector.from_host(p))
    after = rng.choice(n, n // 5, replace=False)

    rng = np.random.default_rng(1)
    got = benchkit.seed_columns(HOST_PG, n, nodes, width, seeds, rng)
    assert len(got) == width and all(isinstance(column, HostVector) for column in got)
    for mine, theirs in zip(got, columns):
        assert np.array_equal(mine.values, theirs.values) and mine.values.sum() == seeds
    assert np.array_equal(rng.choice(n, n // 5, replace=False), after)


def test_seed_vector_draws_once_and_sorting_the_draw_changes_nothing():
    n, seeds = 50, 5
    nodes = np.sort(np.random.default_rng(7).choice(n, size=37, replace=False))
    rng = np.random.default_rng(1)
    p = np.zeros(n)
    p[np.sort(rng.choice(nodes, size=min(seeds, len(nodes)), replace=False))] = 1.0
    after = rng.random(4)
    rng = np.random.default_rng(1)
    assert np.array_equal(benchkit.seed_vector(n, nodes, seeds, rng), p)
    assert np.array_equal(rng.random(4), after)


def test_more_seeds_than_eligible_nodes_sets_them_all():
    n = 50
    nodes = np.sort(np.random.default_rng(7).choice(n, size=37, replace=False))
    want = np.zeros(n)
    want[nodes] = 1.0
    assert np.array_equal(benchkit.seed_vector(n, nodes, 100, np.random.default_rng(1)), want)
    for column in benchkit.seed_columns(HOST_PG, n, nodes, 3, 100, np.random.default_rng(1)):
        assert np.array_equal(column.values, want)


def test_engine_names_what_the_library_lacks(monkeypatch):
    calls = []
    L = types.ModuleType("pygrank_amd._lib")
    L.ensure_init = lambda: calls.append("ensure_init")
    L.entry = lambda name: None if name == "pgh_absent" else object()
    pg = types.ModuleType("pygrank_amd")
    pg.load_backend = lambda name: calls.append(("load_backend", name))
    pg._lib = L
    monkeypatch.setitem(sys.modules, "pygrank_amd", pg)
    monkeypatch.setitem(sys.modules, "pygrank_amd._lib", L)
    with pytest.raises(SystemExit) as raised:
        benchkit.engine("pgh_present", "pgh_absent", what="the entries of include/pgh_absent.h")
    assert str(raised.value) == "the engine library lacks the entries of include/pgh_absent.h"
    assert calls == [("load_backend", "hip"), "ensure_init"]
    with pytest.raises(SystemExit) as raised:
        benchkit.engine("pgh_absent")
    assert str(raised.value) == "the engine library lacks pgh_absent"
