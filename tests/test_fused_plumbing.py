"""The plumbing every fused route shares (no GPU): _lib.entry and _lib.accepted, DeviceMatrix.chunks and device.EnginePlan."""
import os

import numpy as np
import pytest

import host_double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")


def test_entry_binds_per_library(oracle_build_dir):
    """Every optional name is bound on the HIP library (dlopen only), None once the host double is installed, and bound again once
    it is removed: the cache belongs to the library object."""
    from pygrank_amd import _lib
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pygrank_amd", "csrc")])
    names = [name for table in _lib.OPTIONAL.values() for name in table]
    assert len(_lib.OPTIONAL) == 13 and len(names) == len(set(names)) == 41 and set(names).isdisjoint(_lib.SIGNATURES)
    assert not host_double.active()
    try:
        with pytest.raises(KeyError):
            _lib.entry("pgh_no_such_entry")
        with pytest.raises(KeyError):
            _lib.entry("pgh_spmv")                              # a required symbol is no optional entry
        hip = _lib.lib()
        for table in _lib.OPTIONAL.values():
            for name, (restype, argtypes) in table.items():
                assert _lib.entry(name) is not None and _lib.entry(name).argtypes == argtypes, name
        host_double.install(os.path.join(oracle_build_dir, "libpgh_host_oracle.so"))
        assert _lib.lib() is not hip
        assert all(_lib.entry(name) is None for name in names)
        with pytest.raises(KeyError):
            _lib.entry("pgh_no_such_entry")
        host_double.remove()
        assert all(_lib.entry(name) is not None for name in names)
    finally:
        host_double.remove()


def test_entry_reads_the_family_cache_on_the_library_object(host_engine):
    """A family's table sits on the library object as _pgh_<family>_entries: what a test puts there is what entry returns."""
    from pygrank_amd import _lib
    cdll = _lib.lib()
    assert _lib.entry("pgh_lfpr_close") is None and set(cdll._pgh_lfpr_entries) == set(_lib.LFPR_SIGNATURES)
    stand_in, saved = object(), cdll._pgh_lfpr_entries
    cdll._pgh_lfpr_entries = dict(saved, pgh_lfpr_close=stand_in)
    try:
        assert _lib.entry("pgh_lfpr_close") is stand_in and _lib.entry("pgh_lfpr_setup") is None
        assert _lib.entry("pgh_post_ordinals") is None          # another family: its own table
    finally:
        cdll._pgh_lfpr_entries = saved


def test_accepted(host_engine):
    from pygrank_amd import _lib
    assert _lib.DECLINED == 2
    assert _lib.accepted(0) is True
    assert _lib.accepted(_lib.DECLINED) is False
    for status in (1, 3, -1):
        with pytest.raises(_lib.EngineError):
            _lib.accepted(status)


@pytest.mark.parametrize("b, width, widths", [(1, 64, [1]), (64, 64, [64]), (65, 64, [64, 1]), (130, 64, [64, 64, 2]), (3, 1, [1, 1, 1])])
def test_chunks(host_engine, b, width, widths):
    pg = host_engine
    source = np.arange(3 * b, dtype=np.float64).reshape(3, b) - 7.0
    slab = pg.DeviceMatrix.from_host(source)
    parts = list(slab.chunks() if width == 64 else slab.chunks(width=width))
    if b <= width:
        assert len(parts) == 1 and parts[0][0] == 0 and parts[0][1] is slab
    assert [part.b for _, part in parts] == widths
    assert [first for first, _ in parts] == [sum(widths[:i]) for i in range(len(widths))]
    for first, part in parts:
        assert part.n == 3 and np.array_equal(part.numpy(), source[:, first:first + part.b])


class _Recorder:
    """Stands in for _lib.entry: hands out one destroy function and records what it is asked for and called with."""

    def __init__(self, raises=False):
        self.asked, self.destroyed, self.raises = [], [], raises

    def __call__(self, name):
        self.asked.append(name)
        return self._destroy

    def _destroy(self, handle):
        self.destroyed.append(handle)
        if self.raises:
            raise RuntimeError("destroy failed")
        return 0


def _plan(handle):
    from pygrank_amd.device import EnginePlan

    class Plan(EnginePlan):
        _DESTROY = "pgh_some_plan_destroy"

        def __init__(self):
            self._h = handle
    return Plan()


def test_engine_plan_frees_its_handle_once(host_engine, monkeypatch):
    from pygrank_amd import _lib
    _lib.lib()
    recorder = _Recorder()
    monkeypatch.setattr(_lib, "entry", recorder)
    handle = object()
    plan = _plan(handle)
    plan.__del__()                                             # what dropping the last reference runs
    assert recorder.asked == ["pgh_some_plan_destroy"] and recorder.destroyed == [handle] and plan._h is None
    plan.__del__()
    del plan
    assert recorder.destroyed == [handle]
    _plan(handle)                                               # dropped at once: CPython runs __del__ here
    assert recorder.destroyed == [handle, handle]
    assert _plan(None).__del__() is None and len(recorder.destroyed) == 2      # no handle yet (a lazy plan): nothing to free


def test_engine_plan_without_a_library_or_with_a_failing_destroy(host_engine, monkeypatch):
    from pygrank_amd import _lib
    _lib.lib()
    recorder = _Recorder(raises=True)
    monkeypatch.setattr(_lib, "entry", recorder)
    plan = _plan(object())
    plan.__del__()                                              # the destroy entry raises: swallowed, the handle is given up
    assert len(recorder.destroyed) == 1 and plan._h is None
    plan = _plan(object())
    monkeypatch.setattr(_lib, "_lib", None)                     # the library is gone (interpreter shutdown): no call at all
    plan.__del__()
    assert len(recorder.destroyed) == 1 and len(recorder.asked) == 1 and plan._h is None


def test_the_three_plans_name_their_destroy_entries():
    """__del__ swallows every exception, so a misspelt _DESTROY would leak every plan without a sound: each is a declared entry."""
    from pygrank_amd import _lib, autotune, measures, multigroup
    from pygrank_amd.device import EnginePlan
    assert autotune._ProbePlan is measures._ProbePlan
    for cls, table in ((measures._ProbePlan, _lib.TUNE_SIGNATURES), (measures._RankPlan, _lib.RANK_SIGNATURES),
                       (multigroup._LinkPlan, _lib.LINK_SIGNATURES)):
        assert issubclass(cls, EnginePlan) and "__del__" not in vars(cls)
        assert cls._DESTROY in table and cls._DESTROY.endswith("_plan_destroy"), cls
