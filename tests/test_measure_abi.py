"""include/pgh_measure.h at the C-ABI (no GPU): its table in _lib matches the header and is disjoint from the other three, the HIP
library exports and binds every entry, and the host test double has none of them."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    return sorted(set(re.findall(r"\b(pgh_[a-z0-9_]+)\s*\(", _header(name))))


def _defined(name, macro):
    return int(re.search(r"#define\s+" + macro + r"\s+(\d+)", _header(name)).group(1))


@pytest.fixture(scope="module")
def hip_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pygrank_amd", "csrc")])
    return LIB


def test_measure_header_and_table_agree():
    from pygrank_amd import _lib
    assert sorted(_lib.MEASURE_SIGNATURES) == _declared("pgh_measure.h") == ["pgh_cut_forms", "pgh_mat_col_stats"]
    assert _lib.OPTIONAL["pgh_measure.h"] is _lib.MEASURE_SIGNATURES
    for header, other in [("pgh.h", _lib.SIGNATURES), *_lib.OPTIONAL.items()]:
        if header != "pgh_measure.h":
            assert set(_lib.MEASURE_SIGNATURES).isdisjoint(other), header
    assert _lib.DECLINED == _defined("pgh_measure.h", "PGH_MEASURE_DECLINED")
    assert _lib.CUT_ALL == _defined("pgh_measure.h", "PGH_CUT_ALL")
    assert _lib.CUT_INTERNAL == _defined("pgh_measure.h", "PGH_CUT_INTERNAL")
    # pgh.h keeps its own table: nothing of this header leaked into it
    assert sorted(_lib.SIGNATURES) == _declared("pgh.h")


def test_hip_library_exports_and_binds_the_measure_entries(hip_lib):
    from pygrank_amd import _lib
    cdll = _lib.load_library(hip_lib)
    bound = _lib.bind_optional(cdll, _lib.MEASURE_SIGNATURES)
    assert sorted(bound) == _declared("pgh_measure.h")
    for name in _declared("pgh_measure.h"):
        assert hasattr(cdll, name), name
        assert bound[name] is not None and bound[name].argtypes == _lib.MEASURE_SIGNATURES[name][1], name


def test_host_double_has_no_measure_entry(host_engine):
    from pygrank_amd import _lib
    for name in _lib.MEASURE_SIGNATURES:
        assert _lib.entry(name) is None, name
