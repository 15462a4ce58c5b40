"""include/pgh_fair.h at the C-ABI (no GPU): its table in _lib matches the header and is disjoint from the others, the Makefile builds
its source against the header, the HIP library exports and binds the entry, and the host test double does not have it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"\b(pgh_[a-z0-9_]+)\s*\(", text)))


def _defined(header, name):
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", open(os.path.join(ROOT, "include", header)).read()).group(1))


@pytest.fixture(scope="module")
def hip_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pygrank_amd", "csrc")])
    return LIB


def test_fair_header_table_and_makefile_agree():
    import ctypes as C
    from pygrank_amd import _lib
    assert sorted(_lib.FAIR_SIGNATURES) == _declared("pgh_fair.h") == ["pgh_prior_edit"]
    assert _lib.OPTIONAL["pgh_fair.h"] is _lib.FAIR_SIGNATURES
    for header, other in [("pgh.h", _lib.SIGNATURES), *_lib.OPTIONAL.items()]:
        if header != "pgh_fair.h":
            assert set(_lib.FAIR_SIGNATURES).isdisjoint(other), header
    assert _lib.DECLINED == _defined("pgh_fair.h", "PGH_FAIR_DECLINED")
    assert _lib.FAIR_MAX_PROBES == _defined("pgh_fair.h", "PGH_FAIR_MAX_PROBES")
    assert _lib.FAIR_MAX_BUCKETS == _defined("pgh_fair.h", "PGH_FAIR_MAX_BUCKETS")
    restype, argtypes = _lib.FAIR_SIGNATURES["pgh_prior_edit"]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    makefile = open(os.path.join(ROOT, "pygrank_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bpgh_fair\.hip\b", makefile, re.M)
    assert re.search(r"^_build/%\.o:.*include/pgh_fair\.h\b", makefile, re.M)


def test_hip_library_exports_and_binds_the_fair_entry(hip_lib):
    from pygrank_amd import _lib
    cdll = _lib.load_library(hip_lib)
    bound = _lib.bind_optional(cdll, _lib.FAIR_SIGNATURES)
    assert sorted(bound) == _declared("pgh_fair.h")
    for name in _declared("pgh_fair.h"):
        assert hasattr(cdll, name), name
        assert bound[name] is not None and bound[name].argtypes == _lib.FAIR_SIGNATURES[name][1], name


def test_host_double_has_no_fair_entry(host_engine):
    from pygrank_amd import _lib
    for name in _lib.FAIR_SIGNATURES:
        assert _lib.entry(name) is None, name
