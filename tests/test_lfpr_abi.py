"""include/pgh_lfpr.h at the C-ABI (no GPU): its table in _lib matches the header and is disjoint from the others, the Makefile builds
its source against the header, the HIP library exports and binds both entries, and the host test double has neither."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")
ENTRIES = ["pgh_lfpr_close", "pgh_lfpr_setup"]


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


def test_lfpr_header_table_and_makefile_agree():
    import ctypes as C
    from pygrank_amd import _lib
    assert sorted(_lib.LFPR_SIGNATURES) == _declared("pgh_lfpr.h") == ENTRIES
    assert _lib.OPTIONAL["pgh_lfpr.h"] is _lib.LFPR_SIGNATURES
    for header, other in [("pgh.h", _lib.SIGNATURES), *_lib.OPTIONAL.items()]:
        if header != "pgh_lfpr.h":
            assert set(_lib.LFPR_SIGNATURES).isdisjoint(other), header
            assert set(ENTRIES).isdisjoint(_declared(header)), header
    assert _lib.DECLINED == _defined("pgh_lfpr.h", "PGH_LFPR_DECLINED")
    vec, dbl = C.c_void_p, C.c_double
    restype, argtypes = _lib.LFPR_SIGNATURES["pgh_lfpr_setup"]
    assert restype is C.c_int
    assert argtypes == [vec, vec, vec, vec, dbl, vec, vec, vec, vec, vec, C.POINTER(C.c_double)]
    restype, argtypes = _lib.LFPR_SIGNATURES["pgh_lfpr_close"]
    assert restype is C.c_int
    assert argtypes == [vec, vec, dbl, vec, vec, vec, vec, vec, dbl, dbl, dbl, C.c_int32, vec, vec, C.POINTER(C.c_double)]
    makefile = open(os.path.join(ROOT, "pygrank_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bpgh_lfpr\.hip\b", makefile, re.M)
    assert re.search(r"^_build/%\.o:.*include/pgh_lfpr\.h\b", makefile, re.M)


def test_hip_library_exports_and_binds_the_lfpr_entries(hip_lib):
    from pygrank_amd import _lib
    cdll = _lib.load_library(hip_lib)
    bound = _lib.bind_optional(cdll, _lib.LFPR_SIGNATURES)
    assert sorted(bound) == ENTRIES
    for name in ENTRIES:
        assert hasattr(cdll, name), name
        assert bound[name] is not None and bound[name].argtypes == _lib.LFPR_SIGNATURES[name][1], name


def test_host_double_has_no_lfpr_entry(host_engine):
    from pygrank_amd import _lib
    for name in _lib.LFPR_SIGNATURES:
        assert _lib.entry(name) is None, name
