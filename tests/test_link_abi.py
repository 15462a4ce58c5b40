"""include/pgh_link.h at the C-ABI (no GPU): its table in _lib matches the header and is disjoint from the others, the constants match,
the Makefile builds its source against the header, the HIP library exports and binds every entry, and the host test double has none."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")
ENTRIES = ["pgh_link_auc", "pgh_link_factors", "pgh_link_plan_create", "pgh_link_plan_destroy", "pgh_link_plan_info", "pgh_link_predictions"]


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


def test_link_header_table_and_makefile_agree():
    import ctypes as C
    from pygrank_amd import _lib
    assert sorted(_lib.LINK_SIGNATURES) == _declared("pgh_link.h") == ENTRIES
    tables = [name for name in dir(_lib) if name.endswith("SIGNATURES") and name != "LINK_SIGNATURES"]
    assert "SIGNATURES" in tables and "RANK_SIGNATURES" in tables and "KRYLOV_SIGNATURES" in tables
    for name in tables:
        assert set(_lib.LINK_SIGNATURES).isdisjoint(getattr(_lib, name)), name
    headers = [os.path.basename(path) for path in glob.glob(os.path.join(ROOT, "include", "*.h"))]
    assert "pgh.h" in headers and "pgh_link.h" in headers
    for header in headers:
        if header != "pgh_link.h":
            assert set(ENTRIES).isdisjoint(_declared(header)), header
    assert _lib.DECLINED == _defined("pgh_link.h", "PGH_LINK_DECLINED") == 2
    assert _lib.LINK_MAX_PAIRS == _defined("pgh_link.h", "PGH_LINK_MAX_PAIRS") == 2 ** 27
    assert _lib.LINK_COS == _defined("pgh_link.h", "PGH_LINK_COS")
    assert _lib.LINK_DOT == _defined("pgh_link.h", "PGH_LINK_DOT")
    assert _lib.LINK_COS != _lib.LINK_DOT
    mat, vec, plan = C.c_void_p, C.c_void_p, C.c_void_p
    i32p, i64p, dblp, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    want = {
        "pgh_link_plan_create": [C.c_int64, C.c_int64, i32p, i32p, u8p, C.POINTER(plan)],
        "pgh_link_plan_info": [plan, i64p, i64p, i64p],
        "pgh_link_plan_destroy": [plan],
        "pgh_link_auc": [mat, plan, C.c_int32, dblp, i64p, i64p],
        "pgh_link_predictions": [mat, plan, C.c_int32, C.c_int64, C.c_int64, dblp],
        "pgh_link_factors": [mat, C.c_int32, vec],
    }
    for name, argtypes in want.items():
        restype, got = _lib.LINK_SIGNATURES[name]
        assert restype is C.c_int and got == argtypes, name
    makefile = open(os.path.join(ROOT, "pygrank_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bpgh_link\.hip\b", makefile, re.M)
    assert re.search(r"^_build/%\.o:.*include/pgh_link\.h\b", makefile, re.M)


def test_hip_library_exports_and_binds_the_link_entries(hip_lib):
    from pygrank_amd import _lib
    cdll = _lib.load_library(hip_lib)
    bound = _lib.bind_optional(cdll, _lib.LINK_SIGNATURES)
    assert sorted(bound) == ENTRIES
    for name in ENTRIES:
        assert hasattr(cdll, name), name
        assert bound[name] is not None and bound[name].argtypes == _lib.LINK_SIGNATURES[name][1], name


def test_host_double_has_no_link_entry(host_engine):
    from pygrank_amd import _lib
    for name in _lib.LINK_SIGNATURES:
        assert _lib.entry(name) is None, name
