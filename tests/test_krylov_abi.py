"""include/pgh_krylov.h at the C-ABI (no GPU): its table in _lib matches the header and is disjoint from the others, the Makefile builds
its source against the header, the HIP library exports and binds both entries, and the host test double has neither."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")
ENTRIES = ["pgh_krylov_residuals", "pgh_lanczos_close"]


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


def test_krylov_header_table_and_makefile_agree():
    import ctypes as C
    from pygrank_amd import _lib
    assert sorted(_lib.KRYLOV_SIGNATURES) == _declared("pgh_krylov.h") == ENTRIES
    tables = [name for name in dir(_lib) if name.endswith("SIGNATURES") and name != "KRYLOV_SIGNATURES"]
    assert "SIGNATURES" in tables and "LFPR_SIGNATURES" in tables and "RANK_SIGNATURES" in tables
    for name in tables:
        assert set(_lib.KRYLOV_SIGNATURES).isdisjoint(getattr(_lib, name)), name
    headers = [os.path.basename(path) for path in glob.glob(os.path.join(ROOT, "include", "*.h"))]
    assert "pgh.h" in headers and "pgh_krylov.h" in headers
    for header in headers:
        if header != "pgh_krylov.h":
            assert set(ENTRIES).isdisjoint(_declared(header)), header
    assert _lib.DECLINED == _defined("pgh_krylov.h", "PGH_KRYLOV_DECLINED")
    assert _lib.KRYLOV_MAX_DIMS == _defined("pgh_krylov.h", "PGH_KRYLOV_MAX_DIMS")
    assert _lib.KRYLOV_MAX_PROBES == _defined("pgh_krylov.h", "PGH_KRYLOV_MAX_PROBES")
    vec, mat, dbl, dblp = C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_double)
    restype, argtypes = _lib.KRYLOV_SIGNATURES["pgh_lanczos_close"]
    assert restype is C.c_int
    assert argtypes == [vec, vec, dbl, vec, dbl, vec, mat, C.c_int32, dblp]
    restype, argtypes = _lib.KRYLOV_SIGNATURES["pgh_krylov_residuals"]
    assert restype is C.c_int
    assert argtypes == [mat, dblp, C.c_int32, C.c_int32, dblp, dblp]
    makefile = open(os.path.join(ROOT, "pygrank_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bpgh_krylov\.hip\b", makefile, re.M)
    assert re.search(r"^_build/%\.o:.*include/pgh_krylov\.h\b", makefile, re.M)


def test_hip_library_exports_and_binds_the_krylov_entries(hip_lib):
    from pygrank_amd import _lib
    cdll = _lib.load_library(hip_lib)
    bound = _lib.bind_optional(cdll, _lib.KRYLOV_SIGNATURES)
    assert sorted(bound) == ENTRIES
    for name in ENTRIES:
        assert hasattr(cdll, name), name
        assert bound[name] is not None and bound[name].argtypes == _lib.KRYLOV_SIGNATURES[name][1], name


def test_host_double_has_no_krylov_entry(host_engine):
    from pygrank_amd import _lib
    for name in _lib.KRYLOV_SIGNATURES:
        assert _lib.entry(name) is None, name
