"""include/pgh_oversample.h at the C-ABI (no GPU): its table in _lib matches the header and is disjoint from the others, the Makefile
builds its source against the header, the HIP library exports and binds all four entries, and the host test double has none."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")
ENTRIES = ["pgh_boost_forms", "pgh_boost_update", "pgh_seed_floor", "pgh_seed_resample"]


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


def test_oversample_header_table_and_makefile_agree():
    import ctypes as C
    from pygrank_amd import _lib
    assert sorted(_lib.OVERSAMPLE_SIGNATURES) == _declared("pgh_oversample.h") == ENTRIES
    assert _lib.OPTIONAL["pgh_oversample.h"] is _lib.OVERSAMPLE_SIGNATURES
    for header, other in [("pgh.h", _lib.SIGNATURES), *_lib.OPTIONAL.items()]:
        if header != "pgh_oversample.h":
            assert set(_lib.OVERSAMPLE_SIGNATURES).isdisjoint(other), header
            assert set(ENTRIES).isdisjoint(_declared(header)), header
    assert _lib.DECLINED == _defined("pgh_oversample.h", "PGH_OVERSAMPLE_DECLINED")
    assert _lib.OVERSAMPLE_MAX_COLS == _defined("pgh_oversample.h", "PGH_OVERSAMPLE_MAX_COLS") == 64
    mat, f64p, i64p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)
    want = dict(pgh_seed_floor=[mat, mat, f64p, i64p],
                pgh_seed_resample=[mat, f64p, C.c_int32, mat, mat, i64p],
                pgh_boost_forms=[mat, mat, mat, f64p],
                pgh_boost_update=[mat, mat, f64p, mat, f64p, i64p])
    for name, (restype, argtypes) in _lib.OVERSAMPLE_SIGNATURES.items():
        assert restype is C.c_int and argtypes == want[name], name
    makefile = open(os.path.join(ROOT, "pygrank_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bpgh_oversample\.hip\b", makefile, re.M)
    assert re.search(r"^_build/%\.o:.*include/pgh_oversample\.h\b", makefile, re.M)


def test_hip_library_exports_and_binds_the_oversample_entries(hip_lib):
    from pygrank_amd import _lib
    cdll = _lib.load_library(hip_lib)
    bound = _lib.bind_optional(cdll, _lib.OVERSAMPLE_SIGNATURES)
    assert sorted(bound) == ENTRIES
    for name in ENTRIES:
        assert hasattr(cdll, name), name
        assert bound[name] is not None and bound[name].argtypes == _lib.OVERSAMPLE_SIGNATURES[name][1], name


def test_host_double_has_no_oversample_entry(host_engine):
    from pygrank_amd import _lib
    for name in _lib.OVERSAMPLE_SIGNATURES:
        assert _lib.entry(name) is None, name
