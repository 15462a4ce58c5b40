"""include/pgh_post.h at the C-ABI (no GPU): its table in _lib matches the header and is disjoint from the others, the Makefile
builds its source against the header, the HIP library exports and binds all five entries, and the host test double has none."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")
ENTRIES = ["pgh_post_col_affine", "pgh_post_col_threshold", "pgh_post_kth_largest", "pgh_post_ordinals", "pgh_post_row_op"]


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


def test_post_header_table_and_makefile_agree():
    import ctypes as C
    from pygrank_amd import _lib
    assert sorted(_lib.POST_SIGNATURES) == _declared("pgh_post.h") == ENTRIES
    assert _lib.OPTIONAL["pgh_post.h"] is _lib.POST_SIGNATURES
    for header, other in [("pgh.h", _lib.SIGNATURES), *_lib.OPTIONAL.items()]:
        if header != "pgh_post.h":
            assert set(_lib.POST_SIGNATURES).isdisjoint(other), header
            assert set(ENTRIES).isdisjoint(_declared(header)), header
    assert _lib.DECLINED == _defined("pgh_post.h", "PGH_POST_DECLINED") == 2
    assert _lib.POST_MAX_COLS == _defined("pgh_post.h", "PGH_POST_MAX_COLS") == 64
    assert _lib.POST_ROW_SUB == _defined("pgh_post.h", "PGH_POST_ROW_SUB")
    assert _lib.POST_ROW_SWEEP == _defined("pgh_post.h", "PGH_POST_ROW_SWEEP")
    mat, vec, f64p = C.c_void_p, C.c_void_p, C.POINTER(C.c_double)
    want = dict(pgh_post_kth_largest=[mat, C.c_int64, f64p],
                pgh_post_col_threshold=[mat, f64p, C.c_int32, mat],
                pgh_post_col_affine=[mat, f64p, f64p, mat],
                pgh_post_row_op=[mat, vec, C.c_int32, C.c_double, mat],
                pgh_post_ordinals=[mat, mat])
    for name, (restype, argtypes) in _lib.POST_SIGNATURES.items():
        assert restype is C.c_int and argtypes == want[name], name
    makefile = open(os.path.join(ROOT, "pygrank_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bpgh_post\.hip\b", makefile, re.M)
    assert re.search(r"^_build/%\.o:.*include/pgh_post\.h\b", makefile, re.M)


def test_hip_library_exports_and_binds_the_post_entries(hip_lib):
    from pygrank_amd import _lib
    cdll = _lib.load_library(hip_lib)
    bound = _lib.bind_optional(cdll, _lib.POST_SIGNATURES)
    assert sorted(bound) == ENTRIES
    for name in ENTRIES:
        assert hasattr(cdll, name), name
        assert bound[name] is not None and bound[name].argtypes == _lib.POST_SIGNATURES[name][1], name


def test_host_double_has_no_post_entry(host_engine):
    from pygrank_amd import _lib
    for name in _lib.POST_SIGNATURES:
        assert _lib.entry(name) is None, name
