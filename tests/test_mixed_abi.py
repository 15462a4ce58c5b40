"""include/pgh_mixed.h at the C-ABI (no GPU): its table in _lib matches the header and is disjoint from the others, the Makefile builds
the engine against the header, the HIP library exports and binds both entries, and the host test double has neither."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")
ENTRIES = ["pgh_poly_run_batch_mixed", "pgh_ppr_run_batch_mixed"]


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


def test_mixed_header_table_and_makefile_agree():
    import ctypes as C
    from pygrank_amd import _lib
    assert sorted(_lib.MIXED_SIGNATURES) == _declared("pgh_mixed.h") == ENTRIES
    assert _lib.OPTIONAL["pgh_mixed.h"] is _lib.MIXED_SIGNATURES
    for header, other in [("pgh.h", _lib.SIGNATURES), *_lib.OPTIONAL.items()]:
        if header != "pgh_mixed.h":
            assert set(_lib.MIXED_SIGNATURES).isdisjoint(other), header
    assert _lib.DECLINED == _defined("pgh_mixed.h", "PGH_MIXED_DECLINED")
    cfg, res = C.POINTER(_lib.LoopCfg), C.POINTER(_lib.LoopResult)
    restype, argtypes = _lib.MIXED_SIGNATURES["pgh_ppr_run_batch_mixed"]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, cfg, C.c_void_p, C.c_void_p, res]
    restype, argtypes = _lib.MIXED_SIGNATURES["pgh_poly_run_batch_mixed"]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, cfg, C.c_void_p, res]
    # the uniform loops' signatures with one more pointer / the same shape: the parameter moved from cfg into an array
    assert len(_lib.SIGNATURES["pgh_ppr_run_batch"][1]) + 1 == len(_lib.MIXED_SIGNATURES["pgh_ppr_run_batch_mixed"][1])
    assert _lib.BATCH_SIGNATURES["pgh_poly_run_batch"] == _lib.MIXED_SIGNATURES["pgh_poly_run_batch_mixed"]
    makefile = open(os.path.join(ROOT, "pygrank_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bpgh_spmm\.hip\b", makefile, re.M)
    assert re.search(r"^_build/%\.o:.*include/pgh_mixed\.h\b", makefile, re.M)
    source = open(os.path.join(ROOT, "pygrank_amd", "csrc", "pgh_spmm.hip")).read()
    assert '#include "pgh_mixed.h"' in source
    for name in ENTRIES:
        assert re.search(r'extern "C" int ' + name + r"\(", source), name


def test_hip_library_exports_and_binds_the_mixed_entries(hip_lib):
    from pygrank_amd import _lib
    cdll = _lib.load_library(hip_lib)
    bound = _lib.bind_optional(cdll, _lib.MIXED_SIGNATURES)
    assert sorted(bound) == _declared("pgh_mixed.h")
    for name in _declared("pgh_mixed.h"):
        assert hasattr(cdll, name), name
        assert bound[name] is not None and bound[name].argtypes == _lib.MIXED_SIGNATURES[name][1], name


def test_host_double_has_no_mixed_entry(host_engine):
    from pygrank_amd import _lib
    for name in _lib.MIXED_SIGNATURES:
        assert _lib.entry(name) is None, name
