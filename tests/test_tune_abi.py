"""include/pgh_tune.h at the C-ABI (no GPU): its table in _lib matches the header and is disjoint from the other two, the HIP
library exports and binds every entry, and the host test double has none of them."""
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


def test_tune_header_and_table_agree():
    from pygrank_amd import _lib
    assert sorted(_lib.TUNE_SIGNATURES) == _declared("pgh_tune.h")
    assert _lib.OPTIONAL["pgh_tune.h"] is _lib.TUNE_SIGNATURES
    for header, other in [("pgh.h", _lib.SIGNATURES), *_lib.OPTIONAL.items()]:
        if header != "pgh_tune.h":
            assert set(_lib.TUNE_SIGNATURES).isdisjoint(other), header
    assert sorted(_lib.SIGNATURES) == _declared("pgh.h")
    assert sorted(_lib.BATCH_SIGNATURES) == _declared("pgh_batch.h")
    assert _lib.DECLINED == _defined("pgh_tune.h", "PGH_TUNE_DECLINED")
    assert _lib.TUNE_LDS_BYTES == _defined("pgh_tune.h", "PGH_TUNE_LDS_BYTES")
    assert _lib.TUNE_MAX_POSITIVES == _defined("pgh_tune.h", "PGH_TUNE_MAX_POSITIVES")


def test_hip_library_exports_and_binds_the_tune_entries(hip_lib):
    from pygrank_amd import _lib
    cdll = _lib.load_library(hip_lib)
    bound = _lib.bind_optional(cdll, _lib.TUNE_SIGNATURES)
    assert sorted(bound) == _declared("pgh_tune.h")
    for name in _declared("pgh_tune.h"):
        assert hasattr(cdll, name), name
        assert bound[name] is not None and bound[name].argtypes == _lib.TUNE_SIGNATURES[name][1], name


def test_host_double_has_no_tune_entry(host_engine):
    from pygrank_amd import _lib
    for name in _lib.TUNE_SIGNATURES:
        assert _lib.entry(name) is None, name
