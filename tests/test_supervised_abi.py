"""include/pgh_supervised.h at the C-ABI (no GPU): its table in _lib matches the header (entries, argument counts, constants) and is
disjoint from the other four, the HIP library exports and binds the entry, and the host test double does not have it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")
HEADER = "pgh_supervised.h"


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _code(name):
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)


def _declared(name):
    return sorted(set(re.findall(r"\b(pgh_[a-z0-9_]+)\s*\(", _code(name))))


def _argument_count(name, entry):
    arguments = re.search(r"\b" + entry + r"\s*\(([^)]*)\)", _code(name)).group(1).strip()
    return 0 if arguments in ("", "void") else arguments.count(",") + 1


def _defined(name, macro):
    return int(re.search(r"#define\s+" + macro + r"\s+(\d+)", _header(name)).group(1))


@pytest.fixture(scope="module")
def hip_lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pygrank_amd", "csrc")])
    return LIB


def test_supervised_header_and_table_agree():
    from pygrank_amd import _lib
    assert sorted(_lib.SUPERVISED_SIGNATURES) == _declared(HEADER) == ["pgh_pair_forms"]
    for entry, (restype, argtypes) in _lib.SUPERVISED_SIGNATURES.items():
        assert len(argtypes) == _argument_count(HEADER, entry), entry
    assert len(_lib.SUPERVISED_SIGNATURES["pgh_pair_forms"][1]) == 9
    assert _lib.OPTIONAL[HEADER] is _lib.SUPERVISED_SIGNATURES
    for header, other in [("pgh.h", _lib.SIGNATURES), *_lib.OPTIONAL.items()]:
        if header != HEADER:
            assert set(_lib.SUPERVISED_SIGNATURES).isdisjoint(other), header
    assert _lib.DECLINED == _defined(HEADER, "PGH_PAIR_DECLINED")
    assert _lib.PAIR_SLOTS == _defined(HEADER, "PGH_PAIR_SLOTS") == 20
    assert _lib.PAIR_MOMENTS == _defined(HEADER, "PGH_PAIR_MOMENTS")
    assert _lib.PAIR_LOGS == _defined(HEADER, "PGH_PAIR_LOGS")
    # pgh.h keeps its own table: nothing of this header leaked into it
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(pgh_[a-z0-9_]+)\s*\(", _header("pgh.h"))))


def test_hip_library_exports_and_binds_the_supervised_entry(hip_lib):
    from pygrank_amd import _lib
    cdll = _lib.load_library(hip_lib)
    bound = _lib.bind_optional(cdll, _lib.SUPERVISED_SIGNATURES)
    assert sorted(bound) == _declared(HEADER)
    for name in _declared(HEADER):
        assert hasattr(cdll, name), name
        assert bound[name] is not None and bound[name].argtypes == _lib.SUPERVISED_SIGNATURES[name][1], name


def test_host_double_has_no_supervised_entry(host_engine):
    from pygrank_amd import _lib
    for name in _lib.SUPERVISED_SIGNATURES:
        assert _lib.entry(name) is None, name
