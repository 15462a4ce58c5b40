"""include/pgh_rank.h at the C-ABI (no GPU): its table in _lib matches the header (entries, argument counts, constants) and is disjoint
from the other tables, the HIP library exports and binds the entries, and the host test double does not have them."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pygrank_amd", "csrc", "libpgh_hip.so")
HEADER = "pgh_rank.h"
ENTRIES = ["pgh_ndcg", "pgh_ndcg_vec", "pgh_rank_plan_create", "pgh_rank_plan_destroy", "pgh_rank_plan_info", "pgh_spearman",
           "pgh_spearman_vec"]


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


def test_rank_header_and_table_agree():
    from pygrank_amd import _lib
    assert sorted(_lib.RANK_SIGNATURES) == _declared(HEADER) == ENTRIES
    for entry, (restype, argtypes) in _lib.RANK_SIGNATURES.items():
        assert len(argtypes) == _argument_count(HEADER, entry), entry
    assert len(_lib.RANK_SIGNATURES["pgh_ndcg"][1]) == 6 and len(_lib.RANK_SIGNATURES["pgh_spearman"][1]) == 3
    assert _lib.OPTIONAL[HEADER] is _lib.RANK_SIGNATURES
    for header, other in [("pgh.h", _lib.SIGNATURES), *_lib.OPTIONAL.items()]:
        if header != HEADER:
            assert set(_lib.RANK_SIGNATURES).isdisjoint(other), header
    assert _lib.DECLINED == _defined(HEADER, "PGH_RANK_DECLINED") == 2
    assert _lib.RANK_MAX_RELEVANT == _defined(HEADER, "PGH_RANK_MAX_RELEVANT") == 8192
    assert _lib.RANK_LDS_BYTES == _defined(HEADER, "PGH_RANK_LDS_BYTES")
    assert (_lib.RANK_AUTO, _lib.RANK_STREAMING, _lib.RANK_SORTED) == tuple(
        _defined(HEADER, "PGH_RANK_" + name) for name in ("AUTO", "STREAMING", "SORTED"))
    # pgh.h keeps its own table: nothing of this header leaked into it
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(pgh_[a-z0-9_]+)\s*\(", _header("pgh.h"))))


def test_hip_library_exports_and_binds_the_rank_entries(hip_lib):
    from pygrank_amd import _lib
    cdll = _lib.load_library(hip_lib)
    bound = _lib.bind_optional(cdll, _lib.RANK_SIGNATURES)
    assert sorted(bound) == _declared(HEADER)
    for name in _declared(HEADER):
        assert hasattr(cdll, name), name
        assert bound[name] is not None and bound[name].argtypes == _lib.RANK_SIGNATURES[name][1], name


def test_the_package_exports_the_new_measures():
    import pygrank_amd as pg
    from pygrank_amd import combination, measures
    for name in ("NDCG", "SpearmanCorrelation", "MeasureCombination", "AM", "GM", "Disparity", "Parity"):
        assert getattr(pg, name) is getattr(measures, name), name
    for name in ("MeasureCombination", "AM", "GM", "Disparity", "Parity"):
        assert getattr(pg, name) is getattr(combination, name), name
    assert issubclass(pg.NDCG, pg.Supervised) and issubclass(pg.SpearmanCorrelation, pg.Supervised)


def test_host_double_has_no_rank_entry(host_engine):
    from pygrank_amd import _lib
    for name in _lib.RANK_SIGNATURES:
        assert _lib.entry(name) is None, name
