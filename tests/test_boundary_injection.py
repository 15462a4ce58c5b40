"""The drop-in boundary, proven on the reference's own code: tests/golden/make_boundary_injection.py (run where
the reference is installed) registers pygrank_amd/backend/hip.py in the unmodified reference loader and runs the reference's
PageRank / HeatKernel / AbsorbingWalks / SymmetricAbsorbingRandomWalks on it; this test holds the committed outcome to equal
iteration counts and <= 1e-6 relative L-inf against the reference's numpy backend."""
import json
import os

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load():
    with open(os.path.join(HERE, "boundary_injection.json")) as f:
        return json.load(f)


def test_committed_injection_results():
    data = _load()
    cases = {k: v for k, v in data.items() if not k.startswith("_")}
    assert len(cases) >= 16 and data["_meta"]["slot"] == "matvec"
    for name, row in cases.items():
        assert row["iterations_injected"] == row["iterations_numpy"], name
        assert row["rel_linf"] <= 1e-6, (name, row["rel_linf"])
    kinds = {name.split("/")[1].split("_")[0] for name in cases}
    assert {"pagerank", "heat", "absorbing", "sarw"} <= kinds

