"""Ready-made families of graph filters to compare or to choose from (pygrank/benchmarks/comparables.py:6-113).

The filters of one family share their preprocessor (one uploaded graph image per normalisation), which is also what lets
``AlgorithmSelection`` run a family's PageRanks as one mixed batch and its closed-form filters as another (include/pgh_mixed.h).
``create_variations`` takes ``{"+SO": SeedOversampling, "+BSO": BoostedSeedOversampling}`` (pygrank_amd/oversampling.py) or the six
wrappers of ``create_many_variation_types``.  Its ``SweepO`` and ``SweepNeigh`` members hand ``SeedOversampling`` a wrapped ranker:
``Sweep.propagate`` keeps that ranker's batch (pygrank_amd/postprocess.py), so a round of seed sets is still one multi-seed run.
"""
from pygrank_amd.filters import AbsorbingWalks, HeatKernel, PageRank
from pygrank_amd.oversampling import SeedOversampling
from pygrank_amd.postprocess import Sweep, Tautology
from pygrank_amd.preprocessing import preprocessor as _preprocessor


def create_demo_filters(preprocessor=None, tol=1.E-9, max_iters=1000):
    """comparables.py:6-31: three PageRanks and three heat kernels on one immutable-graph preprocessor (automatic normalisation
    unless one is handed in).  The default tolerance lies below fp32 eps: these filters choose the engine's f64 loops."""
    pre = _preprocessor(assume_immutability=True) if preprocessor is None else preprocessor
    common = dict(preprocessor=pre, max_iters=max_iters, tol=tol)
    family = {}
    for name, alpha in (("PPR.85", 0.85), ("PPR.9", 0.9), ("PPR.95", 0.95)):
        family[name] = PageRank(alpha=alpha, **common)
    for t in (3, 5, 7):
        family[f"HK{t}"] = HeatKernel(t=t, **common)
    return family


def create_many_filters(tol=1.E-6, max_iters=10000):
    """comparables.py:34-77: PageRank and AbsorbingWalks at alpha 0.85 / 0.9 / 0.95 / 0.99 and HeatKernel at t 1 / 3 / 5 / 7, each on
    a column-normalised and on a symmetrically normalised ("L" in the name) immutable graph: 24 filters on two preprocessors."""
    pre = {"": _preprocessor("col", assume_immutability=True), "L": _preprocessor("symmetric", assume_immutability=True)}
    alphas = (("85", 0.85), ("90", 0.9), ("95", 0.95), ("99", 0.99))
    family = {}

    def add(stem, order, make):
        for tag in order:
            for suffix, value in make[0]:
                family[f"{stem}{tag}{make[1]}{suffix}"] = make[2](value, dict(preprocessor=pre[tag], max_iters=max_iters, tol=tol))
    add("PPR", ("L", ""), (alphas, ".", lambda alpha, kw: PageRank(alpha=alpha, **kw)))
    add("HK", ("", "L"), ((("1", 1), ("3", 3), ("5", 5), ("7", 7)), "", lambda t, kw: HeatKernel(t=t, **kw)))
    add("Absorb", ("L", ""), (alphas, ".", lambda alpha, kw: AbsorbingWalks(alpha=alpha, **kw)))
    return family


def create_many_variation_types():
    """comparables.py:80-87: name suffix -> callable(ranker) -> ranker: as it is, swept, seed-oversampled ("safe" and "neighbors"), and
    swept inside either oversampling."""
    return {"": Tautology,
            "Sweep": Sweep,
            "O": lambda ranker: SeedOversampling(ranker, "safe"),
            "SweepO": lambda ranker: SeedOversampling(Sweep(ranker), "safe"),
            "Neigh": lambda ranker: SeedOversampling(ranker, "neighbors"),
            "SweepNeigh": lambda ranker: SeedOversampling(Sweep(ranker), "neighbors")}


def create_variations(algorithms, variations):
    """comparables.py:90-113: every algorithm wrapped by every variation (a mapping name -> callable(ranker) -> ranker, or one such
    callable); the variation's name is appended to the algorithm's."""
    if callable(variations):
        variations = {"": variations}
    return {name + suffix: wrap(ranker) for suffix, wrap in variations.items() for name, ranker in algorithms.items()}
