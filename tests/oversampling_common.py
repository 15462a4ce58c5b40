"""Shared by the seed oversampling tests: include/pgh_oversample.h in numpy f64 from f32 operands (what the GPU kernels are compared
with), the cases of tests/golden/golden_oversampling.npz (make_golden_oversampling.py) and how one of them is run through
pg.SeedOversampling / pg.BoostedSeedOversampling."""
import os

import numpy as np

import cases
from parity_common import rel_linf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = ["er10k", "rmat12_sym", "rmat10_dir", "weighted300"]
RANKER = dict(alpha=0.9, tol=1e-6, max_iters=1000)             # error_type=L1 is added where the package is at hand
SO_METHODS = ["safe", "top", "neighbors"]
BOOSTED = [("partial", "previous"), ("naive", "original")]
TIGHT = ("rmat10_dir", "partial", "previous")                  # the case the fixture also holds around PageRank(tol=1e-9)
MULTI = "rmat10_dir"                                           # the graph of the three-column propagate case
BAR = 1e-6                                                     # the project's bar

_fixture = None
_graphs = {}


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = np.load(os.path.join(ROOT, "tests", "golden", "golden_oversampling.npz"))
    return _fixture


def graph_of(key):
    if key not in _graphs:
        _graphs[key] = cases.GRAPHS[key]()
    return _graphs[key]


def bar_of(stem):
    """The bar of a case: the project's, or 4x the emulation's own error where the fixture records one above it."""
    fx = fixture()
    name = stem + "/emulation_rel_linf"
    return max(BAR, 4.0 * float(fx[name])) if name in fx.files else BAR


class Case:
    def __init__(self, pg, key):
        A, directed, p = graph_of(key)
        self.pg, self.key, self.n = pg, key, A.shape[0]
        self.graph = pg.AdjacencyWrapper(A, directed=directed)
        self.seeds = {int(v): 1.0 for v in np.flatnonzero(p)}

    def ranker(self, **kwargs):
        pg = self.pg
        return pg.PageRank(error_type=pg.L1, **{**RANKER, **kwargs})

    def signal(self, stem=None, tag=""):
        """The graph's own seeds as ones, or the seed set the fixture records beside the case `stem`."""
        fx = fixture()
        if stem is not None and stem + "/nodes" + tag in fx.files:
            return self.pg.to_signal(self.graph, {int(v): 1.0 for v in fx[stem + "/nodes" + tag]})
        return self.pg.to_signal(self.graph, self.seeds)

    def seed_oversampling(self, method, **kwargs):
        algo = self.pg.SeedOversampling(self.ranker(), method, **kwargs)
        return algo, np.asarray(algo.rank(self.graph, self.signal(f"{self.key}/so_{method}")).np, dtype=np.float64)

    def boosted(self, objective, source, ranker=None, tag="", **kwargs):
        algo = self.pg.BoostedSeedOversampling(self.ranker() if ranker is None else ranker, objective, source, **kwargs)
        return algo, np.asarray(algo.rank(self.graph, self.signal(f"{self.key}/bso_{objective}_{source}", tag)).np, dtype=np.float64)

    def check_seed_oversampling(self, method, **kwargs):
        fx, stem = fixture(), f"{self.key}/so_{method}"
        algo, got = self.seed_oversampling(method, **kwargs)
        worst = rel_linf(got, fx[stem + "/ranks"])
        print(stem, kwargs, "rel-Linf", worst, "seeds", algo.last_seed_counts, "reference", int(fx[stem + "/seeds"]))
        assert list(algo.last_seed_counts) == [int(fx[stem + "/seeds"])]
        assert worst <= bar_of(stem), (stem, worst)
        return algo, got

    def check_boosted(self, objective, source, tag="", **kwargs):
        """tag "_tol1e-9": the fixture's run around PageRank(tol=1e-9), hand the matching ranker in."""
        fx, stem = fixture(), f"{self.key}/bso_{objective}_{source}"
        algo, got = self.boosted(objective, source, tag=tag, **kwargs)
        worst = rel_linf(got, fx[stem + "/ranks" + tag])
        print(stem + tag, kwargs, "rel-Linf", worst, "rounds", algo.last_rounds, "reference", int(fx[stem + "/rounds" + tag]), "seeds",
              algo.last_seed_counts, "weights", algo.last_weights)
        assert list(algo.last_rounds) == [int(fx[stem + "/rounds" + tag])]
        assert [int(c) for c in algo.last_seed_counts[0]] == [int(c) for c in fx[stem + "/seeds" + tag]]
        # the weights are continuous in the ranks: 1e-5 is the margin the fixture keeps between a weight step and its tolerance
        assert np.allclose(algo.last_weights[0], fx[stem + "/weights" + tag], rtol=0, atol=1e-5)
        assert worst <= (BAR if tag else bar_of(stem)), (stem, worst)
        return algo, got


def multi_features(key=MULTI):
    """The three seed sets of the fixture's propagate case, as an [n, 3] array of zeros and ones."""
    fx = fixture()
    n = graph_of(key)[0].shape[0]
    F = np.zeros((n, 3))
    for j in range(3):
        F[fx[f"{key}/multi/seeds{j}"], j] = 1.0
    return F


# ---- include/pgh_oversample.h in numpy f64 over f32-valued operands
def seed_floor(ranks, seeds):
    ranks, seeds = np.asarray(ranks, dtype=np.float64), np.asarray(seeds, dtype=np.float64)
    hit = seeds == 1.0
    floors = np.array([ranks[hit[:, c], c].min() if hit[:, c].any() else np.inf for c in range(ranks.shape[1])])
    return floors, hit.sum(axis=0).astype(np.int64)


def seed_resample(ranks, floors, strict, keep):
    ranks32 = np.asarray(ranks, dtype=np.float32)
    floors32 = np.asarray(floors, dtype=np.float32)[None, :]
    out = (ranks32 > floors32) if strict else (ranks32 >= floors32)
    if keep is not None:
        out = out | (np.asarray(keep) == 1.0)
    return out.astype(np.float64), out.sum(axis=0).astype(np.int64)


def boost_forms(seeds, fresh, total):
    s, R, RN = (np.asarray(v, dtype=np.float64) for v in (seeds, fresh, total))
    return np.stack([(s * (R * R)).sum(axis=0), (R * R).sum(axis=0), ((s * RN) * R).sum(axis=0)], axis=1)


def boost_update(total, fresh, weights, mask):
    """(the new total before the store's rounding, floors and counts over its f32 rounding)."""
    t, R = np.asarray(total, dtype=np.float64), np.asarray(fresh, dtype=np.float64)
    new = t + np.asarray(weights, dtype=np.float64)[None, :] * R
    floors, counts = seed_floor(new.astype(np.float32), mask)
    return new, floors, counts


def numpy_entries(lib):
    """{name: callable} with the signatures of include/pgh_oversample.h, evaluated in numpy through the slab transfers of `lib`: stand-ins
    that let the fused route of the two postprocessors run on the host test double."""
    import ctypes as C

    def down(h):
        n, b = C.c_int64(), C.c_int32()
        assert lib.pgh_mat_shape(h, C.byref(n), C.byref(b)) == 0
        out = np.empty((n.value, b.value), dtype=np.float64)
        assert lib.pgh_mat_d2h_f64(h, out.ctypes.data_as(C.c_void_p)) == 0
        return out

    def up(h, values):
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert lib.pgh_mat_h2d_f64(h, values.ctypes.data_as(C.c_void_p)) == 0

    def give(floors, counts, floor_host, count_host):
        for c in range(len(counts)):
            if floor_host is not None:
                floor_host[c] = floors[c]
            count_host[c] = int(counts[c])

    def floor(ranks, seeds, floor_host, count_host):
        give(*seed_floor(down(ranks), down(seeds)), floor_host, count_host)
        return 0

    def resample(ranks, floor_host, strict, keep, out, count_host):
        r = down(ranks)
        grown, counts = seed_resample(r, [floor_host[c] for c in range(r.shape[1])], strict, None if keep is None else down(keep))
        up(out, grown)
        give(None, counts, None, count_host)
        return 0

    def forms(seeds, fresh, total, forms_host):
        got = boost_forms(down(seeds), down(fresh), down(total))
        for k, value in enumerate(got.ravel()):
            forms_host[k] = float(value)
        return 0

    def update(total, fresh, weights_host, mask, floor_host, count_host):
        t = down(total)
        new, floors, counts = boost_update(t, down(fresh), [weights_host[c] for c in range(t.shape[1])], down(mask))
        up(total, new.astype(np.float32))
        give(floors, counts, floor_host, count_host)
        return 0
    return dict(pgh_seed_floor=floor, pgh_seed_resample=resample, pgh_boost_forms=forms, pgh_boost_update=update)
