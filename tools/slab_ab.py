"""Diagnostic: feed two builds of the engine the same seeded inputs through every slab-measure entry point (include/pgh_tune.h,
pgh_measure.h, pgh_supervised.h, pgh_fair.h, pgh_lfpr.h, pgh_oversample.h, pgh_rank.h, pgh_krylov.h, pgh_link.h) and compare every
output array and scalar bit for bit.  Raw ctypes, one process.  The shapes sit at the part, wavefront and quad edges the kernel tests
use; the inputs hold a tie group, a -0.0, a NaN column (rank entries) and an all-excluded label vector.
Usage: python tools/slab_ab.py old/libpgh_hip.so pygrank_amd/csrc/libpgh_hip.so"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pygrank_amd import _lib as L  # noqa: E402

NS = (1, 65, 4099, 262147)
BS = (1, 3, 33, 64)
KS = (1, 5, 64)            # probes / terms
TABLES = (L.SIGNATURES, L.TUNE_SIGNATURES, L.MEASURE_SIGNATURES, L.SUPERVISED_SIGNATURES, L.FAIR_SIGNATURES, L.LFPR_SIGNATURES,
          L.OVERSAMPLE_SIGNATURES, L.RANK_SIGNATURES, L.KRYLOV_SIGNATURES, L.LINK_SIGNATURES)


def bind(path):
    cdll = C.CDLL(os.path.abspath(path))
    for table in TABLES:
        for name, (restype, argtypes) in table.items():
            fn = getattr(cdll, name)
            fn.restype, fn.argtypes = restype, argtypes
    return cdll


def ptr(a, kind=C.c_void_p):
    return a.ctypes.data_as(kind)


def f64(a):
    return ptr(a, L.c_f64p)


def i64(a):
    return ptr(a, L.c_i64p)


class Engine:
    """One library, its device buffers, and the record of everything it returned."""

    def __init__(self, lib):
        self.lib, self.out, self.vecs, self.mats = lib, {}, [], []
        self.ok(lib.pgh_init(0))

    def ok(self, status):
        if status != 0:
            raise RuntimeError(self.lib.pgh_last_error().decode())

    def status(self, status):
        """a status that may be a refusal: recorded with its text"""
        return np.frombuffer(f"{status}:{self.lib.pgh_last_error().decode() if status else ''}".encode(), dtype=np.uint8)

    def vec(self, host):
        host = np.ascontiguousarray(host, dtype=np.float32)
        h = L.c_vec()
        self.ok(self.lib.pgh_vec_alloc(host.size, C.byref(h)))
        self.ok(self.lib.pgh_vec_h2d_f32(h, ptr(host), host.size))
        self.vecs.append(h)
        return h

    def mat(self, host):
        host = np.ascontiguousarray(host, dtype=np.float64)
        h = L.c_mat()
        self.ok(self.lib.pgh_mat_alloc(host.shape[0], host.shape[1], C.byref(h)))
        self.ok(self.lib.pgh_mat_h2d_f64(h, ptr(host)))
        self.mats.append(h)
        return h

    def vec_host(self, h, n):
        got = np.empty(n, dtype=np.float32)
        self.ok(self.lib.pgh_vec_d2h_f32(h, ptr(got), n))
        return got

    def mat_host(self, h, n, b):
        got = np.empty((n, b), dtype=np.float64)
        self.ok(self.lib.pgh_mat_d2h_f64(h, ptr(got)))
        return got

    def free(self):
        for h in self.vecs:
            self.lib.pgh_vec_free(h)
        for h in self.mats:
            self.lib.pgh_mat_free(h)
        self.vecs, self.mats = [], []


def slab(rng, n, b):
    """scores in (0, 1) as f32 values: a tie group in the first rows, a -0.0"""
    s = rng.random((n, b)).astype(np.float32)
    s[: min(n, 5), :] = np.float32(0.5)
    s[n // 2, 0] = np.float32(-0.0)
    return s


def labels(rng, n):
    known = np.where(rng.random(n) < min(0.3, 3000.0 / n), rng.random(n), 0.0).astype(np.float32)   # (the per-column sorts hold 8192)
    known[0] = np.float32(0.75)                       # at least one positive and, below, one negative
    if n > 1:
        known[n - 1] = 0.0
    exclude = (rng.random(n) < 0.2).astype(np.float32)
    exclude[0] = 0.0
    if n > 1:
        exclude[n - 1] = 0.0
    return known, exclude


def run_measure(e, rng):
    lib = e.lib
    for n in NS:
        for b in BS:
            out = np.zeros(4 * b)
            e.ok(lib.pgh_mat_col_stats(e.mat(slab(rng, n, b)), ptr(out)))
            e.out[f"pgh_mat_col_stats n={n} b={b}"] = [out]
        e.free()
    g = L.c_graph()
    e.ok(lib.pgh_graph_rmat(10, 16, 0.57, 0.19, 0.19, 0, L.NORM_COL, 1, 0, 0, C.byref(g)))
    n = 1 << 10
    for b in BS:
        scores = e.mat(slab(rng, n, b))
        factors = rng.random(b) + 0.5
        for forms in (L.CUT_ALL, L.CUT_INTERNAL):
            out = np.zeros(4 * b)
            st = e.status(lib.pgh_cut_forms(g, scores, ptr(factors), 1.0, forms, ptr(out)))
            e.out[f"pgh_cut_forms n={n} b={b} forms={forms}"] = [st, out]
    e.free()
    lib.pgh_graph_destroy(g)


def run_pairs(e, rng):
    lib = e.lib
    for n in NS:
        for b in BS:
            s = e.mat(slab(rng, n, b))
            known, exclude = labels(rng, n)
            kv, xv = e.vec(known), e.vec(exclude)
            km = e.mat(np.where(rng.random((n, b)) < 0.3, rng.random((n, b)), 0.0).astype(np.float32))
            xm = e.mat((rng.random((n, b)) < 0.2).astype(np.float32))
            factors = rng.random(b) + 0.5
            for groups in (L.PAIR_MOMENTS, L.PAIR_LOGS):
                for tag, args in (("vec", (kv, None, None, None)), ("vec+ex", (kv, None, xv, None)), ("slab", (None, km, None, None)),
                                  ("slab+ex", (None, km, None, xm))):
                    out = np.zeros(L.PAIR_SLOTS * b)
                    e.ok(lib.pgh_pair_forms(s, *args, ptr(factors), 1e-12, groups, ptr(out)))
                    e.out[f"pgh_pair_forms n={n} b={b} groups={groups} known={tag}"] = [out]
            e.free()


def run_probe(e, rng):
    lib = e.lib
    for n in NS:
        known, exclude = labels(rng, n)
        cases = [("plain", known, None), ("exclude", known, exclude), ("all-excluded", known, np.ones(n, dtype=np.float32))]
        for tag, k, x in cases:
            plan = L.c_plan()
            e.ok(lib.pgh_probe_plan_create(e.vec(k), None if x is None else e.vec(x), C.byref(plan)))
            pos, neg = C.c_int64(), C.c_int64()
            e.ok(lib.pgh_probe_plan_info(plan, C.byref(pos), C.byref(neg)))
            e.out[f"pgh_probe_plan n={n} {tag}"] = [np.array([pos.value, neg.value])]
            for b in BS:
                s = e.mat(slab(rng, n, b))
                for terms in KS:
                    for probes in KS:
                        if terms > b:
                            continue
                        coeffs = rng.standard_normal(terms * probes)
                        auc = np.zeros(probes)
                        st = e.status(lib.pgh_probe_auc(s, ptr(coeffs), terms, probes, plan, f64(auc)))
                        e.out[f"pgh_probe_auc n={n} b={b} terms={terms} probes={probes} {tag}"] = [st, auc]
            lib.pgh_probe_plan_destroy(plan)
            e.free()


def run_rank(e, rng):
    lib = e.lib
    for n in NS:
        known, exclude = labels(rng, n)
        negative = known.copy()
        negative[n // 2] = np.float32(-0.25)
        cases = [("plain", known, None), ("exclude", known, exclude), ("negative", negative, exclude),
                 ("all-excluded", known, np.ones(n, dtype=np.float32))]
        for tag, k, x in cases:
            plan = L.c_rank_plan()
            e.ok(lib.pgh_rank_plan_create(e.vec(k), None if x is None else e.vec(x), C.byref(plan)))
            kept, rel, neg = C.c_int64(), C.c_int64(), C.c_int32()
            e.ok(lib.pgh_rank_plan_info(plan, C.byref(kept), C.byref(rel), C.byref(neg)))
            e.out[f"pgh_rank_plan n={n} {tag}"] = [np.array([kept.value, rel.value, neg.value])]
            for b in BS:
                host = slab(rng, n, b)
                host[n // 3, b - 1] = np.nan                   # one NaN column
                s = e.mat(host)
                for route in (L.RANK_STREAMING, L.RANK_SORTED):
                    dcg, idcg = np.zeros(b), np.zeros(1)
                    st = e.status(lib.pgh_ndcg(s, plan, max(1, n // 2), route, f64(dcg), f64(idcg)))
                    e.out[f"pgh_ndcg n={n} b={b} route={route} {tag}"] = [st, dcg, idcg]
                rho = np.zeros(b)
                st = e.status(lib.pgh_spearman(s, plan, f64(rho)))
                e.out[f"pgh_spearman n={n} b={b} {tag}"] = [st, rho]
            v = e.vec(slab(rng, n, 1)[:, 0])
            dcg, idcg, rho = np.zeros(1), np.zeros(1), np.zeros(1)
            st = e.status(lib.pgh_ndcg_vec(v, plan, n, L.RANK_AUTO, f64(dcg), f64(idcg)))
            st2 = e.status(lib.pgh_spearman_vec(v, plan, f64(rho)))
            e.out[f"pgh_ndcg_vec pgh_spearman_vec n={n} {tag}"] = [st, dcg, idcg, st2, rho]
            lib.pgh_rank_plan_destroy(plan)
            e.free()


def run_oversample(e, rng):
    lib = e.lib
    for n in NS:
        for b in BS:
            ranks_host = slab(rng, n, b)
            seeds_host = (rng.random((n, b)) < 0.1).astype(np.float32)
            seeds_host[0, :] = 1.0
            ranks, seeds = e.mat(ranks_host), e.mat(seeds_host)
            floor, count = np.zeros(b), np.zeros(b, dtype=np.int64)
            e.ok(lib.pgh_seed_floor(ranks, seeds, f64(floor), i64(count)))
            e.out[f"pgh_seed_floor n={n} b={b}"] = [floor, count]
            for strict in (0, 1):
                for keep in (None, seeds):
                    out, ones = e.mat(np.zeros((n, b))), np.zeros(b, dtype=np.int64)
                    e.ok(lib.pgh_seed_resample(ranks, f64(floor), strict, keep, out, i64(ones)))
                    e.out[f"pgh_seed_resample n={n} b={b} strict={strict} keep={keep is not None}"] = [ones, e.mat_host(out, n, b)]
            fresh, total = e.mat(slab(rng, n, b)), e.mat(slab(rng, n, b))
            forms = np.zeros(3 * b)
            e.ok(lib.pgh_boost_forms(seeds, fresh, total, f64(forms)))
            e.out[f"pgh_boost_forms n={n} b={b}"] = [forms]
            weights = rng.random(b) + 0.25
            e.ok(lib.pgh_boost_update(total, fresh, f64(weights), seeds, f64(floor), i64(count)))
            e.out[f"pgh_boost_update n={n} b={b}"] = [floor.copy(), count.copy(), e.mat_host(total, n, b)]
            e.free()


def run_lfpr(e, rng):
    lib = e.lib
    for n in NS:
        sens = (rng.random(n) < 0.4).astype(np.float32)
        out_r, out_b = rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)
        out_r[0] = 0.0
        orig = rng.random(n).astype(np.float32)
        ins = [e.vec(a) for a in (sens, out_r, out_b, orig)]
        outs = [e.vec(np.zeros(n)) for _ in range(5)]
        for with_orig in (True, False):
            sums = np.zeros(2)
            e.ok(lib.pgh_lfpr_setup(ins[0], ins[1], ins[2], ins[3] if with_orig else None, 0.4, *outs, f64(sums)))
            e.out[f"pgh_lfpr_setup n={n} original={with_orig}"] = [sums] + [e.vec_host(h, n) for h in outs]
        y0, x = e.vec(rng.random(n)), e.vec(rng.random(n))
        y, u = e.vec(np.zeros(n)), e.vec(np.zeros(n))
        for kind in (L.ERR_MABS, L.ERR_LINF):
            sums = np.zeros(5)
            e.ok(lib.pgh_lfpr_close(y0, x, 0.5, outs[3], outs[4], outs[0], outs[1], outs[2], 0.3, 0.2, 0.9, kind, y, u, f64(sums)))
            e.out[f"pgh_lfpr_close n={n} err_kind={kind}"] = [sums, e.vec_host(y, n), e.vec_host(u, n)]
        e.free()


def run_krylov(e, rng):
    lib = e.lib
    for n in NS:
        w, v, u = (e.vec(rng.standard_normal(n)) for _ in range(3))
        out = e.vec(np.zeros(n))
        for b in BS:
            basis = e.mat(slab(rng, n, b))
            for with_u in (True, False):
                for with_basis in (True, False):
                    sums = np.zeros(2)
                    e.ok(lib.pgh_lanczos_close(w, v, 0.7, u if with_u else None, 0.3, out, basis if with_basis else None, b - 1, f64(sums)))
                    e.out[f"pgh_lanczos_close n={n} b={b} u={with_u} basis={with_basis}"] = [sums, e.vec_host(out, n), e.mat_host(basis, n, b)]
            for count in KS:
                for probes in KS:
                    if count > b:
                        continue
                    deltas = rng.standard_normal(count * probes)
                    abssum, absmax = np.zeros(probes), np.zeros(probes)
                    e.ok(lib.pgh_krylov_residuals(basis, f64(deltas), count, probes, f64(abssum), f64(absmax)))
                    e.out[f"pgh_krylov_residuals n={n} b={b} count={count} probes={probes}"] = [abssum, absmax]
        e.free()


def run_link(e, rng):
    lib = e.lib
    for n in NS:
        pairs = min(4 * n + 3, 70001)
        first = rng.integers(0, n, pairs).astype(np.int32)
        second = rng.integers(0, n, pairs).astype(np.int32)
        label = (rng.random(pairs) < 0.4).astype(np.uint8)
        label[0], label[pairs - 1] = 1, 0
        plan = L.c_link_plan()
        e.ok(lib.pgh_link_plan_create(n, pairs, ptr(first, L.c_i32p), ptr(second, L.c_i32p), ptr(label, C.POINTER(C.c_uint8)), C.byref(plan)))
        for b in BS:
            host = slab(rng, n, b)
            host[n // 4, :] = 0.0                              # a zero row: the cosine's denominator is 0
            s = e.mat(host)
            for sim in (L.LINK_COS, L.LINK_DOT):
                auc, pos, neg = C.c_double(), C.c_int64(), C.c_int64()
                e.ok(lib.pgh_link_auc(s, plan, sim, C.byref(auc), C.byref(pos), C.byref(neg)))
                preds = np.zeros(pairs - 1)
                e.ok(lib.pgh_link_predictions(s, plan, sim, 1, pairs - 1, f64(preds)))
                factors = e.vec(np.zeros(n))
                e.ok(lib.pgh_link_factors(s, sim, factors))
                e.out[f"pgh_link_auc pgh_link_predictions pgh_link_factors n={n} b={b} similarity={sim}"] = [
                    np.array([auc.value]), np.array([pos.value, neg.value]), preds, e.vec_host(factors, n)]
        lib.pgh_link_plan_destroy(plan)
        e.free()


def run_fair(e, rng):
    lib = e.lib
    for n in NS:
        pers, sens, ranks = e.vec(rng.random(n)), e.vec((rng.random(n) < 0.4).astype(np.float32)), e.vec(rng.random(n))
        for probes in KS:
            for buckets in (0, 1, 4):
                for skew in (0, 1):
                    params = rng.standard_normal(probes * (4 * buckets + 1))
                    out = e.mat(np.zeros((n, probes)))
                    e.ok(lib.pgh_prior_edit(pers, sens, ranks, 0.9, ptr(params), buckets, probes, skew, out))
                    e.out[f"pgh_prior_edit n={n} probes={probes} buckets={buckets} skew={skew}"] = [e.mat_host(out, n, probes)]
        e.free()


SECTIONS = (run_measure, run_pairs, run_probe, run_rank, run_oversample, run_lfpr, run_krylov, run_link, run_fair)


def main():
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    results = []
    for path in sys.argv[1:]:
        engine = Engine(bind(path))
        for k, section in enumerate(SECTIONS):
            section(engine, np.random.default_rng(100 + k))     # both builds see the same inputs
        results.append(engine.out)
    old, new = results
    ok = set(old) == set(new)
    for label, a in old.items():
        b = new.get(label, [])
        same = len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
        refused = " ".join(x.tobytes().decode() for x in a if x.dtype == np.uint8 and x.size > 2)
        print(f"{'same' if same else 'DIFF'}  {label}{'  [' + refused + ']' if refused else ''}", flush=True)
        ok = ok and same
    print("slab ab ok" if ok else "slab ab MISMATCH")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
