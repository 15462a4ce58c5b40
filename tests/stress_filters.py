"""Randomised parity of the whole filters on the GPU (run by tests/test_gpu_parity.py as a subprocess with serialised
kernels): random graphs x layout switches x {PageRank, AbsorbingWalks, HeatKernel taylor / chebyshev, propagate} against
the oracle (oracle/ref_loops.py) run on the engine's stored f32 matrix.  Usage: python tests/stress_filters.py --seconds 20"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pygrank_amd as pg  # noqa: E402
from oracle import ref_loops as orc  # noqa: E402
from pygrank_amd.device import DeviceGraph  # noqa: E402
from pygrank_amd.preprocessing import Adjacency  # noqa: E402
from pygrank_amd.signals import _IdentityMap  # noqa: E402
from stress_gpu import random_graph  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)
# batch widths of the propagate leg: each lane shape of the multi-seed kernels, both sides of its boundaries, partial and full float4s,
# and a second chunk after a full one
PROPAGATE_WIDTHS = (1, 3, 4, 5, 15, 16, 17, 24, 31, 32, 33, 48, 63, 64, 81, 130)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if os.environ.get("PGH_TEST_ENGINE") == "host":               # replay a seed on the host double (no GPU)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import host_double
        host_double.install()
    pg.load_backend("hip")
    rng = np.random.default_rng(args.seed)
    prop_rng = np.random.default_rng([args.seed, 1])               # the propagate leg's own draws
    t_end = time.time() + args.seconds
    done = 0
    # what the harness PROVES, leg by leg: how many runs land within north_star's 1e-6, within 2e-6, above; and how far
    # the stopping iterations lie from the oracle's.  Every run outside the four analysed classes -- alpha >= 0.99, runs of more than
    # 100 steps, a signed personalization, the "chebyshev" recurrence -- is HELD to 1e-6.
    stats = {}

    def record(leg, rel, delta):
        row = stats.setdefault(leg, dict(runs=0, le_1e6=0, le_2e6=0, above=0, worst=0.0, deltas={}))
        row["runs"] += 1
        row["le_1e6" if rel <= 1e-6 else ("le_2e6" if rel <= 2e-6 else "above")] += 1
        row["worst"] = max(row["worst"], float(rel))
        row["deltas"][int(delta)] = row["deltas"].get(int(delta), 0) + 1

    while time.time() < t_end:
        A = random_graph(rng)
        n = A.shape[0]
        if n < 2 or A.nnz == 0 or n > 80000:
            continue
        for key, val in (("PGH_BLOCKS", str(int(rng.choice([1, 2, 4, 8])))), ("PGH_RELABEL", str(int(rng.integers(0, 2)))),
                         ("PGH_PB", str(int(rng.random() < 0.3))), ("PGH_PB_FORCE", "1"), ("PGH_TRIM", str(int(rng.integers(0, 2)))),
                         ("PGH_PB_HEAVY", str(int(rng.choice([16384, 8, 64])))), ("PGH_PB_HUBMAX", str(int(rng.choice([262144, 150, 4000])))),
                         ("PGH_PB_BINROWS", str(int(rng.choice([4096, 8192, 16384])))),     # the finish kernel's three shapes
                         # round 6, the f64 image (the "chebyshev" legs): a hot cache of a few dozen to a few thousand sources, so that these small
                         # graphs have a cold tail -- its propagation-blocking image (hub bins, heavy rows in the stream), 2- or 4-byte stream words
                         ("PGH_HOT64", str(int(rng.choice([20224, 32, 256, 2048])))), ("PGH_STREAM16", str(int(rng.integers(0, 2)))),
                         ("PGH_PB64", str(int(rng.random() < 0.8)))):
            os.environ[key] = val
        # round 6: one run in seven is PageRank / AbsorbingWalks at tol = 1e-9 -- below fp32 eps the filters choose f64 iterates on the f64
        # image (whose layout the switches above vary); the oracle then runs with the reference's fp64 eps and the iteration counts must be
        # EQUAL.  These runs store the matrix VALUED (PGH_VALUES=1): the f64 image of a value-free graph multiplies its f32 scales in f64
        # (3 x f32(1 / 3) = 1 + 3e-8) where the downloaded matrix the oracle gets holds the f32 product (1.0) -- two matrices 6e-8 apart, and
        # at 1e-9 a run sees that: on a regular graph (the reference's residual falls faster than alpha^k) the difference decays at alpha^k and
        # the engine stops 3 steps later (seed 31 #5353: 19 against 16); a start ON the fixed point (M = I, seed 31 #3073) becomes a run of
        # 18 steps.  With stored values both sides hold the same numbers.
        f64leg = rng.random() < 1.0 / 7.0
        os.environ["PGH_VALUES"] = "1" if f64leg else "0"
        norm = str(rng.choice(["col", "symmetric"]))
        g = DeviceGraph.from_adjacency(A, norm)
        M = sp.csr_array(g.download_transposed().T.astype(np.float64))        # the engine's matrix (f32 values), un-transposed
        adj = Adjacency(g)
        adj._pygrank_preprocessed = {"hip": adj}
        adj._pygrank_node2id = _IdentityMap(n)
        adj.is_directed = lambda: True
        p = np.zeros(n)
        p[rng.integers(0, n, min(n, 7))] = 0.5 + rng.random(min(n, 7))
        shape = float(rng.random())
        if shape < 0.15:                                           # a dense personalization (the gather pass instead of the seed list)
            p = 0.1 + rng.random(n)
        elif shape < 0.35 and norm == "col":                       # negative entries: the in-kernel residual must hand the decision back
            p[rng.integers(0, n, min(n, 3))] = -0.3
            # (the L1 quotient divides by sum(y) = alpha * sum(M^T x) + (1 - alpha) * sum(p / |p|_1): a personalization whose sum is
            # negative enough makes that ZERO in exact arithmetic -- p = (-0.3, -0.3) at alpha = 0.5 -- and every evaluation garbage,
            # the reference's included; the draws keep sum(p) >= 0.3 |p|_1)
            if p.sum() < 0.3 * np.abs(p).sum():
                p[int(np.argmax(p))] += 1.0 + np.abs(p).sum()
        desc = f"#{done} n={n} nnz={A.nnz} norm={norm} p={'dense' if shape < 0.15 else ('signed' if shape < 0.35 and norm == 'col' else 'seeds')} " \
            + " ".join(f"{k}={os.environ[k]}" for k in ("PGH_BLOCKS", "PGH_RELABEL", "PGH_PB", "PGH_TRIM", "PGH_PB_HEAVY", "PGH_PB_HUBMAX", "PGH_HOT64",
                                                         "PGH_STREAM16", "PGH_PB64"))
        which = int(rng.integers(0, 2)) if f64leg else int(rng.integers(0, 6))
        eps_kw = {} if f64leg else dict(eps=EPS32)
        if f64leg:
            p = p.astype(np.float32).astype(np.float64)            # the boundary hands f32 vectors: the oracle gets what the engine gets
        if which == 5:
            # rank(..., graph_dropout=) as one device loop on whatever layout the switches gave: against a host loop that rebuilds every
            # step's mask with the numpy twin of the hash (the mask of step k + 1: seed0 + 2 + k, tests/kernel_checks.py)
            from oracle import rmat_np
            MT = g.download_transposed()
            rate, steps = float(rng.choice([0.2, 0.5])), int(rng.integers(2, 7))
            pg.backend.hip.set_dropout_seed(1000 + done)
            ranker = pg.PageRank(0.85, error_type="iters", max_iters=steps + 1)
            got = np.asarray(ranker.rank(adj, p.copy(), graph_dropout=rate).np)
            norm1 = np.abs(p).sum()
            pn = (p.astype(np.float32) / np.float32(norm1)).astype(np.float64)
            x, quot = pn.copy(), 1.0
            e = np.arange(MT.nnz, dtype=np.uint64)
            for k in range(steps):
                with np.errstate(over="ignore"):
                    h = rmat_np.splitmix64(np.uint64(1000 + done + 2 + k) ^ (e * np.uint64(0xD6E8FEB86659FD93)))
                keep = (h >> np.uint64(32)).astype(np.int64) >= int(np.floor(rate * 4294967296.0))
                data = (MT.data.astype(np.float32) * np.float32(1.0 / (1.0 - rate))).astype(np.float32).astype(np.float64) * keep
                y = 0.85 * quot * (sp.csr_array((data, MT.indices, MT.indptr), shape=MT.shape) @ x) + 0.15 * pn
                quot, x = (1.0 / y.sum() if y.sum() != 0 else 0.0), y
            want = x * quot * norm1
            rel = np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-30)
            # (a signed personalization under a mask that drops half the entries loses digits to cancellation in ANY f32 evaluation: the
            # host double reproduces the engine's 7.65e-6 of seed 41 #3900 to the last digit)
            record("dropout loop, signed p" if (p < 0).any() else "dropout loop", rel, 0)
            if rel > (2e-5 if (p < 0).any() else 4e-6) or ranker.last_loop["spmv"] != steps:
                print("MISMATCH dropout loop", desc, "rate", rate, "steps", steps, "rel", rel, flush=True)
                sys.exit(1)
            done += 1
            continue
        if which == 0:
            kw = dict(alpha=float(rng.choice([0.5, 0.85] if f64leg else [0.5, 0.85, 0.99])), use_quotient=bool(rng.integers(0, 2)))
            err = str(rng.choice(["l1", "mabs", "linf"]))
            tol = 1e-9 if f64leg else float(rng.choice([1e-5, 1e-6]))
            ranker = pg.PageRank(kw["alpha"], use_quotient=kw["use_quotient"], error_type={"l1": pg.L1, "mabs": pg.Mabs, "linf": pg.MaxDifference}[err],
                                 tol=tol, max_iters=300)
            same_steps = lambda k: orc.pagerank(M, p, error_type="iters", max_iters=k, **eps_kw, **kw)[0]   # noqa: E731
            at_tol = lambda f: orc.pagerank(M, p, error_type=err, tol=tol * f, max_iters=300, **eps_kw, **kw)[1]   # noqa: E731
            try:
                want, it = orc.pagerank(M, p, error_type=err, tol=tol, max_iters=300, **eps_kw, **kw)
            except Exception:                                      # does not converge in 300 iterations: the engine must say so too
                try:
                    ranker.rank(adj, p.copy())
                except Exception:
                    done += 1
                    continue
                # the engine converged: a run whose residual shrinks ~1 % per step (alpha = 0.99) crosses the tolerance within f32 rounding of it for
                # several steps, so the engine may stop at 299 where the oracle needs 302 (seed 9062 #8001: a 2-node graph, Mabs 1e-6).  The oracle
                # then gets the slack the comparison below allows (its // 25 steps) beyond the limit; it must converge there
                try:
                    want, it = orc.pagerank(M, p, error_type=err, tol=tol, max_iters=300 + 300 // 25, **eps_kw, **kw)
                except Exception:
                    print("MISSING non-convergence exception", desc, type(ranker).__name__, "engine iterations:", ranker.convergence.iteration,
                          "A:", A.toarray().tolist() if n <= 4 else "", "p:", p.tolist() if n <= 4 else "", kw, err, tol, flush=True)
                    sys.exit(1)
        elif which == 1:
            tol = 1e-9 if f64leg else 1e-6
            ranker = pg.AbsorbingWalks(0.85, error_type=pg.L1, tol=tol, max_iters=300)
            same_steps = lambda k: orc.absorbing_walks(M, p, alpha=0.85, error_type="iters", max_iters=k, **eps_kw)[0]   # noqa: E731
            at_tol = lambda f: orc.absorbing_walks(M, p, alpha=0.85, error_type="l1", tol=tol * f, max_iters=300, **eps_kw)[1]   # noqa: E731
            try:
                want, it = orc.absorbing_walks(M, p, alpha=0.85, error_type="l1", tol=tol, max_iters=300, **eps_kw)
            except Exception:
                try:
                    ranker.rank(adj, p.copy())
                except Exception:
                    done += 1
                    continue
                try:                                                # (as above)
                    want, it = orc.absorbing_walks(M, p, alpha=0.85, error_type="l1", tol=tol, max_iters=300 + 300 // 25, **eps_kw)
                except Exception:
                    print("MISSING non-convergence exception", desc, type(ranker).__name__, "engine iterations:", ranker.convergence.iteration,
                          "A:", A.toarray().tolist() if n <= 4 else "", "p:", p.tolist() if n <= 4 else "", flush=True)
                    sys.exit(1)
        elif which in (2, 3):
            ctype = "taylor" if which == 2 else "chebyshev"
            want, it = orc.heat_kernel(M, p, t=3, coefficient_type=ctype, error_type="iters", max_iters=20, eps=EPS32)
            ranker = pg.HeatKernel(3, coefficient_type=ctype, error_type="iters", max_iters=20)
        else:
            # the draws of the first propagate leg, kept so that every other leg sees the same sequence of graphs; what this leg runs is
            # drawn from a generator of its own
            for _ in range(int(rng.choice([1, 3, 12, 17, 33]))):
                rng.integers(0, n, 3)
            # the multi-seed loops of PageRank, HeatKernel (taylor), AbsorbingWalks and SymmetricAbsorbingRandomWalks at every lane shape
            # (4 / 8 / 16 lanes per row, partial float4s, a second chunk past 64 columns), on seed, signed and dense columns
            filt = str(prop_rng.choice(["PageRank", "HeatKernel taylor", "AbsorbingWalks", "SymmetricAbsorbingRandomWalks"]))
            b = int(prop_rng.choice(PROPAGATE_WIDTHS))
            feats = np.zeros((n, b))
            for j in range(b):
                kind = prop_rng.random()
                if kind < 0.15:                                    # dense
                    feats[:, j] = 0.1 + prop_rng.random(n)
                else:
                    feats[prop_rng.integers(0, n, 3), j] = 1.0 + j
                    if kind < 0.4 and norm == "col":               # signed, with sum(p) >= 0.3 |p|_1 as in the single-vector legs
                        feats[prop_rng.integers(0, n, 2), j] = -0.3
                        if feats[:, j].sum() < 0.3 * np.abs(feats[:, j]).sum():
                            feats[int(np.argmax(feats[:, j])), j] += 1.0 + np.abs(feats[:, j]).sum()
            feats = feats.astype(np.float32).astype(np.float64)
            if filt == "HeatKernel taylor":
                make = lambda: pg.HeatKernel(3, error_type="iters", max_iters=20)   # noqa: E731
                column_oracle = lambda q, **kw: orc.heat_kernel(M, q, t=3, eps=EPS32, **(kw or dict(error_type="iters", max_iters=20)))  # noqa: E731
            else:
                make, fn = {"PageRank": (lambda: pg.PageRank(0.85, error_type=pg.L1, tol=1e-6, max_iters=300),
                                         lambda q, **kw: orc.pagerank(M, q, alpha=0.85, eps=EPS32, **kw)),
                            "AbsorbingWalks": (lambda: pg.AbsorbingWalks(0.85, error_type=pg.L1, tol=1e-6, max_iters=300),
                                               lambda q, **kw: orc.absorbing_walks(M, q, alpha=0.85, eps=EPS32, **kw)),
                            "SymmetricAbsorbingRandomWalks": (lambda: pg.SymmetricAbsorbingRandomWalks(error_type=pg.L1, tol=1e-6, max_iters=300),
                                                              lambda q, **kw: orc.symmetric_absorbing_walks(M, q, eps=EPS32, **kw))}[filt]
                column_oracle = lambda q, _fn=fn, **kw: _fn(q, **(kw or dict(error_type="l1", tol=1e-6, max_iters=300)))  # noqa: E731
            ranker = make()
            tolerance_based = filt != "HeatKernel taylor"
            oracle_runs, oracle_fails, late = [], False, False
            for j in range(b):
                if not feats[:, j].any():
                    oracle_runs.append((feats[:, j], 0))
                    continue
                try:
                    oracle_runs.append(column_oracle(feats[:, j]))
                except Exception:
                    # a column that crosses the tolerance within f32 rounding of it around the limit (seed 9084 #4277: the engine stops inside
                    # the 300 steps, the oracle just outside): the oracle gets the slack the comparison below allows anyway, as in the
                    # single-vector legs; a column that does not converge THERE must raise in the engine too
                    try:
                        oracle_runs.append(column_oracle(feats[:, j], error_type="l1", tol=1e-6, max_iters=300 + 300 // 25))
                        late = True
                    except Exception:
                        oracle_fails = True
                        oracle_runs.append(None)
            try:
                out = np.asarray(ranker.propagate(adj, pg.to_primitive(feats)))
            except Exception as exc:
                if oracle_fails or late:                           # a column that does not converge (or only just outside the limit) raises
                    done += 1
                    continue
                print("EXCEPTION propagate", filt, desc, exc, flush=True)
                sys.exit(1)
            if oracle_fails:
                print("MISSING non-convergence exception in propagate", filt, desc, flush=True)
                sys.exit(1)
            if not hasattr(ranker, "last_batches"):
                if os.environ.get("PGH_TEST_ENGINE") != "host":    # (the host double has only PageRank's multi-seed loop)
                    print("propagate did not take the batch route", filt, desc, flush=True)
                    sys.exit(1)
                iterations = []
                for j in range(b):                                 # the column loop's stops, column by column
                    single = make()
                    if feats[:, j].any():
                        single.rank(adj, feats[:, j].copy())
                    iterations.append(single.convergence.iteration)
            else:
                iterations = [c["iterations"] for batch in ranker.last_batches for c in batch]
            for j in range(b):
                want, it = oracle_runs[j]
                if not feats[:, j].any():
                    if np.any(out[:, j] != 0):
                        print("MISMATCH propagate", filt, desc, "zero column", j, flush=True)
                        sys.exit(1)
                    continue
                its = iterations[j]
                if tolerance_based and its != it and abs(its - it) <= max(2, it // 25):   # stopped a step apart: compare at the engine's step count
                    want = column_oracle(feats[:, j], error_type="iters", max_iters=its)[0]
                rel = np.max(np.abs(out[:, j] - want)) / max(np.max(np.abs(want)), 1e-30)
                # a residual within f32 rounding of the tolerance may stop an iteration apart: the iterates then differ by ~tol.
                # Round 6 (tools/probe_propagate_stops.py, profiles/r06/propagate_stops.log): these inputs -- three seeds per column on graphs
                # of a few dozen nodes -- land within a few percent of the tolerance in ~2 % of the columns; the SAME columns through the
                # single-vector loop stop apart just as often (1.9 % against 2.1 %), and with f64 iterates (dtype="float64") never: what decides
                # is the f32 trajectory, 1e-7 beside the fp64 one, not the batch loop.
                # Each row is held to the bound of the single-vector leg of its class: 1e-6; a signed column 2e-6; a run of more than 100
                # steps 2e-6
                signed = bool((feats[:, j] < 0).any())
                leg = "propagate " + filt + (", signed p" if signed else "")
                bound = 2e-6 if signed else 1e-6
                if tolerance_based and its > 100:
                    leg, bound = leg + ", > 100 steps", 2e-6
                record(leg, rel, its - it)
                if (abs(its - it) > max(2, it // 25) if tolerance_based else its != it) or rel > bound:
                    print("MISMATCH propagate", filt, desc, "column", j, rel, "iterations", its, it, flush=True)
                    if os.environ.get("PGH_STRESS_DUMP"):          # replay material for a scratch script
                        sp.save_npz(os.path.join(os.environ["PGH_STRESS_DUMP"], "case_graph.npz"), sp.csr_matrix(A))
                        np.savez(os.path.join(os.environ["PGH_STRESS_DUMP"], "case_data.npz"), feats=feats, out=out, norm=norm,
                                 env=np.array([f"{k}={v}" for k, v in os.environ.items() if k.startswith("PGH_")]))
                    sys.exit(1)
            done += 1
            continue
        # Round 6: a third of the PageRank / AbsorbingWalks / taylor runs take the BACKEND-PRIMITIVE route (the whole-loop entry points
        # switched off: lazy vectors, resident iterates, pgh_resident_step on whatever layout the switches gave) -- held to the same bounds
        primitives = which in (0, 1, 2) and not f64leg and rng.random() < 0.33
        if primitives:
            ranker._fused_loop = lambda *a, **k: False
            ranker._fused_rank = lambda *a, **k: None
        try:
            got = np.asarray(ranker.rank(adj, p.copy()).np)
        except Exception as exc:                                   # non-convergence must agree with the oracle too
            if which in (0, 1) and (p < 0).any():
                # ... but for a SIGNED personalization: its iterate is a difference of large terms, and an f32 evaluation can end in a limit
                # cycle of a few ulp whose residual sits just above the tolerance -- seed 9062 #22129 (host double AND engine): AbsorbingWalks
                # on [[0, 0], [3, 1]], p = (-0.3, 0.904), the oracle stops after 51 steps, the f32 iterates alternate between two states
                # 3 ulp apart (residual 1.1e-6 against 1e-6) for ever.  Such a run is held to the signed class's bound AT the oracle's
                # step count, and logged as a leg of its own.
                stalled = (pg.PageRank(kw["alpha"], use_quotient=kw["use_quotient"], error_type="iters", max_iters=it) if which == 0
                           else pg.AbsorbingWalks(0.85, error_type="iters", max_iters=it))
                got_it = np.asarray(stalled.rank(adj, p.copy()).np)
                rel_it = np.max(np.abs(got_it - want)) / max(np.max(np.abs(want)), 1e-30)
                record(type(ranker).__name__ + ", signed p, f32 limit cycle above the tolerance", rel_it, 0)
                if rel_it <= 2e-6:
                    done += 1
                    continue
            print("EXCEPTION", desc, type(ranker).__name__, exc, "oracle:", it, "A:", A.toarray().tolist() if n <= 4 else "", "p:", p.tolist() if n <= 4 else "",
                  {k: v for k, v in vars(ranker).items() if k in ("alpha", "use_quotient")}, vars(ranker.convergence).get("tol"), flush=True)
            sys.exit(1)
        its = ranker.convergence.iteration
        tolerance_based = which in (0, 1)
        # slowly converging runs (alpha = 0.99: the residual shrinks ~1 % per step) sit within f32 rounding of the tolerance
        # for several iterations; the RESULT is still held to 2e-6 against the oracle stopped at the engine's step count
        slack = max(1, it // 25)
        # a residual within f32 rounding of the tolerance may stop an iteration apart: the result is then compared with the
        # oracle stopped after the engine's number of steps
        if tolerance_based and abs(its - it) > slack:
            # a residual that is NOT monotone (alpha = 0.99 on a near-bipartite graph: seed 51 #4476 dips to 0.99984e-6 at step 136 in
            # f64, 1.0058e-6 in f32, and next falls below the tolerance ten steps later) stops wherever its rounding puts the dip: the
            # engine's count must then be the oracle's at a tolerance 3 % tighter or looser
            try:
                near = sorted((at_tol(0.97), at_tol(1.03)))
            except Exception:
                near = [it, it]
            if near[0] - 1 <= its <= near[1] + 1:
                slack = abs(its - it)
        if tolerance_based and its != it and abs(its - it) <= slack and not f64leg:
            want = same_steps(its)
        rel = np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-30)
        fp64_basis = False
        if tolerance_based and not f64leg and 1e-6 < rel <= 2e-6 and its == it:
            # The oracle above runs on the engine's DOWNLOADED matrix (f32 values), so that storage rounding does not enter the comparison --
            # but that matrix is itself a perturbation of the reference's (preprocessing.py:99-142 in fp64), and a slowly mixing graph
            # carries it through every step: seed 47 #5865 (a band graph of 70 001 nodes, 59 steps) puts the engine 6.9e-7 from the
            # reference's own result, the oracle-on-f32-values 4.2e-7 on the other side of it, 1.12e-6 apart.  north_star's bound is
            # parity with the REFERENCE: a run in (1e-6, 2e-6] is held to 1e-6 against the fp64 normalisation of the graph, a leg of its own.
            M64 = orc.normalize(sp.csr_array(A, dtype=np.float64), norm, True)
            if which == 0:
                w64, it64 = orc.pagerank(M64, p, error_type=err, tol=tol, max_iters=300 + 300 // 25, **eps_kw, **kw)
            else:
                w64, it64 = orc.absorbing_walks(M64, p, alpha=0.85, error_type="l1", tol=tol, max_iters=300 + 300 // 25, **eps_kw)
            rel64 = np.max(np.abs(got - w64)) / max(np.max(np.abs(w64)), 1e-30)
            if it64 == its and rel64 <= 1e-6:
                fp64_basis, rel = True, rel64
        if os.environ.get("PGH_STRESS_TRACE") and its != it:
            print("NOTE", desc, type(ranker).__name__, {k: v for k, v in vars(ranker).items() if k in ("alpha", "use_quotient")},
                  getattr(ranker.convergence, "tol", None), getattr(ranker.convergence.error_type, "__name__", ranker.convergence.error_type),
                  "iterations", its, it, "rel", rel, flush=True)
        signed = bool((p < 0).any())
        leg = {0: "PageRank", 1: "AbsorbingWalks", 2: "HeatKernel taylor", 3: "HeatKernel chebyshev"}[which]
        if which == 0 and kw["alpha"] >= 0.99:
            leg += " alpha=0.99"
        finite = False
        if f64leg and its != it:
            # a run that TERMINATES in fp64 -- the start vector is the fixed point, or the operator is nilpotent: the oracle's count does not
            # move when its tolerance drops to 1e-13 -- has no residual to compare: the engine's operands are the f32 scales of the image
            # (3 x f32(1 / 3) = 1 + 3e-8 where the oracle's matrix holds f32(1.0)), so it converges geometrically to a point 1e-7 beside
            # (seed 31 #3073: M = I, 18 steps against 3).  Held to the result bound, logged as a leg of its own.
            try:
                finite = at_tol(1e-4) == it
            except Exception:
                finite = False
        if f64leg:
            leg += ", tol 1e-9 (f64 iterates)" + (", finite termination in fp64" if finite else "")
        if fp64_basis:
            leg += ", held against the reference's fp64 matrix"
        if primitives:
            leg += " (backend primitives)"
        if signed:
            leg += ", signed p"
        if which in (0, 1) and its > 100 and "0.99" not in leg:
            leg += ", > 100 steps"
        record(leg, rel, its - it)
        # north_star's bound for every run outside the analysed classes; the "chebyshev" recurrence S_k = (2 M^T - I) S_{k-1} amplifies
        # the f32 rounding of the INPUT vectors (x20 on rmat12/heat_cheb) whatever precision the recurrence itself runs in: 4e-6; a signed
        # personalization loses digits to cancellation in any f32 evaluation (the host double reproduces the engine's misses): 2e-6
        bound = 4e-6 if which == 3 else (2e-6 if signed else 1e-6)
        if which in (0, 1) and its > 100 and bound < 2e-6:
            # a run of hundreds of steps (a slowly mixing graph: rings, bands) carries the f32 rounding of its STORED operands (degrees,
            # p / |p|) through every step: seed 11 #687 (AbsorbingWalks, 286 steps) misses the oracle by 1.8658913e-06 on the engine AND,
            # to the last digit, on the host double -- storage, not evaluation.  Held to 2e-6, logged as a leg of its own.
            bound = 2e-6
        if which == 0 and kw["alpha"] >= 0.99:
            # alpha = 0.99 amplifies every rounding of a step by up to 1 / (1 - alpha) over a run of 100+ steps: ANY f32 evaluation
            # drifts -- the host double misses the oracle by 3.13e-6 where the engine misses it by 3.25e-6 (seed 62 #8480, 143 steps)
            bound = 8e-6
        if rel > bound or (tolerance_based and abs(its - it) > slack and not finite) or (not tolerance_based and its != it) or (f64leg and its != it and not finite):
            print("MISMATCH", type(ranker).__name__, desc, "rel", rel, "iterations", its, it,
                  {k: v for k, v in vars(ranker).items() if k in ("alpha", "use_quotient", "t", "coefficient_type")},
                  getattr(ranker.convergence, "tol", None), getattr(ranker.convergence.error_type, "__name__", ranker.convergence.error_type), flush=True)
            if os.environ.get("PGH_STRESS_DUMP"):                  # the case as data: replayed offline (tools/scratch)
                coo = sp.coo_array(A)
                np.savez(os.path.join(os.environ["PGH_STRESS_DUMP"], "case_data.npz"), row=coo.row, col=coo.col, val=coo.data, n=n, p=p, got=got,
                         want=want, its=its, it=it, norm=norm)
            sys.exit(1)
        done += 1
    for leg in sorted(stats):
        row = stats[leg]
        deltas = " ".join(f"{k:+d}:{v}" for k, v in sorted(row["deltas"].items()))
        print(f"  {leg:34s} runs {row['runs']:6d}  rel-Linf <= 1e-6: {row['le_1e6']:6d}  (1e-6, 2e-6]: {row['le_2e6']:4d}  above: {row['above']:4d}  "
              f"worst {row['worst']:.2e}  iterations engine - oracle: {deltas}", flush=True)
    print(f"filters stress ok: {done} runs in {args.seconds:.0f} s (seed {args.seed})", flush=True)


if __name__ == "__main__":
    main()
