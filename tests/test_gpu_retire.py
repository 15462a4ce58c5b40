"""The multi-seed loops that retire converged columns inside the run (include/pgh_retire.h; ``retire=`` of PageRank, AbsorbingWalks,
SymmetricAbsorbingRandomWalks and AlgorithmSelection) on the golden graphs of tests/golden/cases.py.

Every held column meets the suite's acceptance rule (tests/retire_common.py: the fp64 oracle and the single-vector device run, 1e-6,
equal iteration counts, a stop one check apart only within 2 % of the tolerance, zero columns exactly zero).  What a test needs of its
inputs it asserts from the oracle alone, before it looks at the engine: at most 2 columns of a batch may need the one-check allowance,
and -- where the run is to narrow -- the oracle's stopping iterations cross enough levels.  On rmat12_sym, where a dense start settles
over a hundred steps with a residual that falls by a few per cent per step, the stage structure is checked on every column and the
acceptance rule on the columns the oracle vouches for (retire_common.vouched).

The report of every run must be the one the engine's own per-column step counts imply under the rule of include/pgh_retire.h
(retire_common.stages_of)."""
import ctypes as C

import numpy as np
import pytest

import cases
import retire_common as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def uploads(gpu_engine):
    from pygrank_amd import _lib
    for name in _lib.RETIRE_SIGNATURES:
        assert _lib.entry(name) is not None, name
    built = {}

    def get(key):
        if key not in built:
            A, directed, _ = cases.GRAPHS[key]()
            built[key] = rc._graph(gpu_engine, A, "col" if directed else "symmetric")
        return built[key]
    return get


# ------------------------------------------------------------------------------------------------------------- helpers
def oracle_view(G, F, spec, hook=True, oracle_kw=None):
    """Per column, from the oracle alone: its steps (iterations - 1; 0 for a zero column), whether it may need the one-check allowance,
    whether the oracle vouches for its stop."""
    _, oracle, rule, tol, modulo = spec
    steps, near, vouched = [], [], []
    for j in range(F.shape[1]):
        _, its, margins = rc.oracle_trace(oracle, G["M"], F[:, j], rule, tol, modulo, hook=hook, **(oracle_kw(j) if oracle_kw else {}))
        steps.append(max(its - 1, 0))
        near.append(rc.near(margins))
        vouched.append(rc.vouched(margins))
    return steps, near, vouched


def sample(gkey, near, vouched):
    """The columns the acceptance rule is held on: all of them, with at most 2 that may need the allowance (asserted); on rmat12_sym
    the ones the oracle vouches for."""
    if gkey == "rmat12_sym":
        cols = [j for j, ok in enumerate(vouched) if ok]
        assert len(cols) >= max(len(vouched) // 4, 2), (len(cols), len(vouched))
    else:
        cols = list(range(len(near)))
    assert sum(near[j] for j in cols) <= 2, [j for j in cols if near[j]]
    return cols


def run(pg, G, F, spec, retire, call_kw=None, **more):
    ranker = spec[0](retire=retire, **more)
    out = np.asarray(ranker.propagate(G["adj"], pg.to_primitive(F), **(call_kw or {})), dtype=np.float64)
    assert out.shape == F.shape and len(ranker.last_batches) == (F.shape[1] + 63) // 64
    return ranker, out, [c["iterations"] for batch in ranker.last_batches for c in batch]


def check_report(batch, levels, narrowings=None):
    """One chunk's record in last_batches: the report is the one its own step counts imply; bit 5 of every column's flags says whether
    the run narrowed.  Returns the stages."""
    steps, stopped = [c["spmv"] for c in batch], [c["converged"] for c in batch]
    want, streamed = rc.stages_of(steps, stopped, len(batch), levels, max(steps))
    for c in batch:
        assert rc.report_stages(c["stages"]) == want and c["stages"]["column_steps"] == streamed, (c["stages"], want, streamed)
        assert bool(c["flags"] & rc.NARROWED) == (len(want) > 1), (c["flags"], want)
    if narrowings is not None:
        assert len(want) - 1 >= narrowings, want
    return want


def abi(pg, G, F, name, ranker, levels="plain", alpha=0.85, alphas=None, lam=None, start=None):
    """One call of the C-ABI entry `name` (levels == "plain") or of its retiring sibling (levels: None for the default list, or a
    list): (status, ranks, results, report)."""
    from pygrank_amd import _lib as L
    from pygrank_amd.device import DeviceMatrix
    X = DeviceMatrix.from_host(F)
    norms = X.col_abssum()
    P = X.div_cols(norms)
    R = DeviceMatrix.empty(*F.shape) if start is None else DeviceMatrix.from_host(start)
    b = F.shape[1]
    cfg = ranker._loop_cfg(alpha, bool(ranker.use_quotient), 1.0)
    cfg.start_from_p = 1 if start is None else 0
    results, scales = (L.LoopResult * b)(), (C.c_double * b)(*[float(v) for v in norms])
    head = [G["g"]._h, P._h] + ([lam._h] if lam is not None else []) + [R._h, C.byref(cfg)]
    head += ([(C.c_double * b)(*alphas)] if alphas is not None else []) + [scales, results]
    report = L.RetireReport()
    if isinstance(levels, str):
        fn = getattr(L.lib(), name) if name in L.SIGNATURES else L.entry(name)
        status = fn(*head)
    else:
        arr, count = L.retire_levels(True if levels is None else list(levels))
        status = L.entry(name + "_retire")(*head, arr, count, C.byref(report))
    return status, R.numpy(), results, report


def abi_stages(report):
    from pygrank_amd import _lib as L
    return L.retire_stages(report)


# ------------------------------------------------------------------------------------------------------------- 1. columns
# (family, rule, graph, width, seed of the mix, levels in turn): every width under every PageRank rule; both level lists on the wide ones
PPR = [("l1", "rmat12_sym", 64, 1, (rc.DEFAULT_LEVELS, rc.WIDE_LEVELS)), ("mabs", "er10k", 64, 1, (rc.WIDE_LEVELS, rc.DEFAULT_LEVELS)),
       ("linf", "rmat10_dir", 64, 1, (rc.DEFAULT_LEVELS,)), ("modulo3", "rmat12_sym", 64, 9, (rc.WIDE_LEVELS,)),
       ("l1", "er10k", 33, 3, (rc.WIDE_LEVELS, rc.DEFAULT_LEVELS)), ("mabs", "rmat10_dir", 33, 2, (rc.DEFAULT_LEVELS,)),
       ("linf", "weighted300", 33, 1, (rc.DEFAULT_LEVELS, rc.WIDE_LEVELS)), ("modulo3", "rmat12_sym", 33, 9, (rc.DEFAULT_LEVELS,)),
       ("l1", "rmat10_dir", 17, 11, (rc.DEFAULT_LEVELS, rc.WIDE_LEVELS)), ("mabs", "weighted300", 17, 12, (rc.WIDE_LEVELS,)),
       ("linf", "rmat12_sym", 17, 13, (rc.DEFAULT_LEVELS,)), ("modulo3", "er10k", 17, 14, (rc.DEFAULT_LEVELS,)),
       ("l1", "weighted300", 5, 16, (rc.DEFAULT_LEVELS,)), ("mabs", "rmat12_sym", 5, 17, (rc.WIDE_LEVELS,)),
       ("linf", "er10k", 5, 1, (rc.DEFAULT_LEVELS,)), ("modulo3", "rmat10_dir", 5, 19, (rc.WIDE_LEVELS,))]


@pytest.mark.parametrize("rule,gkey,width,seed,level_lists", PPR, ids=[f"{r}-{g}-b{w}" for r, g, w, _, _ in PPR])
def test_pagerank_columns_against_oracle_and_single_runs(gpu_engine, uploads, rule, gkey, width, seed, level_lists):
    pg, G = gpu_engine, uploads(gkey)
    spec = rc.family(pg, "pagerank", rule)
    F = rc.mix(G, width, seed)
    steps, near, vouched = oracle_view(G, F, spec)
    cols = sample(gkey, near, vouched)
    due = {levels: len(rc.stages_of(steps, [True] * width, width, levels, max(steps))[0]) - 1 for levels in level_lists}
    print("oracle steps", min(steps), "..", max(steps), "near", sum(near), "held", len(cols), "narrowings due", due)
    if width >= 17 and rc.DEFAULT_LEVELS in due:
        assert due[rc.DEFAULT_LEVELS] >= 2, due                    # the stopping iterations cross at least two of the default levels
    assert all(count >= 1 for count in due.values()), due
    refs = rc.References(pg, G, F, spec, cols, label=f"pagerank/{rule}/{gkey}/b{width}")
    for levels in level_lists:
        ranker, out, iters = run(pg, G, F, spec, True if levels == rc.DEFAULT_LEVELS else list(levels))
        stages = check_report(ranker.last_batches[0], levels, narrowings=1)
        print("levels", levels, "stages", stages, "streamed", ranker.last_batches[0][0]["stages"]["column_steps"], "of", stages[0][0] * max(iters))
        refs.hold(out, iters, who=f"levels {levels[0]}")


@pytest.mark.parametrize("levels", [rc.DEFAULT_LEVELS, rc.WIDE_LEVELS], ids=["default", "wide"])
def test_mixed_alphas_against_oracle_and_single_runs(gpu_engine, uploads, levels):
    """pgh_ppr_run_batch_mixed_retire with 32 alphas from 0.5 to 0.97: a column's alpha follows it through every narrowing."""
    pg, G = gpu_engine, uploads("rmat10_dir")
    alphas = [float(a) for a in np.linspace(0.5, 0.97, 32)]
    F = rc.mix(G, 32, 1)
    specs = [rc.family(pg, "pagerank", "l1", alpha=a) for a in alphas]
    views = [oracle_view(G, F[:, j:j + 1], specs[j]) for j in range(32)]
    steps, near = [v[0][0] for v in views], [v[1][0] for v in views]
    assert sum(near) <= 2, near
    assert len(rc.stages_of(steps, [True] * 32, 32, levels, max(steps))[0]) >= 3
    status, out, results, report = abi(pg, G, F, "pgh_ppr_run_batch_mixed", specs[0][0](), levels=levels, alphas=alphas)
    assert status == 0
    got_steps = [r.spmv_count for r in results]
    want, streamed = rc.stages_of(got_steps, [bool(r.converged) for r in results], 32, levels, max(got_steps))
    assert rc.report_stages(abi_stages(report)) == want and report.column_steps == streamed and len(want) >= 3
    assert all(r.flags & rc.NARROWED for r in results)
    for j in range(32):                                             # each column has its own family (its alpha): one reference set each
        refs = rc.References(pg, G, F, specs[j], [j], label=f"mixed/alpha {alphas[j]:.3f}")
        refs.hold(out, [r.iterations for r in results])


WALKS = [("absorbing", "l1", "weighted300", 17, 1, rc.DEFAULT_LEVELS), ("absorbing", "mabs", "er10k", 33, 1, rc.WIDE_LEVELS),
         ("sarw", "default", "er10k", 17, 1, rc.DEFAULT_LEVELS)]


@pytest.mark.parametrize("name,rule,gkey,width,seed,levels", WALKS, ids=[f"{n}-{r}-{g}-b{w}" for n, r, g, w, _, _ in WALKS])
def test_walk_columns_against_oracle_and_single_runs(gpu_engine, uploads, name, rule, gkey, width, seed, levels):
    pg, G = gpu_engine, uploads(gkey)
    spec = rc.family(pg, name, rule)
    F = rc.mix(G, width, seed)
    steps, near, vouched = oracle_view(G, F, spec, hook=name != "sarw")
    cols = sample(gkey, near, vouched)
    assert len(rc.stages_of(steps, [True] * width, width, levels, max(steps))[0]) >= 3
    refs = rc.References(pg, G, F, spec, cols, label=f"{name}/{rule}/{gkey}/b{width}")
    ranker, out, iters = run(pg, G, F, spec, True if levels == rc.DEFAULT_LEVELS else list(levels))
    check_report(ranker.last_batches[0], levels, narrowings=2)
    refs.hold(out, iters)


# ------------------------------------------------------------------------------------------------------------- 2. same bits
def test_same_bits_before_the_first_narrowing(gpu_engine, uploads):
    pg, G = gpu_engine, uploads("rmat10_dir")
    spec = rc.family(pg, "pagerank", "l1")
    F = rc.mix(G, 33, 2)
    _, plain, plain_res, _ = abi(pg, G, F, "pgh_ppr_run_batch", spec[0]())
    # no levels: one stage, the plain entry's bits and results
    status, out, res, report = abi(pg, G, F, "pgh_ppr_run_batch", spec[0](), levels=[])
    assert status == 0 and np.array_equal(out, plain)
    assert rc.report_stages(abi_stages(report)) == [(36, 33, 1)] and report.column_steps == 36 * max(r.spmv_count for r in res)
    for r, q in zip(res, plain_res):
        assert (r.iterations, r.converged, r.spmv_count, r.flags, r.last_error) == (q.iterations, q.converged, q.spmv_count, q.flags, q.last_error)
    # every column stops together: one stage, the plain bits
    iters_spec = rc.family(pg, "pagerank", "iters")
    _, fixed_plain, _, _ = abi(pg, G, F, "pgh_ppr_run_batch", iters_spec[0]())
    status, fixed, res, report = abi(pg, G, F, "pgh_ppr_run_batch", iters_spec[0](), levels=None)
    assert status == 0 and np.array_equal(fixed, fixed_plain) and report.num_stages == 1 and not any(r.flags & rc.NARROWED for r in res)
    assert all(r.iterations == 12 for r in res)
    # a run that narrows: the columns retired at its first narrowing only ever ran wide steps
    status, out, res, report = abi(pg, G, F, "pgh_ppr_run_batch", spec[0](), levels=None)
    stages = rc.report_stages(abi_stages(report))
    assert status == 0 and len(stages) >= 3 and all(r.flags & rc.NARROWED for r in res)
    first = [j for j in range(33) if res[j].converged and res[j].spmv_count < stages[1][2]]
    assert len(first) == 33 - stages[1][1] >= 1
    for j in first:
        assert res[j].iterations == plain_res[j].iterations and np.array_equal(out[:, j], plain[:, j]), j
    for j in range(33):
        assert abs(res[j].iterations - plain_res[j].iterations) <= 1 and rc._rel(out[:, j], plain[:, j]) <= rc.BOUND, j


# ------------------------------------------------------------------------------------------------------------- 3. pause + narrowing
def test_a_pause_and_narrowings_in_one_run(gpu_engine, uploads):
    """One column carries a negative value on a row nothing propagates into: it stays negative in every iterate, the fused residual
    pauses at the first check and the run goes on with the separate kernel -- and narrows behind committed closes as before."""
    pg, G = gpu_engine, uploads("rmat10_dir")
    spec = rc.family(pg, "pagerank", "l1")
    F = rc.mix(G, 20, 11)
    F[G["dead"][0], 9] = np.float32(-0.2)
    assert F[:, 9].sum() > 0.2 * np.abs(F[:, 9]).sum()
    assert np.any(spec[1](G["M"], F[:, 9], error_type="iters", max_iters=2)[0] < 0)       # the first iterate holds a negative value
    steps, near, _ = oracle_view(G, F, spec)
    assert sum(near) <= 2 and len(rc.stages_of(steps, [True] * 20, 20, rc.DEFAULT_LEVELS, max(steps))[0]) >= 3
    ranker, out, iters = run(pg, G, F, spec, True)
    flags = [c["flags"] for c in ranker.last_batches[0]]
    assert all(f & 1 for f in flags) and all(f & 2 for f in flags), flags
    check_report(ranker.last_batches[0], rc.DEFAULT_LEVELS, narrowings=2)
    rc.References(pg, G, F, spec, range(20), label="pause").hold(out, iters)


# ------------------------------------------------------------------------------------------------------------- 4. warm start
def test_warm_start_through_the_c_abi(gpu_engine, uploads):
    """start_from_p = 0 with non-zero ranks: every row takes part (no row is skipped as dead), so the narrow sums slab needs its
    structural zeros again."""
    pg, G = gpu_engine, uploads("rmat10_dir")
    spec = rc.family(pg, "pagerank", "l1")
    width, n = 17, G["n"]
    F = rc.mix(G, width, 11)
    rng = np.random.default_rng(5)
    start = rng.uniform(0.5, 1.5, (n, width))
    start = (start / start.sum(axis=0)).astype(np.float32).astype(np.float64)
    warm = lambda j: dict(warm_start=start[:, j].copy())      # noqa: E731
    steps, near, _ = oracle_view(G, F, spec, oracle_kw=warm)
    assert sum(near) <= 2 and len(rc.stages_of(steps, [True] * width, width, rc.DEFAULT_LEVELS, max(steps))[0]) >= 3
    status, out, res, report = abi(pg, G, F, "pgh_ppr_run_batch", spec[0](), levels=None, start=start)
    assert status == 0
    got = [r.spmv_count for r in res]
    want, streamed = rc.stages_of(got, [bool(r.converged) for r in res], width, rc.DEFAULT_LEVELS, max(got))
    assert rc.report_stages(abi_stages(report)) == want and report.column_steps == streamed and len(want) >= 3
    refs = rc.References(pg, G, F, spec, range(width), rank_kw=warm, oracle_kw=warm, label="warm")
    refs.hold(out, [r.iterations for r in res])


# ------------------------------------------------------------------------------------------------------------- 5. edges
def test_zero_and_dead_columns_cross_a_level_at_the_first_close(gpu_engine, uploads):
    pg, G = gpu_engine, uploads("rmat10_dir")
    spec = rc.family(pg, "pagerank", "l1")
    zeros = tuple(range(1, 40, 4))                                  # 10 of 40 columns: 30 <= 32 live behind the first close
    F = rc.mix(G, 40, 7, zeros=zeros, dead=(2, 22))
    assert sum(1 for j in range(40) if F[:, j].any()) == 30
    steps, near, _ = oracle_view(G, F, spec)
    assert sum(near) <= 2
    ranker, out, iters = run(pg, G, F, spec, True)
    stages = check_report(ranker.last_batches[0], rc.DEFAULT_LEVELS, narrowings=2)
    assert stages[1] == (32, 30, 2), stages
    assert not out[:, list(zeros)].any()
    rc.References(pg, G, F, spec, range(40), label="first close").hold(out, iters)


def test_columns_that_run_out_of_iterations_after_others_retired(gpu_engine, uploads):
    pg, G = gpu_engine, uploads("rmat10_dir")
    F = rc.mix(G, 17, 11)
    full = rc.family(pg, "pagerank", "l1")
    steps, _, _ = oracle_view(G, F, full)
    cap = sorted(steps)[len(steps) // 2] + 1                        # iterations at which about half the columns have stopped
    assert min(steps) + 1 < cap < max(steps) + 1
    spec = rc.family(pg, "pagerank", "l1", max_iters=cap)
    _, plain, plain_res, _ = abi(pg, G, F, "pgh_ppr_run_batch", spec[0]())
    status, out, res, report = abi(pg, G, F, "pgh_ppr_run_batch", spec[0](), levels=None)
    assert status == 0 and report.num_stages >= 2
    late = [j for j in range(17) if not res[j].converged]
    assert 1 <= len(late) < 17 and all(res[j].iterations == cap for j in late)
    for j in range(17):
        assert (res[j].iterations, res[j].converged) == (plain_res[j].iterations, plain_res[j].converged), j
        assert rc._rel(out[:, j], plain[:, j]) <= rc.BOUND, j
    for retire in (False, True):                                    # Python raises as the plain route does
        with pytest.raises(Exception, match="Could not converge"):
            spec[0](retire=retire).propagate(G["adj"], pg.to_primitive(F))


def test_two_chunks(gpu_engine, uploads):
    pg, G = gpu_engine, uploads("weighted300")
    spec = rc.family(pg, "pagerank", "l1")
    F = rc.mix(G, 81, 3)
    steps, near, _ = oracle_view(G, F, spec)
    cols = [j for j in range(81) if not near[j]][::4] + [j for j in range(81) if near[j]][:2]
    ranker, out, iters = run(pg, G, F, spec, True)
    assert [len(batch) for batch in ranker.last_batches] == [64, 17]
    for batch in ranker.last_batches:                               # each chunk is a run of its own, with a report of its own
        check_report(batch, rc.DEFAULT_LEVELS, narrowings=1)
    assert ranker.last_batches[0][0]["stages"] != ranker.last_batches[1][0]["stages"]
    rc.References(pg, G, F, spec, cols, label="two chunks").hold(out, iters)


def test_widths_and_levels_that_never_narrow(gpu_engine, uploads):
    pg, G = gpu_engine, uploads("weighted300")
    spec = rc.family(pg, "pagerank", "l1")
    F = rc.mix(G, 5, 16)
    for width, levels in ((1, None), (1, [4, 2, 1]), (5, [60, 40, 8]), (4, None)):     # no level lies below the slab's 4 or 8 columns
        _, plain, plain_res, _ = abi(pg, G, F[:, :width], "pgh_ppr_run_batch", spec[0]())
        status, out, res, report = abi(pg, G, F[:, :width], "pgh_ppr_run_batch", spec[0](), levels=levels)
        assert status == 0 and report.num_stages == 1 and report.ld[0] == (width + 3) & ~3 and report.live[0] == width, (width, levels)
        assert np.array_equal(out, plain) and [r.iterations for r in res] == [r.iterations for r in plain_res]
    # 5 columns with a level of 4: one narrowing, 8 -> 4
    status, out, res, report = abi(pg, G, F, "pgh_ppr_run_batch", spec[0](), levels=[7, 4])
    assert status == 0 and rc.report_stages(abi_stages(report))[1][0] == 4


def test_a_level_list_that_does_not_descend_is_an_error(gpu_engine, uploads):
    pg, G = gpu_engine, uploads("weighted300")
    from pygrank_amd import _lib as L
    spec = rc.family(pg, "pagerank", "l1")
    F = rc.mix(G, 5, 16)
    for levels in ([8, 16], [16, 16, 4], [64, 32], [8, 0]):
        status, out, _, _ = abi(pg, G, F, "pgh_ppr_run_batch", spec[0](), levels=levels)
        assert status not in (0, L.DECLINED), levels
        with pytest.raises(L.EngineError):
            spec[0](retire=levels).propagate(G["adj"], pg.to_primitive(F))


def test_graph_dropout_takes_the_plain_route(gpu_engine, uploads):
    pg, G = gpu_engine, uploads("weighted300")
    spec = rc.family(pg, "pagerank", "iters")
    F = rc.mix(G, 9, 4)
    ranker = spec[0](retire=True)
    out = np.asarray(ranker.propagate(G["adj"], pg.to_primitive(F), graph_dropout=0.2), dtype=np.float64)
    assert np.all(np.isfinite(out)) and all("stages" not in c for c in ranker.last_batches[0])
    ranker.propagate(G["adj"], pg.to_primitive(F))
    assert all("stages" in c for c in ranker.last_batches[0])


# ------------------------------------------------------------------------------------------------------------- 6. Python surface
def test_wrappers_keep_their_batch(gpu_engine):
    pg = gpu_engine
    A, directed, _ = cases.GRAPHS["rmat10_dir"]()
    graph = pg.AdjacencyWrapper(A, directed=directed)
    F = np.zeros((A.shape[0], 12))
    rng = np.random.default_rng(2)
    for j in range(12):
        F[rng.choice(A.shape[0], 3 + 40 * (j % 3), replace=False), j] = 1.0
    kw = dict(error_type=pg.L1, tol=1e-6, max_iters=1000)
    on, off = pg.PageRank(0.85, retire=True, **kw), pg.PageRank(0.85, **kw)
    top_on, top_off = (on >> pg.Top(10)).propagate(graph, F).numpy(), (off >> pg.Top(10)).propagate(graph, F).numpy()
    assert [len(batch) for batch in on.last_batches] == [12] and "stages" in on.last_batches[0][0] and "stages" not in off.last_batches[0][0]
    assert on.last_batches[0][0]["stages"]["ld"][0] == 12 and len(on.last_batches[0][0]["stages"]["ld"]) >= 2
    assert top_on.shape == top_off.shape and np.all(top_on.sum(axis=0) == top_off.sum(axis=0))
    inner = pg.PageRank(0.85, retire=True, **kw)
    so = pg.SeedOversampling(inner, "top", min_batch_width=2)
    many = so.propagate(graph, F).numpy()
    assert "stages" in inner.last_batches[0][0]
    plain = pg.SeedOversampling(pg.PageRank(0.85, **kw), "top", min_batch_width=2).propagate(graph, F).numpy()
    for j in range(12):
        assert rc._rel(many[:, j], plain[:, j]) <= rc.BOUND, j


def test_algorithm_selection_selects_the_same_filter(gpu_engine):
    """A recorded selection case (tests/golden/golden_selection.json, three splits): with retire the mixed PageRank group runs through
    pgh_ppr_run_batch_mixed_retire, and the selection, its values and its ranks are those of retire=False."""
    import selection_common as sc
    pg = gpu_engine
    case = sc.fixture()["cases"][2]
    graph, signal = sc.problem(pg)
    outcome = {}
    for retire in (False, True):
        rankers = sc.family(pg, pg.create_many_filters(**sc.FAMILY))
        tuner = pg.AlgorithmSelection(rankers.values(), measure=getattr(pg, case["measure"]), fraction_of_training=case["fractions"],
                                      min_batch_width=2, retire=retire)
        ranks = np.asarray(tuner.rank(graph, signal).np, dtype=np.float64)
        outcome[retire] = (tuner.last_selection, ranks)
    (off, ranks_off), (on, ranks_on) = outcome[False], outcome[True]
    assert on["selected"] == off["selected"] == case["selected"]
    assert [r["route"] for r in on["rankers"]] == [r["route"] for r in off["rankers"]] and "mixed_ppr" in [r["route"] for r in on["rankers"]]
    for call, plain in zip(on["mixed_calls"], off["mixed_calls"]):
        assert ("stages" in call) == (call["kind"] == "mixed_ppr") and "stages" not in plain
        assert call["kind"] == plain["kind"] and call["width"] == plain["width"]
    for mine, theirs in zip(on["rankers"], off["rankers"]):
        for got, ref in zip(mine["values"], theirs["values"]):
            assert abs(got - ref) <= sc.ALLOWANCE * abs(ref), (got, ref)
    assert rc._rel(ranks_on, ranks_off) <= rc.BOUND
