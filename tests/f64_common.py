"""Row-wise references, bounds and graphs for the f64 image's step kernels (pygrank_amd/csrc/pgh_bsf64.hip), shared by
tests/test_gpu_f64_kernels.py (the engine), tests/test_f64_kernels_host.py (the host double) and tests/test_f64_bounds_host.py (which
proves that the bounds reject wrong results).

The reference.  Every step of the f64 routes is  y = a * w (.) (M^T (v (.) x)) + b * t  (Epi64: `w` the walks' row weights, `v` their
pre-scale of the iterate).  References are evaluated in long double (64-bit significand on x86: their own error lies 2^-11 below
every f64 term of the bounds) on the matrix the kernels MULTIPLY BY, which on a value-free two-sided image is not the stored f32
matrix: k_bsf64_bring and the epilogue's xg_out scale the gather vector by the f32 `src_scale` (the `left` of from_factored, on the
SOURCE j: pgh_graph.hip "M^T = diag(right) * W^T * diag(left)"), the stream adds it once per unit of an entry's integer multiplicity, and
the epilogue (k_bsf64_combine / k_pb64_finish::apply) multiplies the row sum by the f32 `dst_scale` (the `right`, on the OUTPUT i) -- all
in f64.  effective_matrix() builds M^T[i, j] = right_i * W[j, i] * left_j in f64 from f32-representable factors.

The bound of row i (row_bounds; every term derived, none measured):
  output rounding      2^-24 |ref_i| + 2^-126: half an f32 ulp (k_bsf64_take / _take_col round once), and the smallest normal so that
                       the verdict does not depend on the denormal mode;
  f64 summation        (nnz_i + 8) 2^-52 S_i, S_i = the sum of the magnitudes of every term of row i (the epilogue's b * t included):
                       the a-priori bound of a sum of nnz_i products in ANY order is (nnz_i - 1) u S_i with u = 2^-53; the products'
                       own roundings (the source scale, the value, the output scale, a, w) and the epilogue's add are eight more;
                       2^-52 = 2 u leaves the other half to the (far better) reference;
  carried              for chained steps, with B the bound of the previous vectors:  B_k = f64 term + |a| w |M^T| (v B_x) + |b| B_t
                       -- |M^T| applied to the previous bound (step());
  cold image only      k_pb64_finish turns every cold product into 64-bit fixed point with fma(v, S, kMagic), S = 2^(E - e):
                       one rounding to the quantum 2^(e - E) each, where 2^e is the first power of two above the launch's largest
                       cold product (`e` from amax, pgh_bsf64.hip "const int e = max((int)(amax >> 52) - 1022, -960)") and
                       E = min(51, 62 - count_bits) ("const int E = min(51, 62 - count_bits)"; count_bits = ceil(log2(cold entries of
                       the bin's largest row)), pgh_pb.hip pb_build "2^count_bits >= entries of the bin's largest row").  Row i:
                       cold_nnz_i 2^(e - E), carried through apply()'s factors dst_scale, a and row_w.  The tests take upper bounds
                       from their own operands: every entry counts as cold, e from the largest product of ANY entry, count_bits
                       from the longest row."""
import contextlib
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

F32 = np.float32
LD = np.longdouble
U52 = 2.0 ** -52
HALF_ULP32 = 2.0 ** -24
MIN_NORMAL32 = 2.0 ** -126
SENTINEL = -7.25

F64_FORMATS = {}          # case -> format() of its graph (the GPU cases)
F64_REPORT = {}           # case -> {check: worst |error| / bound}; filled by the batteries (printed by the test modules at teardown)

ENV_KEYS = ("PGH_HOT64", "PGH_BLOCKS64", "PGH_PB64", "PGH_PB", "PGH_PB_FORCE", "PGH_PB_HEAVY", "PGH_PB_HUBMAX", "PGH_STREAM16",
            "PGH_CHEB_CSR", "PGH_CHEB_F32", "PGH_VALUES", "PGH_FORMAT", "PGH_RELABEL", "PGH_BLOCKS")


@contextlib.contextmanager
def layout_env(**values):
    """Sets the layout switches for the block (every other one of ENV_KEYS unset) and restores all of them afterwards."""
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    try:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(values)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def report(case, check, ratio):
    slot = F64_REPORT.setdefault(case, {})
    slot[check] = max(slot.get(check, 0.0), float(ratio))


def is_f32(a):
    a = np.asarray(a, dtype=np.float64)
    return bool(np.array_equal(a.astype(F32).astype(np.float64), a))


# ------------------------------------------------------------------------------------------------------------------ the matrix
class Operator:
    """The matrix a step multiplies by, as the kernels see it.  MT: CSR of M^T in f64 (row i = output i); stream: the weights the
    STREAM holds per entry (multiplicities, or the f32 values), src / dst: the f64 copies of the f32 scales (ones when absent);
    nnz_row: stream entries per row (a multiplicity of m is m entries); valued: the stream carries f32 values."""

    def __init__(self, MT, stream, src, dst, nnz_row, valued):
        self.MT = sp.csr_array(MT)
        self.MT.sort_indices()
        self.absMT = abs(self.MT)
        self.stream = stream
        self.src, self.dst = src, dst
        self.nnz_row = np.asarray(nnz_row, dtype=np.float64)
        self.valued = valued
        self.n = self.MT.shape[0]

    def fixed_point_bits(self):
        """E of k_pb64_finish for the bin of the longest row (a lower bound of every bin's E: the largest quantum)."""
        longest = int(self.nnz_row.max()) if self.n else 1
        count_bits = int(np.ceil(np.log2(max(longest, 1))))
        return min(51, 62 - count_bits)

    def product_exponent(self, xs):
        """e with 2^e above every product the stream can hand to the cold image for the gathered vector xs (before the source scale):
        value-free entries hand over xs_j * src_j, valued ones val_ij * xs_j."""
        g = np.abs(np.asarray(xs, dtype=np.float64)) * np.abs(self.src)
        if self.valued:
            amax = float(np.max(np.abs(self.stream.data) * g[self.stream.indices])) if self.stream.nnz else 0.0
        else:
            amax = float(np.max(g[np.unique(self.MT.indices)])) if self.MT.nnz else 0.0
        if amax == 0.0:
            return -960
        return max(int(np.frexp(amax)[1]), -960)          # amax = m 2^ex with m in [0.5, 1): amax < 2^ex

    def quantum(self, xs, bits=None):
        """The cold image's term of every row BEFORE the factors a and row_w: nnz_i 2^(e - E) |dst_i|."""
        E = self.fixed_point_bits() if bits is None else bits
        return self.nnz_row * 2.0 ** (self.product_exponent(xs) - E) * np.abs(self.dst)


def effective_matrix(W, left=None, right=None, valued=False):
    """The Operator of M = diag(left) W diag(right) uploaded with DeviceGraph.from_factored (value-free: integer W, f32-representable
    factors kept apart) or of M = W uploaded with scipy_sparse_to_backend (valued: f32-representable data, no factors)."""
    W = sp.csr_array(W).astype(np.float64)
    n = W.shape[0]
    WT = sp.csr_array(W.T)
    WT.sort_indices()
    if valued:
        assert left is None and right is None and is_f32(WT.data)
        ones = np.ones(n)
        return Operator(WT, WT, ones, ones, np.diff(WT.indptr), True)
    assert np.array_equal(WT.data, np.round(WT.data)) and WT.data.min() >= 1
    src = np.ones(n) if left is None else np.asarray(left, dtype=np.float64)
    dst = np.ones(n) if right is None else np.asarray(right, dtype=np.float64)
    assert is_f32(src) and is_f32(dst)
    MT = sp.csr_array(sp.diags(dst) @ WT @ sp.diags(src))
    mult_rows = np.asarray(WT.sum(axis=1)).ravel()
    return Operator(MT, WT, src, dst, mult_rows, False)


def stored_operator(g):
    """The Operator of the host double, which iterates in double over the stored f32 matrix (oracle/host_abi.cpp)."""
    MT = sp.csr_array(g.download_transposed().astype(np.float64))
    ones = np.ones(MT.shape[0])
    return Operator(MT, MT, ones, ones, np.diff(MT.indptr), True)


def matvec_ld(MT, x):
    """M^T x with long-double products and row sums."""
    out = np.zeros(MT.shape[0], dtype=LD)
    if MT.nnz == 0:
        return out
    prods = MT.data.astype(LD) * np.asarray(x, dtype=LD)[MT.indices]
    counts = np.diff(MT.indptr)
    rows = np.flatnonzero(counts > 0)
    out[rows] = np.add.reduceat(prods, MT.indptr[:-1][rows])
    return out


# ------------------------------------------------------------------------------------------------------------------ the bounds
def f64_term(S, nnz):
    return (np.asarray(nnz, dtype=np.float64) + 8.0) * U52 * np.asarray(S, dtype=np.float64)


def row_bounds(got, ref, S, nnz, carried=0.0, quantum=0.0, factor=1.0):
    """(bound, |got - ref| / bound) per row.  ref: the exact result (long double), S: the sum of the magnitudes of every term of the
    row, nnz: its stream entries, carried: the bound the inputs brought along, quantum: the cold image's term, all of the f64 value
    the engine rounds to f32 after multiplying it by `factor`."""
    ref = np.asarray(ref, dtype=LD)
    inner = (f64_term(S, nnz) + carried + quantum) * abs(float(factor))
    bound = HALF_ULP32 * np.abs(ref).astype(np.float64) + MIN_NORMAL32 + inner
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    return bound, err / bound


class Vec:
    """An f64 vector of the engine as the reference knows it: value (long double), err (bound of |engine's f64 - value|), and the
    pieces row_bounds takes when the vector leaves as f32."""

    def __init__(self, value, err=None, S=None, nnz=None, quantum=None):
        self.value = np.asarray(value, dtype=LD)
        n = len(self.value)
        self.err = np.zeros(n) if err is None else np.asarray(err, dtype=np.float64)
        self.S = np.abs(self.value).astype(np.float64) if S is None else S
        self.nnz = np.zeros(n) if nnz is None else nnz
        self.quantum = np.zeros(n) if quantum is None else quantum

    def verdict(self, got, factor=1.0):
        """row_bounds of an f32 output that should be value * factor."""
        carried = self.err - f64_term(self.S, self.nnz) - self.quantum
        return row_bounds(got, self.value * LD(factor), self.S, self.nnz, np.maximum(carried, 0.0), self.quantum, factor)


def step(op, x, a, b=0.0, t=None, w=None, v=None, cold=False):
    """One step  y = a w (.) (M^T (v (.) x)) + b t  as a Vec.  The recurrence of the bound:
         B_y = (nnz + 8) 2^-52 S + |a| w |M^T| (v B_x) + |b| B_t + [cold] |a| w nnz 2^(e - E) |dst|,   S = |a| w |M^T| |v x| + |b t|."""
    n = op.n
    w64 = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    v64 = np.ones(n) if v is None else np.asarray(v, dtype=np.float64)
    xs = x.value * v64.astype(LD)
    y = LD(a) * w64.astype(LD) * matvec_ld(op.MT, xs)
    S = abs(a) * w64 * (op.absMT @ np.abs(xs).astype(np.float64))
    carried = abs(a) * w64 * (op.absMT @ (v64 * x.err))
    if b != 0.0:
        y = y + LD(b) * t.value
        S = S + abs(b) * np.abs(t.value).astype(np.float64)
        carried = carried + abs(b) * t.err
    quantum = abs(a) * w64 * op.quantum(xs) if cold else np.zeros(n)
    return Vec(y, f64_term(S, op.nnz_row) + carried + quantum, S, op.nnz_row, quantum)


def chebyshev_terms(op, p32, last, cold=False):
    """[T_1 .. T_last] of pgh_poly_terms: T_1 = p, T_2 = M^T p, T_k = 2 M^T T_{k-1} - T_{k-1}."""
    terms = [Vec(np.asarray(p32, dtype=np.float64))]
    for k in range(2, last + 1):
        prev = terms[-1]
        terms.append(step(op, prev, 1.0, cold=cold) if k == 2 else step(op, prev, 2.0, -1.0, prev, cold=cold))
    return terms


def power_terms(op, p32, last, cold=False):
    """[T_1 .. T_last] of the taylor form: T_k = M^T T_{k-1}."""
    terms = [Vec(np.asarray(p32, dtype=np.float64))]
    for _ in range(2, last + 1):
        terms.append(step(op, terms[-1], 1.0, cold=cold))
    return terms


def combination(terms, coeffs):
    """sum_k c_k T_k as the accumulator of closed_form_run holds it (one rounded multiply-add per term)."""
    value = sum(LD(c) * t.value for c, t in zip(coeffs, terms))
    S = sum(abs(c) * np.abs(t.value).astype(np.float64) for c, t in zip(coeffs, terms))
    err = sum(abs(c) * t.err for c, t in zip(coeffs, terms)) + f64_term(S, len(coeffs))
    return Vec(value, err, S, np.full(len(S), float(len(coeffs))))


def walk_operands(mode, pn, deg32, lam32):
    """(w, v, t) of k_bsf64_walk_operands in f64 from the graph's f32 degrees: mode 1 AbsorbingWalks w = d / (l + d), t = p l / (l + d);
    mode 2 SymmetricAbsorbingRandomWalks a = (1 + sqrt(1 + 4 d)) / 2, v = 1 / a, w = d / (a + d), t = p a / (a + d).  t's own roundings
    (three operations) ride in its err."""
    d = np.asarray(deg32, dtype=np.float64)
    pn = np.asarray(pn, dtype=LD)
    if mode == 1:
        lam = np.asarray(lam32, dtype=np.float64)
        w, v = d / (lam + d), None
        t = pn * lam.astype(LD) / (lam + d).astype(LD)
    else:
        a = (np.sqrt(d * 4.0 + 1.0) + 1.0) / 2.0
        w, v = d / (a + d), 1.0 / a
        t = pn * (a / (a + d)).astype(LD)
    return w, v, Vec(t, 4 * U52 * np.abs(t).astype(np.float64))


def recursive_reference(op, p32, x32, steps, alpha=0.85, mode=0, deg32=None, lam32=None, use_quotient=0, start_from_p=0, in_norm=1.0,
                        out_scale=1.0, err_kind=3, cold=False):
    """The loop of recursive_run_f64 (pgh_spmv.hip) for `steps` steps under max_iters = steps + 1 and a tolerance nothing meets:
    u_{k+1} = a w (.) M^T (v (.) x_k) + b t, x_{k+1} = u_{k+1} / sum(u_{k+1}) under use_quotient.  The check of iteration `it` runs while
    it < max_iters (loop_checks_at), so last_error is the residual |x_k - x_{k-1}| of the LAST BUT ONE step (0 for one step).
    Returns dict(out=Vec of the f32 result before its rounding, factor, iterations, spmv_count, last_error, in_norm, y_l1); y_l1 is
    the L1 norm of the larger of the two iterates that residual compares (a warm start of norm 3 000 against a normalised iterate of
    norm 1 leaves a residual of 3 000: its f64 rounding scales with the former)."""
    p = np.asarray(p32, dtype=np.float64)
    n = len(p)
    norm, reported = in_norm, 0.0
    if norm < 0:
        norm = reported = float(np.abs(p).sum())
    norm = 1.0 if norm == 0.0 else norm
    pn = Vec(p.astype(LD) / LD(norm), 2 * U52 * np.abs(p) / norm)       # the engine multiplies by 1 / norm, the double divides
    if mode == 0:
        a, b, w, v, t = alpha, 1.0 - alpha, None, None, pn
    else:
        w, v, t = walk_operands(mode, pn.value, deg32, lam32)
        t.err = t.err + pn.err
        a, b = 1.0, 1.0
    x = pn if start_from_p else Vec(np.asarray(x32, dtype=np.float64))
    it, spmv, last_error, y_l1 = 1, 0, 0.0, float(np.abs(x.value).sum())
    max_iters = steps + 1
    while it < max_iters:
        u = step(op, x, a, b, t, w, v, cold=cold)
        it += 1
        nxt = u
        if use_quotient:
            total = u.value.sum()
            mags = float(np.abs(u.value).sum())
            rel = (float(u.err.sum()) + (n + 8) * U52 * mags) / abs(float(total))      # of sum(u): n terms in any order
            nxt = Vec(u.value / total, u.err / abs(float(total)) + rel * np.abs(u.value / total).astype(np.float64), u.S / abs(float(total)),
                      u.nnz, u.quantum / abs(float(total)))
        checked = err_kind != 3 and it < max_iters
        if checked:
            d = np.abs(nxt.value - x.value)
            last_error = float(d.max() if err_kind == 2 else d.sum())
            if err_kind == 0:
                last_error /= n
            y_l1 = max(float(np.abs(nxt.value).sum()), float(np.abs(x.value).sum()))      # the larger of the two iterates compared
        x = nxt
        spmv += 1
    factor = norm if out_scale < 0 else out_scale
    return dict(out=x, factor=factor, iterations=it, spmv_count=spmv, converged=0, last_error=last_error, in_norm=reported, y_l1=y_l1)


def cancellation_probe(op, x32, alpha=0.85):
    """p = f32(-alpha / (1 - alpha) M^T x): one PageRank step from the warm start x then leaves alpha s_i + (1 - alpha) p_i, about
    2^-24 |s_i| -- the f32 rounding of THAT is worth 2^-48 |s_i|, so the engine's f64 row sum is seen at ~1e-15 relative."""
    s = matvec_ld(op.MT, np.asarray(x32, dtype=np.float64)).astype(np.float64)
    return (-alpha / (1.0 - alpha) * s).astype(F32)


# ------------------------------------------------------------------------------------------------------------------ the graphs
def small_graph(rng, weights="unit"):
    """kernel_checks.partition_test_graph(rng, 3001) (15 % isolated ids, sink-only and source-only ids, hub rows, a hub source, n no
    multiple of 4) as 0/1, with integer multiplicities up to 3 (few enough that the upload stays value-free: below a quarter more
    entries), or with f32-representable real weights in [0.5, 2).  Returns (W, isolated ids)."""
    from kernel_checks import partition_test_graph
    A, iso = partition_test_graph(rng, 3001)
    W = sp.csr_array(A).astype(np.float64)
    if weights == "mult":
        W.data = rng.choice([1.0, 2.0, 3.0], W.nnz, p=[0.88, 0.08, 0.04])
    elif weights == "real":
        W.data = rng.uniform(0.5, 2.0, W.nnz).astype(F32).astype(np.float64)
    return W, iso


def chain_graph(rng, n=20000, n_iso=2500):
    """One column block's worth of long segments: a row of 17 000 entries (at least 33 tiles of 512: the whole-wavefront chain of
    bsf64_fixup_tiles), one of 8 000 (the short-chain path across many tiles), rows of 1, 2 .. 1 100 entries (segment starts and ends
    on every alignment of a tile and of a lane's 8 entries), n_iso isolated ids.  W[src, dst] = 1.  Returns (W, isolated ids)."""
    ids = rng.permutation(n)
    iso, live = np.sort(ids[:n_iso]), ids[n_iso:]
    rows, cols = [], []
    targets = live[:1102]
    for k, dst in enumerate(targets):
        count = 17000 if k == 0 else (8000 if k == 1 else k - 1)
        rows.append(rng.choice(live, count, replace=False))
        cols.append(np.full(count, dst))
    for dst in live[1102:]:                                       # every other live id: a short row
        count = int(rng.integers(1, 4))
        rows.append(rng.choice(live, count, replace=False))
        cols.append(np.full(count, dst))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    W = sp.csr_array((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    W.sum_duplicates()
    assert W.nnz == len(rows)
    touched = np.zeros(n, dtype=bool)
    touched[rows], touched[cols] = True, True
    assert np.array_equal(np.flatnonzero(~touched), iso)
    return W, iso


def iso_tail_graph(rng, n=24000, n_live=4000):
    """4 000 live ids with 1 .. 8 out-edges each and 20 000 isolated ones: relabelled, the isolated rows are the last 20 000, more than
    the largest bin of the cold image holds (kPbBinRowsLarge = 16 384 rows, pgh_pb.hip).  With ONE bin in the image, the rows behind
    it are items of the work list that k_pb64_finish passes over while the isolated-row flag is clear (pb_build "cover").
    Returns (W, isolated ids)."""
    ids = rng.permutation(n)
    live, iso = ids[:n_live], np.sort(ids[n_live:])
    rows, cols = [], []
    for s in live:
        k = int(rng.integers(1, 9))
        rows.append(np.full(k, s))
        cols.append(rng.choice(live, k, replace=False))
    W = sp.csr_array((np.ones(sum(len(r) for r in rows)), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    return W, iso


def tiny_graphs():
    """One node with a self-loop, two nodes with one edge, a 65-node ring."""
    ring = sp.csr_array((np.ones(65), (np.arange(65), (np.arange(65) + 1) % 65)), shape=(65, 65))
    return {"loop1": sp.csr_array(np.ones((1, 1))), "edge2": sp.csr_array(np.array([[0.0, 1.0], [0.0, 0.0]])), "ring65": ring}


def f32_inverse(sums, power=1.0):
    """f32-representable 1 / sums^power (0 where the sum is 0): factors the test knows exactly."""
    sums = np.asarray(sums, dtype=np.float64)
    inv = np.divide(1.0, sums ** power, out=np.zeros_like(sums), where=sums != 0)
    return inv.astype(F32).astype(np.float64)


def upload(pg, W, kind):
    """(graph, Operator factory) for one upload route whose factors the test knows exactly:
       "none"       from_factored(W): value-free, no factor (integer W)
       "col"        from_factored(W, left = f32(1 / out-weight)): value-free, one-sided (the source scale)
       "two-sided"  from_factored(W, left, right) with f32(1 / sqrt) factors: value-free, both scales
       "valued"     scipy_sparse_to_backend of f32(diag(1 / out-weight) W): the valued stream"""
    from pygrank_amd.device import DeviceGraph
    W = sp.csr_array(W).astype(np.float64)
    out_w = np.asarray(W.sum(axis=1)).ravel()
    in_w = np.asarray(W.sum(axis=0)).ravel()
    if kind == "none":
        return DeviceGraph.from_factored(W), effective_matrix(W)
    if kind == "col":
        left = f32_inverse(out_w)
        return DeviceGraph.from_factored(W, left, None), effective_matrix(W, left, None)
    if kind == "two-sided":
        left, right = f32_inverse(out_w, 0.5), f32_inverse(in_w, 0.5)
        return DeviceGraph.from_factored(W, left, right), effective_matrix(W, left, right)
    assert kind == "valued"
    M = sp.csr_array(sp.diags(f32_inverse(out_w)) @ W)
    M.data = M.data.astype(F32).astype(np.float64)
    return pg.scipy_sparse_to_backend(M), effective_matrix(M, valued=True)


# ------------------------------------------------------------------------------------------------------------------ the calls
class Calls:
    """The C-ABI entries the f64 routes are reached through, on f32 numpy operands."""

    def __init__(self, pg):
        from pygrank_amd import _lib as L
        from pygrank_amd.device import DeviceMatrix, DeviceVector
        self.pg, self.L, self.Mat, self.Vec = pg, L, DeviceMatrix, DeviceVector
        self.hip = L.runtime_name().startswith("hip:")

    def vec(self, a):
        return self.Vec.from_host(np.ascontiguousarray(a, dtype=F32))

    def terms_rc(self, g, p32, skip, count, slab, first_col):
        p = self.vec(p32)                                    # (held until the call returns)
        return self.L.lib().pgh_poly_terms(g._h, p._h, 1, skip, count, slab._h, first_col)

    def terms(self, g, p32, skip, count, width=None, first_col=0, slab=None):
        """The slab (f64 copy of the f32 columns) after pgh_poly_terms wrote `count` terms from T_{skip+1} on at first_col."""
        n = g.shape[0]
        if slab is None:
            slab = self.Mat.from_host(np.full((n, count if width is None else width), SENTINEL))
        self.L.check(self.terms_rc(g, p32, skip, count, slab, first_col))
        return slab.numpy(), slab

    def cfg(self, steps, alpha=0.85, use_quotient=0, err_kind=3, in_norm=1.0, start_from_p=0, out_scale=1.0):
        # (tol = -1: no residual meets it, not even the exact 0 of a fixed point -- one node under the quotient)
        return self.L.LoopCfg(alpha=alpha, use_quotient=use_quotient, err_kind=err_kind, tol=-1.0, max_iters=steps + 1, end_modulo=1,
                              out_scale=out_scale, in_norm=in_norm, start_from_p=start_from_p, reserved=0)

    def recursive_rc(self, g, mode, p, ranks, lam, cfg, res):
        lib = self.L.lib()
        if mode == 0:
            return lib.pgh_ppr_run_f64(g._h, p._h, ranks._h, C.byref(cfg), C.byref(res))
        if mode == 1:
            return lib.pgh_absorb_run_f64(g._h, p._h, lam._h, ranks._h, C.byref(cfg), C.byref(res))
        return lib.pgh_sarw_run_f64(g._h, p._h, ranks._h, C.byref(cfg), C.byref(res))

    def recursive(self, g, mode, p32, x32, steps, lam32=None, **kw):
        """(f32 result as f64, pgh_loop_result) of `steps` steps; x32: the warm start (None: start_from_p)."""
        n = g.shape[0]
        cfg = self.cfg(steps, start_from_p=1 if x32 is None else 0, **kw)
        ranks = self.vec(np.full(n, SENTINEL) if x32 is None else x32)
        res = self.L.LoopResult()
        lam = self.vec(lam32) if lam32 is not None else None
        p = self.vec(p32)
        self.L.check(self.recursive_rc(g, mode, p, ranks, lam, cfg, res))
        return ranks.numpy(F32).astype(np.float64), res

    def poly(self, g, p32, coeffs, form):
        """pgh_poly_run with err_kind = ITERS over all of `coeffs` (form 2: taylor in f64, 1: the "chebyshev" recurrence)."""
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        cfg = self.L.LoopCfg(alpha=0.0, use_quotient=0, err_kind=3, tol=0.0, max_iters=len(coeffs) + 1, end_modulo=1, out_scale=1.0,
                             in_norm=1.0, start_from_p=0, reserved=0)
        out = self.vec(np.full(g.shape[0], SENTINEL))
        res = self.L.LoopResult()
        p = self.vec(p32)
        self.L.check(self.L.lib().pgh_poly_run(g._h, p._h, coeffs.ctypes.data_as(C.c_void_p), len(coeffs), form, out._h,
                                               C.byref(cfg), C.byref(res)))
        return out.numpy(F32).astype(np.float64), res


# ------------------------------------------------------------------------------------------------------------------ the inputs
def inputs(rng, n):
    """positive, signed, and signed over 30 decades (rows far below the largest cold product: where the fixed-point quantum shows)."""
    pos = (0.25 + rng.random(n)).astype(F32)
    sgn = (rng.choice([-1.0, 1.0], n) * (0.25 + rng.random(n))).astype(F32)
    dec = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-30, 0, n)).astype(F32)
    return {"positive": pos, "signed": sgn, "decades": dec}


def worst(case, check, got, vec, factor=1.0, rows=None):
    """Asserts an f32 output row by row against a Vec; records and returns the worst |error| / bound."""
    bound, ratio = vec.verdict(got, factor)
    if rows is not None:
        ratio = ratio[rows]
    top = float(ratio.max()) if len(ratio) else 0.0
    report(case, check, top)
    assert top <= 1.0, (case, check, top, int(np.argmax(ratio)))
    return top


# ------------------------------------------------------------------------------------------------------------------ the batteries
def check_products(calls, g, op, case, cold, rng):
    """Item 1: T_2 = M^T p for the three inputs, row by row; a repeated call gives the same bits."""
    for name, p in inputs(rng, op.n).items():
        got, _ = calls.terms(g, p, 1, 1)
        worst(case, "T2 " + name, got[:, 0], step(op, Vec(p.astype(np.float64)), 1.0, cold=cold))
        again, _ = calls.terms(g, p, 1, 1)
        assert np.array_equal(got, again), (case, name)


def check_probe(calls, g, op, case, cold, rng, alpha=0.85):
    """Item 2: the cancellation probe on pgh_ppr_run_f64, positive and signed x."""
    ins = inputs(rng, op.n)
    for name in ("positive", "signed"):
        x = ins[name]
        p = cancellation_probe(op, x, alpha)
        got, res = calls.recursive(g, 0, p, x, 1, alpha=alpha)
        ref = recursive_reference(op, p, x, 1, alpha=alpha, cold=cold)
        assert (res.iterations, res.spmv_count) == (2, 1), (case, res.iterations, res.spmv_count)
        worst(case, "probe " + name, got, ref["out"])
        longest = int(np.argmax(op.nnz_row))                  # (reported besides: the longest row, a hub bin / piece / long chain)
        report(case, "probe %s longest row" % name, ref["out"].verdict(got)[1][longest])


def check_chains(calls, g, op, case, cold, rng):
    """Item 4: T_2 .. T_8 from one call against the recurrence; skip / count / first_col splits give the same bits and leave the other
    columns of a sentinel-filled slab alone."""
    p = inputs(rng, op.n)["signed"]
    terms = chebyshev_terms(op, p, 8, cold)
    got, _ = calls.terms(g, p, 1, 7)
    for k in range(2, 9):
        worst(case, "chain", got[:, k - 2], terms[k - 1])
    split, slab = calls.terms(g, p, 1, 3, width=9, first_col=1)                 # T_2 .. T_4 -> columns 1 .. 3
    assert np.all(split[:, 0] == SENTINEL) and np.all(split[:, 4:] == SENTINEL), case
    split, slab = calls.terms(g, p, 4, 4, first_col=5, slab=slab)               # T_5 .. T_8 -> columns 5 .. 8
    assert np.all(split[:, 0] == SENTINEL) and np.all(split[:, 4] == SENTINEL), case
    assert np.array_equal(split[:, 1:4], got[:, 0:3]) and np.array_equal(split[:, 5:9], got[:, 3:7]), case
    one, _ = calls.terms(g, p, 0, 1)                                             # T_1 = p: the way in and out is exact
    assert np.array_equal(one[:, 0], p.astype(np.float64)), case


LOOP_CONFIGS = (dict(use_quotient=0, warm=True, in_norm=1.0, out_scale=1.0),
                dict(use_quotient=1, warm=True, in_norm=1.0, out_scale=1.0),
                dict(use_quotient=1, warm=False, in_norm=-1.0, out_scale=1.0),
                dict(use_quotient=0, warm=False, in_norm=-1.0, out_scale=-1.0))


def check_loop(calls, g, op, case, cold, rng, steps_list=(1, 2, 5), mode=0, deg32=None, lam32=None, configs=LOOP_CONFIGS,
               kinds=(1, 0, 2)):
    """Items 5 and 6: the recursive loop for 1, 2 and 5 steps against the numpy loop: with and without the quotient, from p (the
    engine computes the norm) and from a warm start, out_scale < 0; iterations, spmv_count, in_norm, and last_error for L1, Mabs, Linf
    within 1e-12 max(1, |y|_1)."""
    ins = inputs(rng, op.n)
    p, x = ins["positive"], (0.5 + rng.random(op.n)).astype(F32)
    for ci, conf in enumerate(configs):
        for steps in steps_list:
            for kind in (kinds if steps > 1 else kinds[:1]):
                kw = dict(use_quotient=conf["use_quotient"], in_norm=conf["in_norm"], out_scale=conf["out_scale"], err_kind=kind)
                warm = x if conf["warm"] else None
                got, res = calls.recursive(g, mode, p, warm, steps, lam32=lam32, **kw)
                ref = recursive_reference(op, p, warm, steps, mode=mode, deg32=deg32, lam32=lam32, start_from_p=0 if conf["warm"] else 1,
                                          cold=cold, **kw)
                label = (case, mode, ci, steps, kind)
                assert (res.iterations, res.spmv_count, res.converged) == (ref["iterations"], ref["spmv_count"], ref["converged"]), label
                assert abs(res.in_norm - ref["in_norm"]) <= 1e-12 * max(1.0, ref["in_norm"]), (label, res.in_norm, ref["in_norm"])
                assert abs(res.last_error - ref["last_error"]) <= 1e-12 * max(1.0, ref["y_l1"]), (label, res.last_error, ref["last_error"])
                if kind == kinds[0]:
                    worst(case, "loop mode %d" % mode, got, ref["out"], ref["factor"])


def check_walks(calls, g, op, case, cold, rng):
    """Item 6: one and three steps of the absorbing and the symmetric absorbing walk; operands formed as k_bsf64_walk_operands forms
    them, from the graph's own f32 degrees and an f32 lam."""
    deg = calls.pg.degrees(g).numpy(F32)
    lam = (0.25 + rng.random(op.n)).astype(F32)
    conf = (dict(use_quotient=0, warm=True, in_norm=1.0, out_scale=1.0), dict(use_quotient=1, warm=False, in_norm=-1.0, out_scale=1.0))
    check_loop(calls, g, op, case, cold, rng, (1, 3), 1, deg, lam, conf, (1,))
    check_loop(calls, g, op, case, cold, rng, (1, 3), 2, deg, None, conf, (1,))


def check_poly(calls, g, op, case, cold, rng):
    """Item 7: pgh_poly_run in f64 (closed_form_run on PolyStepF64: device state, deferred close, c != 0 and the accumulator), the
    taylor form and the "chebyshev" recurrence, against sum_k c_k T_k."""
    p = inputs(rng, op.n)["signed"]
    for form, coeffs in ((2, (0.5, 0.25, -0.125, 0.0625)), (1, (1.0, -0.5, 0.25)), (1, (0.25, 0.5, -0.75, 0.125))):
        got, res = calls.poly(g, p, coeffs, form)
        terms = (power_terms if form == 2 else chebyshev_terms)(op, p, len(coeffs), cold)
        assert res.iterations == len(coeffs) + 1, (case, form, res.iterations)
        if calls.hip:
            assert res.spmv_count == len(coeffs) - 1, (case, form, res.spmv_count)     # (the double pays the reference's trailing product)
        worst(case, "poly form %d" % form, got, combination(terms, coeffs))


def rows_exactly_zero(got, rows):
    """Every one of `rows` holds +0.0 (a passed-over row that kept a warm start's value, or a rounding's -0.0, does not)."""
    part = np.asarray(got)[rows]
    return bool(np.all(part == 0.0) and not np.any(np.signbit(part)))


def fixed_point_rows(op, xs, bits):
    """M^T xs with EVERY entry summed as k_pb64_finish sums a bin's cold entries: each product rounded to a multiple of 2^(e - bits)
    (fma(v, S, kMagic) rounds to nearest even, as np.rint does), the multiples added as integers, the sum scaled back and multiplied
    by dst_scale.  Value-free entries hand over xs_j * src_j once per unit of multiplicity."""
    e = op.product_exponent(xs)
    g = np.asarray(xs, dtype=np.float64) * op.src
    prods = (op.stream.data if op.valued else 1.0) * g[op.stream.indices]
    fixed = np.rint(np.ldexp(prods, bits - e)).astype(LD) * (1.0 if op.valued else op.stream.data)
    out = np.zeros(op.n, dtype=LD)
    rows = np.flatnonzero(np.diff(op.stream.indptr) > 0)
    out[rows] = np.add.reduceat(fixed, op.stream.indptr[:-1][rows])
    return np.ldexp(out.astype(np.float64), e - bits) * op.dst


def check_isolated(calls, g, op, case, iso, rng, alpha=0.85):
    """Item 8: rows without an entry that nobody references, for PageRank and the absorbing walk's term."""
    n = op.n
    live = np.setdiff1d(np.arange(n), iso)
    base = np.zeros(n, dtype=F32)
    base[live] = (0.25 + rng.random(len(live))).astype(F32)
    lam = np.full(n, 0.5, dtype=F32)
    one = int(iso[len(iso) // 2])
    others = iso[iso != one]
    for mode in (0, 1):
        lam32 = lam if mode == 1 else None
        for steps in (1, 2):                                 # every operand zero on every isolated row
            got, _ = calls.recursive(g, mode, base, base, steps, lam32=lam32, alpha=alpha)
            assert rows_exactly_zero(got, iso), (case, mode, steps)
            assert np.all(got != SENTINEL)
        # p non-zero on one isolated id; |p| a power of two so that p / |p| is exact
        p = np.zeros(n, dtype=F32)
        p[live[:3]] = 1.0
        p[one] = 1.0
        for steps in (1, 2):
            got, res = calls.recursive(g, mode, p, None, steps, lam32=lam32, alpha=alpha, in_norm=-1.0)
            assert res.in_norm == 4.0
            want = F32((1.0 - alpha) * 0.25) if mode == 0 else F32(0.25)
            assert got[one] == float(want), (case, mode, steps, got[one], float(want))
            assert np.all(got[others] == 0.0), (case, mode, steps)
        # the warm start non-zero on EVERY isolated id (wherever the layout puts them), p zero there: the steps alternate between two
        # buffers, and a passed-over row would keep the warm start's value after an even number of them
        x = base.copy()
        x[iso] = 3.0
        for steps in (1, 2, 3):
            got, _ = calls.recursive(g, mode, base, x, steps, lam32=lam32, alpha=alpha)
            assert rows_exactly_zero(got, iso), (case, mode, steps, got[one])
        # ... and the rows that are not isolated are what the loop gives (the isolated operand is inert: nobody references it)
        got, _ = calls.recursive(g, mode, base, x, 2, lam32=lam32, alpha=alpha)
        ref = recursive_reference(op, base, x, 2, alpha=alpha, mode=mode, deg32=calls.pg.degrees(g).numpy(F32), lam32=lam32)
        worst(case, "isolated mode %d" % mode, got, ref["out"])


def check_exact(calls, g, op, case, rng):
    """Item 3: integer weights, no normalisation, small integer inputs: T_2 .. T_6 equal numpy's integers to the bit wherever
    |T_k| < 2^24, and stay within the output rounding elsewhere.  Premise, from the operands: every product lies below 2^E
    (integers are then exact in the fixed-point sums: the quantum 2^(e - E) is at most 1) and every row's sum of magnitudes below 2^53."""
    assert not op.valued and np.all(op.src == 1.0) and np.all(op.dst == 1.0)
    p = np.zeros(op.n, dtype=F32)
    at = rng.choice(op.n, 40, replace=False)
    p[at] = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], len(at))
    MT = sp.csr_array(op.MT)
    t = p.astype(np.float64)
    want = []
    for k in range(2, 7):
        assert op.product_exponent(t) <= op.fixed_point_bits(), (case, k)
        mags = op.absMT @ np.abs(t) * (2.0 if k > 2 else 1.0) + np.abs(t)
        assert mags.max() < 2.0 ** 53, (case, k, mags.max())
        t = MT @ t if k == 2 else 2.0 * (MT @ t) - t              # exact: integers below 2^53 in every partial sum
        want.append(t)
    got, _ = calls.terms(g, p, 1, 5)
    for j, t in enumerate(want):
        small = np.abs(t) < 2.0 ** 24
        assert np.count_nonzero(small & (t != 0)) > 0
        assert np.array_equal(got[small, j], t[small]), (case, j + 2, int(np.argmax(got[:, j] != t)))
        assert np.all(np.abs(got[~small, j] - t[~small]) <= HALF_ULP32 * np.abs(t[~small])), (case, j + 2)


def check_refusals(calls):
    """Item 9: a rectangular graph and (on the engine: the double has no image to refuse) a graph without entries make the three
    *_run_f64 entries and pgh_poly_terms return non-zero with a message and leave sentinel-filled outputs untouched."""
    from pygrank_amd.device import DeviceGraph
    L = calls.L
    graphs = [DeviceGraph.from_factored(sp.csr_array((np.ones(3), ([0, 1, 4], [1, 2, 6])), shape=(5, 7)))]
    if calls.hip:
        graphs.append(calls.pg.scipy_sparse_to_backend(sp.csr_array((6, 6), dtype=np.float64)))
    for g in graphs:
        n_in, n_out = g.shape
        for mode in (0, 1, 2):
            for n_vec in {n_in, n_out}:
                ranks = calls.vec(np.full(n_vec, SENTINEL))
                res = L.LoopResult()
                p, lam = calls.vec(np.ones(n_vec)), calls.vec(np.ones(n_vec))
                rc = calls.recursive_rc(g, mode, p, ranks, lam, calls.cfg(1), res)
                assert rc != 0 and L.lib().pgh_last_error(), (g.shape, mode)
                assert np.all(ranks.numpy(F32) == F32(SENTINEL)), (g.shape, mode)
        for n_vec in {n_in, n_out}:
            slab = calls.Mat.from_host(np.full((n_vec, 2), SENTINEL))
            rc = calls.terms_rc(g, np.ones(n_vec), 1, 1, slab, 0)
            assert rc != 0 and L.lib().pgh_last_error(), g.shape
            assert np.all(slab.numpy() == SENTINEL), g.shape


def full_battery(calls, g, op, case, cold, iso, seed):
    """Items 1, 2, 4, 5, 6, 7 and 8 on one graph image."""
    rng = np.random.default_rng(seed)
    check_products(calls, g, op, case, cold, rng)
    check_probe(calls, g, op, case, cold, rng)
    check_chains(calls, g, op, case, cold, rng)
    check_loop(calls, g, op, case, cold, rng)
    check_walks(calls, g, op, case, cold, rng)
    check_poly(calls, g, op, case, cold, rng)
    if iso is not None and len(iso):
        check_isolated(calls, g, op, case, iso, rng)


def print_report(title):
    print("\n" + title)
    for case in sorted(F64_REPORT):
        if case in F64_FORMATS:
            print("  %-46s %s" % (case, F64_FORMATS[case].split("; f64 image: ")[-1]))
        print("  %-46s %s" % (case, "  ".join("%s=%.3f" % (k, v) for k, v in sorted(F64_REPORT[case].items()))))
