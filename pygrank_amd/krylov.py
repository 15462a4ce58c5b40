"""The Krylov-space route of the closed-form filters: pygrank/algorithms/filters/krylov_space.py:16-85 on the engine.

``krylov_base`` runs the reference's Lanczos recurrence (no reorthogonalisation; it warns "not stable yet" like the reference) and
returns the basis V as an [n, k] device slab and the k x k host matrix H -- with the reference's quirk: krylov_space.py:35 puts
``base_norms[1:]`` on BOTH off-diagonals (not ``base_norms[:-1]``), and the error bound and every filter outcome depend on it.

Two routes:
  * fused (include/pgh_krylov.h): the recurrence lives in the graph's resident id space.  A step is one product (pgh_resident_step,
    mode 0), one pgh_dot and one pgh_lanczos_close that writes the next raw vector straight into the basis slab and returns its
    squared norm.  Normalisation never gets a pass of its own: the loop keeps the RAW vectors r_j and carries s_j = 1 / |r_j| as a
    host scalar into the product's multiplier (its nearest power of two, which the engine's f32 factor holds exactly; the rest stays
    on the host), the dot and the close's coefficients; one pgh_mat_div_cols over the finished slab normalises every column at once.
    (Images with a gather form add one pgh_resident_gather per step.)
  * primitive: the same recurrence in backend primitives, in the caller's ids.  Taken with ``fused=False``, where the library lacks
    the entries (the host test double), where an entry declines, where the image has no resident form, and for more than 64
    dimensions (combine_cols holds any width: those run here and do not raise).

``arnoldi_iteration`` (krylov_space.py:60-85; its consumer is autotune.HopTuner) has the same two routes, chosen by its ``fused``
argument (default False: the primitive loop, as before): the fused step is one product, one pgh_basis_dots, a k x k host solve and one
pgh_arnoldi_close (include/pgh_arnoldi.h).  It never raises on an exhausted space: zero columns follow, as in
the reference.

A deliberate deviation of the Lanczos route: a breakdown -- the next Lanczos vector vanishes, the Krylov space is exhausted -- raises an Exception that says
so.  The reference divides by zero there and returns NaN ranks.  "Vanishes" is |next_w| <= 2^-20 * sqrt(a_j^2 + b_{j-1}^2) (or an exact
zero): |w|^2 = a_j^2 + b_{j-1}^2 + |next_w|^2 for orthogonal Lanczos vectors, and the f32 storage of w leaves rounding noise of about
2^-24 |w| where the exact result is zero.
"""
import ctypes as C
import numbers
import warnings

import numpy as np

from pygrank_amd import _lib as L
from pygrank_amd import backend
from pygrank_amd import measures
from pygrank_amd.device import DeviceGraph, DeviceMatrix, DeviceVector

BREAKDOWN = 2.0 ** -20
MAX_FUSED_DIMS = L.KRYLOV_MAX_DIMS
TOO_ROUGH = 0.01                     # abstract_filters.py:208


def _device_graph(M):
    array = getattr(M, "array", M)
    return array if isinstance(array, DeviceGraph) else None


def _broke_down(norm, a, previous_norm):
    return not norm > BREAKDOWN * (a * a + previous_norm * previous_norm) ** 0.5


def _breakdown(step, degree):
    return Exception("Lanczos breakdown at step " + str(step) + " of " + str(degree) + ": the Krylov space of this personalization is "
                     "exhausted (ask for fewer krylov_dims)")


def _dense(matrix):
    return np.asarray(matrix.toarray() if hasattr(matrix, "toarray") else matrix, dtype=np.float64)


def _hessenberg(alphas, norms):
    """krylov_space.py:35 as written: base_norms[1:] on both off-diagonals."""
    return backend.diag(alphas, 0) + backend.diag(norms[1:], -1) + backend.diag(norms[1:], 1)


class KrylovBasis:
    """What one Lanczos run leaves behind: V [rows, k] (normalised columns; in the id space of `graph` when that is not None, in the
    caller's ids otherwise), H, the first product w_0 = conv(base[0]) and base[0] itself (each as a raw vector and its scale) for the error
    bound, the L2 norm of the personalization, the products it cost and the loss-of-orthogonality diagnostics sum(next_w * v_j) / |next_w|
    of the fused steps."""

    def __init__(self, V, H, graph, n, w0, w0_scale, first, first_scale, p_norm, spmv, fused, drift):
        self.V, self.H, self.graph, self.n = V, H, graph, int(n)
        self.w0, self.w0_scale, self.first, self.first_scale, self.p_norm = w0, float(w0_scale), first, float(first_scale), float(p_norm)
        self.spmv, self.fused, self.drift = int(spmv), bool(fused), drift
        self.dims = int(H.shape[0])

    def project(self, coefficients, scale=1.0):
        """V @ coefficients (times scale) in the caller's ids: ONE pass over the slab (pgh_mat_gemv) and, on the fused route, the one
        way out of the id space."""
        c = np.ascontiguousarray(coefficients, dtype=np.float64)
        if self.graph is None:
            return self.V.gemv(c * float(scale))
        inside = self.V.gemv(c)
        out = DeviceVector.empty(self.n)
        L.check(L.lib().pgh_resident_out(self.graph._h, inside._h, float(scale), out._h))
        return out

    def columns(self):
        """V in the caller's ids as an [n, k] slab (what pg.krylov_base returns)."""
        if self.graph is None:
            return self.V
        out = []
        for column in self.V.columns():
            vec = DeviceVector.empty(self.n)
            L.check(L.lib().pgh_resident_out(self.graph._h, column._h, 1.0, vec._h))
            out.append(vec)
        return DeviceMatrix.from_columns(out)

    def error_bound(self):
        """krylov_error_bound(V, H, M, personalization) with the defaults (Mabs, max_powers=1), from the kept w_0: no product."""
        lib = L.lib()
        got = C.c_double()
        errors = []
        unit = np.zeros(self.dims)
        unit[0] = 1.0
        for known, known_scale, coefficients in ((self.first, self.first_scale, unit), (self.w0, self.w0_scale, self.H[:, 0])):
            approx = self.V.gemv(np.ascontiguousarray(coefficients, dtype=np.float64))
            L.check(lib.pgh_scaled_residual(L.ERR_L1, approx._h, 1.0, known._h, float(known_scale), C.byref(got)))
            errors.append(got.value / max(self.n, 1))
        return max(errors)

    def residual_entry(self, fused=True):
        """pgh_krylov_residuals when `residuals` can use it on this basis, else None."""
        return L.entry("pgh_krylov_residuals") if fused and self.dims <= L.KRYLOV_MAX_DIMS else None

    def residuals(self, deltas, fused=True):
        """(sum_i |V @ d_t|, max_i |V @ d_t|, fused passes it took) for the columns d_t of the [k, T] matrix `deltas`: ONE pass over the
        slab (pgh_krylov_residuals) for T <= 64; with fused=False, where the library lacks the entry or where it declines, one
        pgh_mat_gemv and two reductions per column."""
        entry = self.residual_entry(fused)
        d = np.ascontiguousarray(deltas, dtype=np.float64)
        sums, tops = np.zeros(d.shape[1]), np.zeros(d.shape[1])
        if entry is not None and self.dims <= L.KRYLOV_MAX_DIMS and 1 <= d.shape[1] <= L.KRYLOV_MAX_PROBES:
            as_doubles = lambda a: a.ctypes.data_as(L.c_f64p)                 # noqa: E731
            status = entry(self.V._h, as_doubles(d), int(d.shape[0]), int(d.shape[1]), as_doubles(sums), as_doubles(tops))
            if L.accepted(status):
                return sums, tops, 1
        for t in range(d.shape[1]):
            change = abs(self.V.gemv(np.ascontiguousarray(d[:, t])))
            sums[t], tops[t] = change.sum(), (change.max() if len(change) else 0.0)
        return sums, tops, 0


def _exact_multiplier(scale):
    """(m, scale / m) with m the power of two nearest to `scale`: the step entries apply their multiplier as an f32 factor to an f32
    row sum, and a power of two is the factor that costs no rounding; what is left of the scale, a number in [0.7, 1.42], stays on the
    host in f64."""
    m = 2.0 ** round(np.log2(scale))
    return m, scale / m


def _lanczos_fused(g, p, degree, close):
    """The fused route; None when pgh_lanczos_close declined (nothing of the run is kept).  With r_j the raw vectors, s_j = 1 / |r_j|,
    (m_j, rho_j) = _exact_multiplier(s_j) and w' = m_j M^T r_j the stored product (conv(v_j) = rho_j w'):
      a_j = s_j rho_j <r_j, w'>,   r_{j+1} = (w' - (a_j s_j / rho_j) r_j) - (b_{j-1} s_{j-1} / rho_j) r_{j-1},   b_j = rho_j |r_{j+1}|."""
    lib = L.lib()
    n, n_int, n_gather = len(p), g._n_int, g._n_gather
    got, sums = C.c_double(), (C.c_double * 2)()

    def gather_form(vec):
        if not n_gather:
            return None
        out = DeviceVector.empty(n_gather)
        L.check(lib.pgh_resident_gather(g._h, vec._h, out._h))
        return out
    r = DeviceVector.empty(n_int)
    rg = DeviceVector.empty(n_gather) if n_gather else None
    L.check(lib.pgh_resident_in(g._h, p._h, 0.0, r._h, None if rg is None else rg._h))
    L.check(lib.pgh_dot(r._h, r._h, C.byref(got)))
    p_norm = got.value ** 0.5
    if not p_norm > 0:
        raise _breakdown(0, degree)
    slab = DeviceMatrix.empty(n_int, degree)
    L.check(lib.pgh_mat_set_col(slab._h, 0, r._h))
    first, s = r, 1.0 / p_norm
    previous, previous_s = None, 0.0
    alphas, norms, divisors, drift, w0, w0_scale = [], [], [p_norm], [], None, 1.0
    for j in range(degree):
        m, rho = _exact_multiplier(s)
        w = DeviceVector.empty(n_int)
        wg = DeviceVector.empty(n_gather) if n_gather else None      # (the step entry writes the gather form of its outcome)
        L.check(lib.pgh_resident_step(g._h, 0, r._h, None if rg is None else rg._h, m, None, 0.0, None, None, w._h,
                                      None if wg is None else wg._h, None))
        if j == 0:
            w0, w0_scale = w, rho
        L.check(lib.pgh_dot(r._h, w._h, C.byref(got)))
        a = s * rho * got.value
        last = j == degree - 1
        out = DeviceVector.empty(n_int)
        status = close(w._h, r._h, a * s / rho, None if previous is None else previous._h, norms[j - 1] * previous_s / rho if j else 0.0,
                       out._h, None if last else slab._h, 0 if last else j + 1, sums)
        if not L.accepted(status):
            return None
        raw_norm = sums[0] ** 0.5
        norm = rho * raw_norm
        alphas.append(a)
        norms.append(norm)
        if last:
            break
        if _broke_down(norm, a, norms[j - 1] if j else 0.0):
            raise _breakdown(j + 1, degree)
        drift.append(sums[1] * s / raw_norm)
        divisors.append(raw_norm)
        previous, previous_s = r, s
        r, s = out, 1.0 / raw_norm
        rg = gather_form(r)
    slab = slab.div_cols(divisors)                       # every column normalised at once (an f32 divisor per column)
    return KrylovBasis(slab, _hessenberg(alphas, norms), g, n, w0, w0_scale, first, 1.0 / p_norm, p_norm, degree, True, drift)


def _lanczos_primitive(M, p, degree):
    """krylov_space.py:19-37 in backend primitives, in the caller's ids, by the recurrence of _lanczos_fused: the RAW vectors r_j with
    their scales beside them (v_j = s_j r_j is never rounded to f32 on its own), the columns divided once at the end.
    The elementwise primitives compute in f32 with f32 coefficients, and a coefficient rounded to f32 leaves 2^-24 of the projection it
    should remove: the next vector is therefore formed by the one primitive that evaluates in f64 and rounds once, pgh_mat_gemv, over a
    three-column work slab that holds w', r_j and r_{j-1} in turn -- the arithmetic of pgh_lanczos_close at about three more passes."""
    p_norm = backend.dot(p, p) ** 0.5
    if not p_norm > 0:
        raise _breakdown(0, degree)
    raw, scales = [p], [1.0 / p_norm]
    norms, alphas, w0, w0_scale = [], [], None, 1.0
    zeros = backend.repeat(0.0, len(p))
    work = DeviceMatrix.from_columns([p, zeros, zeros])      # column j % 3 holds r_j
    for j in range(degree):
        r, s = raw[j], scales[j]
        m, rho = _exact_multiplier(s)
        w = backend.conv(r, M) * m
        if j == 0:
            w0, w0_scale = w, rho
        a = s * rho * backend.dot(r, w)
        alphas.append(a)
        work.set_column((j + 1) % 3, w)
        coefficients = np.zeros(3)
        coefficients[(j + 1) % 3], coefficients[j % 3] = 1.0, -(a * s / rho)
        if j > 0:
            coefficients[(j + 2) % 3] = -(norms[j - 1] * scales[j - 1] / rho)
        next_w = work.gemv(coefficients)
        work.set_column((j + 1) % 3, next_w)
        raw_norm = backend.dot(next_w, next_w) ** 0.5
        norms.append(rho * raw_norm)
        if j != degree - 1:
            if _broke_down(norms[j], a, norms[j - 1] if j else 0.0):
                raise _breakdown(j + 1, degree)
            raw.append(next_w)
            scales.append(1.0 / raw_norm)
    V = backend.combine_cols(raw).div_cols([1.0 / s for s in scales])
    return KrylovBasis(V, _hessenberg(alphas, norms), None, len(p), w0, w0_scale, p, 1.0 / p_norm, p_norm, degree, False, [])


def lanczos(M, personalization, krylov_space_degree, fused=True):
    """The KrylovBasis of krylov_base(M, personalization, krylov_space_degree); see the module docstring for the two routes."""
    warnings.warn("Krylov approximation is not stable yet (results may differ in future versions)")
    degree = int(krylov_space_degree)
    if degree < 1:
        raise Exception("krylov_space_degree must be at least 1")
    p = backend.to_primitive(getattr(personalization, "np", personalization))
    g = _device_graph(M)
    close = L.entry("pgh_lanczos_close") if fused and g is not None else None
    if close is not None and degree <= MAX_FUSED_DIMS and isinstance(p, DeviceVector) and g.shape[0] == g.shape[1] == len(p) \
            and len(p) > 0 and g._resident_lengths():
        basis = _lanczos_fused(g, p, degree, close)
        if basis is not None:
            return basis
    return _lanczos_primitive(g if g is not None else M, p, degree)


def krylov_base(M, personalization, krylov_space_degree, fused=True):
    """krylov_space.py:16-37 -> (V, H): V an [n, k] DeviceMatrix with normalised columns in the caller's ids, H the host k x k matrix."""
    basis = lanczos(M, personalization, krylov_space_degree, fused)
    return basis.columns(), basis.H


def krylov2original(V, filterH, krylov_space_degree):
    """krylov_space.py:40-44: the first column of V @ filterH.  A device V costs one pgh_mat_gemv.  The reference's quirk stays: a V
    given as an int or float means ones((k, k)) * V, on the host."""
    H = _dense(filterH)
    if isinstance(V, numbers.Number):
        k = int(krylov_space_degree)
        return backend.to_array((np.ones((k, k)) * V @ H)[:, 0])
    if isinstance(V, KrylovBasis):
        return V.project(H[:, 0])
    if isinstance(V, DeviceMatrix):
        return V.gemv(H[:, 0])
    return backend.to_array((np.asarray(V, dtype=np.float64) @ H)[:, 0])


def krylov_error_bound(V, H, M, personalization, measure=measures.Mabs, max_powers=1):
    """krylov_space.py:47-57.  A KrylovBasis in V's place with the default measure and max_powers reuses its w_0 (no product)."""
    if isinstance(V, KrylovBasis) and measure is measures.Mabs and max_powers == 1:
        return V.error_bound()
    personalization = backend.to_primitive(personalization)
    personalization = personalization / backend.dot(personalization, personalization) ** 0.5
    dims = V.dims if isinstance(V, KrylovBasis) else int(V.shape[1])
    graph = _device_graph(M)
    krylov_result, H = np.eye(dims), _dense(H)
    errors = []
    for power in range(max_powers + 1):
        errors.append(measure(personalization)(krylov2original(V, krylov_result, dims)))
        if power < max_powers:
            krylov_result = krylov_result @ H
            personalization = backend.conv(personalization, graph if graph is not None else M)
    return max(errors)


def _arnoldi_primitive(A, b, n):
    """krylov_space.py:75-85 as written, in backend primitives: 2 k vector passes at step k."""
    h = [[0 for _ in range(n)] for _ in range(n + 1)]
    Q = [backend.self_normalize(b)]
    for k in range(1, n):
        v = backend.conv(Q[k - 1], A)
        for j in range(k):
            h[j][k - 1] = backend.dot(Q[j], v)
            v = v - Q[j] * h[j][k - 1]
        h[k][k - 1] = backend.dot(v, v) ** 0.5
        Q.append(v / h[k][k - 1] if h[k][k - 1] != 0 else v * 0)
    return backend.combine_cols(Q), h


def _arnoldi_fused(g, b, n, dots, close):
    """The fused route (include/pgh_arnoldi.h); None when an entry declined (nothing of the run is kept).

    The slab holds the RAW columns r_j with a scale each, q_j = s_j r_j (s_0 = 1 / sum |b|: the reference's first column is L1-normalised).
    With (m, rho) = _exact_multiplier(s_{k-1}) and w' = m M^T r_{k-1} the stored product (conv(q_{k-1}) = rho w'), step k is
      c_j = s_j rho <r_j, w'>                                  one pgh_basis_dots
      (I + strictly_lower(G)) h = c,  G_ji = <q_j, q_i>        the host, f64: the coefficients of modified Gram-Schmidt for ANY Q
      r_k = w' - sum_j (h_j s_j / rho) r_j                     one pgh_arnoldi_close, written straight into column k
      h_{k,k-1} = rho |r_k|,  s_k = 1 / |r_k|,  G_kj = s_k s_j <r_k, r_j>      from the sums the close returns
    and one pgh_mat_div_cols over the finished slab normalises every column."""
    lib = L.lib()
    size, n_int, n_gather = len(b), g._n_int, g._n_gather
    got = C.c_double()
    r = DeviceVector.empty(n_int)
    rg = DeviceVector.empty(n_gather) if n_gather else None
    L.check(lib.pgh_resident_in(g._h, b._h, 0.0, r._h, None if rg is None else rg._h))
    L.check(lib.pgh_reduce(L.ABSSUM, r._h, C.byref(got)))
    scales = [1.0 / got.value if got.value != 0 else 1.0]
    slab = DeviceMatrix.empty(n_int, n)
    L.check(lib.pgh_mat_set_col(slab._h, 0, r._h))
    h = [[0 for _ in range(n)] for _ in range(n + 1)]
    gram = np.zeros((n, n))
    for k in range(1, n):
        m, rho = _exact_multiplier(scales[k - 1])
        w = DeviceVector.empty(n_int)
        wg = DeviceVector.empty(n_gather) if n_gather else None      # (the step entry writes the gather form of its outcome)
        L.check(lib.pgh_resident_step(g._h, 0, r._h, None if rg is None else rg._h, m, None, 0.0, None, None, w._h,
                                      None if wg is None else wg._h, None))
        sums = np.zeros(k + 1)
        status = dots(slab._h, k, w._h, sums.ctypes.data_as(L.c_f64p))
        if not L.accepted(status):
            return None
        s = np.asarray(scales)
        c = s * rho * sums[:k]
        coefficients = np.zeros(k)
        for j in range(k):                                   # the unit lower triangular solve
            coefficients[j] = c[j] - gram[j, :j] @ coefficients[:j]
        out = DeviceVector.empty(n_int)
        status = close(slab._h, k, w._h, np.ascontiguousarray(coefficients * s / rho).ctypes.data_as(L.c_f64p), out._h, k,
                       sums.ctypes.data_as(L.c_f64p))
        if not L.accepted(status):
            return None
        for j in range(k):
            h[j][k - 1] = float(coefficients[j])
        raw_norm = sums[k] ** 0.5
        h[k][k - 1] = float(rho * raw_norm)
        scales.append(1.0 / raw_norm if raw_norm != 0 else 1.0)      # krylov_space.py:84: a vanished vector stays a zero column
        gram[k, :k] = scales[k] * s * sums[:k]
        r = out
        if n_gather and k < n - 1:
            rg = DeviceVector.empty(n_gather)
            L.check(lib.pgh_resident_gather(g._h, r._h, rg._h))
    slab = slab.div_cols([1.0 / s for s in scales])        # every column normalised at once (an f32 divisor per column)
    columns = []
    for column in slab.columns():
        vec = DeviceVector.empty(size)
        L.check(lib.pgh_resident_out(g._h, column._h, 1.0, vec._h))
        columns.append(vec)
    return DeviceMatrix.from_columns(columns), h


def arnoldi_run(A, b, n, fused=False):
    """(Q, h, route) of arnoldi_iteration: route is "fused" or "primitive"."""
    n = int(n)
    graph = _device_graph(A)
    A = graph if graph is not None else A
    b = getattr(b, "np", b)
    dots = L.entry("pgh_basis_dots") if fused and graph is not None else None
    close = L.entry("pgh_arnoldi_close") if dots is not None else None
    if close is not None and 1 <= n <= L.ARNOLDI_MAX_DIMS and isinstance(b, DeviceVector) and graph.shape[0] == graph.shape[1] == len(b) \
            and len(b) > 0 and graph._resident_lengths():
        result = _arnoldi_fused(graph, b, n, dots, close)
        if result is not None:
            return result[0], result[1], "fused"
    Q, h = _arnoldi_primitive(A, backend.to_primitive(b), n)
    return Q, h, "primitive"


def arnoldi_iteration(A, b, n, fused=False):
    """krylov_space.py:60-85: a basis of the Krylov subspace of A spanned from b by modified Gram-Schmidt.  Returns (Q as an [m, n] slab
    in the caller's ids, h as an (n + 1) x n list of lists; upper Hessenberg).

    fused=False (default): the reference's loop in backend primitives -- a dot and an axpy per earlier column, 2 k vector passes at
    step k.  fused=True: a step is one product in the graph's resident id space, one pgh_basis_dots, a k x k host solve and one
    pgh_arnoldi_close (_arnoldi_fused).  Where the library lacks the entries (the host test double), where an
    entry declines, where the image has no resident form or is not square, for more than 64 columns and for a host `b` the primitive
    loop runs and nothing raises.  An exhausted space appends zero columns on either route, as in the reference."""
    Q, h, _ = arnoldi_run(A, b, n, fused)
    return Q, h
