// include/pgh_arnoldi.h: the two slab passes of an Arnoldi step -- the inner products of a vector with every basis column, and the pass
// that subtracts the projection, stores the next raw column and returns its inner products with the basis.
//
// Reference counterpart: the inner loop of arnoldi_iteration (pygrank/algorithms/filters/krylov_space.py:79-83) -- per earlier column a
// dot and an axpy, 2 k passes over n-vectors with a temporary each at step k.
//
// One kernel serves both entries, on the engine's stream:
//   k_arnoldi_pass<CLOSE>  the lane mapping of k_krylov_residuals (pgh_krylov.hip): LPR lanes share a row and hold four consecutive slab
//                          columns each, so a workgroup reads 256 / LPR whole rows -- `count` contiguous floats each -- and w[i] once
//                          (the lanes of a row ask for one address).  Every lane keeps the f64 sums of its four columns against the
//                          row's value; lane 0 of the row also keeps the sum of squares.
//                          CLOSE: the lane's partial projection c_j q_ij (its columns in ascending order) travels through shuffles
//                          and the row's lanes add the partials in ascending lane order -- every lane of a row holds the same f64
//                          sum --, the value w_i - sum is rounded ONCE to f32, stored by lane 0 (out and the slab column) and enters
//                          the sums as stored.
//   k_fold_fields          the partial sums of the kSlabParts row parts, added in index order (pgh_slab.h); the count + 1 sums travel
//                          as the fields of ceil((count + 1) / 4) columns.
// A row belongs to part (row / rows per workgroup) % kSlabParts whatever the launch: the grid only decides which workgroup walks which
// parts.  Lanes -> wavefront (shuffles) -> workgroup (LDS, wavefront order) -> parts (index order) are fixed orders: the same bits on
// every call and for every grid.  No atomics.
// Compiled with contraction into fused multiply-adds switched off (as pgh_krylov.hip): a projection that cancels against w comes out as
// in a plain f64 evaluation.
#include "pgh_slab.h"
#include "pgh_arnoldi.h"

#include <cmath>

using namespace pgh;

#pragma clang fp contract(off)

namespace {
static_assert(PGH_ARNOLDI_MAX_DIMS == kSlabMaxCols, "sixteen lanes of four columns hold a row");
constexpr int kMaxLpr = PGH_ARNOLDI_MAX_DIMS / 4;

// partial: [kSlabParts][cols][4] with slot s = 4 col + field: s < count the sum against slab column s, s == count the sum of squares,
// zeros behind.  No slab operand carries __restrict__ (loads_issued(), pgh_slab.h; CLOSE reads and writes the slab: col >= count, checked
// by the caller, keeps the column written apart from the columns read).
template <bool CLOSE>
__global__ __launch_bounds__(kSlabBlock) void k_arnoldi_pass(float* basis, int64_t n, int b, int count, const float* w, const double* coeffs,
                                                             float* out, int col, int lpr, int cols, double* __restrict__ partial) {
    __shared__ double s_c[PGH_ARNOLDI_MAX_DIMS];
    __shared__ double s_red[kSlabBlock / 64][kMaxLpr][5];
    const int rows = kSlabBlock / lpr;
    const int l = threadIdx.x & (lpr - 1), r_in = threadIdx.x / lpr;
    const int q0 = 4 * l;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row_lane0 = lane & ~(lpr - 1);
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    if (CLOSE) {
        if (threadIdx.x < PGH_ARNOLDI_MAX_DIMS) s_c[threadIdx.x] = (int)threadIdx.x < count ? coeffs[threadIdx.x] : 0.0;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] = s_c[q0 + u];
    }
    const int64_t step = (int64_t)kSlabParts * rows;
    for (int part = blockIdx.x; part < kSlabParts; part += gridDim.x) {
        double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int64_t i = (int64_t)part * rows + r_in; i < n; i += step) {
            const float* row = basis + i * b;
            float q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool live = q0 + u < count;
                const float x = row[live ? q0 + u : 0];          // (a clamped index, then a select: no load under a branch)
                q[u] = live ? x : 0.f;
            }
            const float wi = w[i];
            loads_issued();
            double o = (double)wi;
            if (CLOSE) {
                double mine = 0.0;
#pragma unroll
                for (int u = 0; u < 4; ++u) mine += c[u] * (double)q[u];
                double proj = 0.0;
                for (int k = 0; k < lpr; ++k) proj += __shfl(mine, row_lane0 + k, 64);     // the lanes of a row leave the loop together
                const float stored = (float)((double)wi - proj);
                if (l == 0) {
                    out[i] = stored;
                    if (col >= 0) basis[i * b + col] = stored;
                }
                o = (double)stored;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] += (double)q[u] * o;
            if (l == 0) a[4] += o * o;
        }
        // lanes of one residue mod lpr hold the same columns
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double v = a[k];
            for (int off = 32; off >= lpr; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane < lpr) s_red[wave][lane][k] = v;
        }
        __syncthreads();
        if ((int)threadIdx.x < cols * 4) {
            const int s = threadIdx.x;
            double r = 0.0;
            if (s <= count) {
                const int from = s < count ? s >> 2 : 0, slot = s < count ? s & 3 : 4;
#pragma unroll
                for (int v = 0; v < kSlabBlock / 64; ++v) r += s_red[v][from][slot];
            }
            partial[(int64_t)part * cols * 4 + s] = r;
        }
        __syncthreads();
    }
}

// the shared body: coeffs_host == nullptr is pgh_basis_dots
int arnoldi_pass(pgh_mat_t basis, int32_t count, pgh_vec_t w, const double* coeffs_host, pgh_vec_t out, int32_t col,
                 double* dots_host) {
    const bool close = coeffs_host != nullptr;
    const int64_t n = basis->n;
    if (n == 0) {
        for (int j = 0; j <= count; ++j) dots_host[j] = 0.0;
        return 0;
    }
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const int lpr = lpr_for(count);
    const int cols = (count + 1 + 3) / 4;
    PoolBuf partial, coeffs;
    PGH_TRY(partial.alloc(sizeof(double) * (size_t)kSlabParts * cols * 4));
    if (close) {
        PGH_TRY(coeffs.alloc(sizeof(double) * PGH_ARNOLDI_MAX_DIMS));
        PGH_HIP(hipMemcpyAsync(coeffs.p, coeffs_host, sizeof(double) * count, hipMemcpyHostToDevice, r.stream));
        PGH_HIP(hipStreamSynchronize(r.stream));           // the caller's array may go away
        k_arnoldi_pass<true><<<parts_grid(), kSlabBlock, 0, r.stream>>>(basis->data, n, basis->b, count, w->data, coeffs.as<double>(), out->data,
                                                                         col, lpr, cols, partial.as<double>());
    } else {
        k_arnoldi_pass<false><<<parts_grid(), kSlabBlock, 0, r.stream>>>(basis->data, n, basis->b, count, w->data, nullptr, nullptr, -1, lpr,
                                                                          cols, partial.as<double>());
    }
    PGH_HIP(hipGetLastError());
    double folded[(PGH_ARNOLDI_MAX_DIMS / 4 + 1) * 4];
    PGH_TRY(fold_fields_to_host<kFoldSums>(partial.as<double>(), kSlabParts, cols, cols, folded));
    for (int j = 0; j <= count; ++j) dots_host[j] = folded[j];
    return 0;
}
}  // namespace

PGH_WARM_KERNEL(k_arnoldi_pass<false>)

extern "C" int pgh_basis_dots(pgh_mat_t basis, int32_t count, pgh_vec_t w, double* dots_host) {
    PGH_CHECK(basis && w && dots_host, "pgh_basis_dots: null argument");
    PGH_CHECK(basis->b >= 1 && basis->b <= PGH_ARNOLDI_MAX_DIMS && count >= 1 && count <= basis->b, "pgh_basis_dots: 1 <= count <= basis.b <= 64");
    PGH_CHECK(w->n == basis->n, "pgh_basis_dots: the slab and the vector differ in length");
    return arnoldi_pass(basis, count, w, nullptr, nullptr, -1, dots_host);
}

extern "C" int pgh_arnoldi_close(pgh_mat_t basis, int32_t count, pgh_vec_t w, const double* coeffs_host, pgh_vec_t out, int32_t col,
                                 double* dots_host) {
    PGH_CHECK(basis && w && coeffs_host && out && dots_host, "pgh_arnoldi_close: null argument");
    PGH_CHECK(basis->b >= 1 && basis->b <= PGH_ARNOLDI_MAX_DIMS && count >= 1 && count <= basis->b,
              "pgh_arnoldi_close: 1 <= count <= basis.b <= 64");
    PGH_CHECK(w->n == basis->n && out->n == basis->n, "pgh_arnoldi_close: the slab and the vectors differ in length");
    PGH_CHECK(col < 0 || (col >= count && col < basis->b), "pgh_arnoldi_close: col is none (negative) or a column of the slab behind the columns read");
    if (basis->n > 0) PGH_CHECK(out->data != w->data, "pgh_arnoldi_close: out shares its memory with w");
    for (int j = 0; j < count; ++j)
        if (!std::isfinite(coeffs_host[j])) return declined(PGH_ARNOLDI_DECLINED, "pgh_arnoldi_close", "a coefficient is not finite");
    return arnoldi_pass(basis, count, w, coeffs_host, out, col < 0 ? -1 : col, dots_host);
}
