// include/pgh_krylov.h: what follows the product of one Lanczos step in one pass, and the convergence residuals of up to 64 iterations
// of a Krylov-space filter in one pass over the basis slab.
//
// Reference counterpart: krylov_base (pygrank/algorithms/filters/krylov_space.py:16-37) -- per step `w - a*v`, `-= base[j-1] * norm`,
// `sum(next_w**2)`, `next_w / norm` and the column stack, each a pass over n-vectors with a temporary -- and the loop of
// ClosedFormGraphFilter._step (abstract_filters.py:248-253) with ConvergenceManager's residual (convergence.py:96-101): one
// V @ result product and one residual pass per iteration.
//
// Four kernels on the engine's stream:
//   k_lanczos_close<U, BASIS>  lane <-> four consecutive elements (16-byte loads and stores), grid-stride; the elements behind the last
//                              whole quad -- or all of them when an operand is not 16-byte aligned -- go one per lane.  The slab column
//                              is written with four 4-byte stores per lane (stride b).  HBM-streaming.
//   k_fold_regions             one workgroup folds the block partials of both sums in their order (pgh_slab.h).
//   k_krylov_residuals<LPR>    the lane mapping of k_mat_gemm (pgh_runtime.hip): LPR lanes share a row (same address: one request) and
//                              hold four probes each, the coefficients sit in LDS as doubles; instead of storing the [n, probes] product
//                              every lane keeps sum |.| and max |.| of its four probes over its rows, the workgroup folds its rows
//                              through LDS in row order and writes one partial per probe.
//   k_krylov_fold_probes       one workgroup folds the block partials of every probe in block order.
// Every grid is a function of the shape alone and no kernel uses atomics, so two calls on the same input return the same bits.
// The stored value (w - a v) - b u is formed from individually rounded f64 operations in that order: this file is compiled with
// contraction into fused multiply-adds switched off (as pgh_lfpr.hip; a difference that cancels comes out as in a plain f64 evaluation).
#include "pgh_slab.h"
#include "pgh_krylov.h"

#include <cmath>
#include <vector>

using namespace pgh;

#pragma clang fp contract(off)

namespace {
constexpr int kMaxResGrid = 1024;    // residual pass: 256 CUs x 4 workgroups (48 KB of LDS each)
static_assert(kPartialRegions >= 2, "one region of block partials per sum");
static_assert(PGH_KRYLOV_MAX_DIMS == 64 && PGH_KRYLOV_MAX_PROBES == 64, "the coefficient tile of k_krylov_residuals is 64 x 64 doubles");

template <bool HAS_U>
__device__ __forceinline__ float close_one(float w, float v, float u, double a, double b, double& sq, double& ov) {
    double t = (double)w - a * (double)v;
    if (HAS_U) t = t - b * (double)u;
    const float stored = (float)t;
    const double o = (double)stored;
    sq += o * o;
    ov += o * (double)v;
    return stored;
}

// No operand carries __restrict__ (loads_issued(), pgh_slab.h); out is distinct from every input, checked by the caller
template <bool HAS_U, bool HAS_BASIS>
__global__ __launch_bounds__(kSlabBlock) void k_lanczos_close(const float* w, const float* v, double a, const float* u, double b, int64_t n,
                                                               int64_t nvec, float* out, float* basis, int ld, int col,
                                                               double* __restrict__ partials) {
    __shared__ double s_red[4];
    const int64_t stride = (int64_t)gridDim.x * kSlabBlock;
    const int64_t gtid = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x;
    double sq = 0.0, ov = 0.0;
    for (int64_t q = gtid; q < nvec; q += stride) {
        const float4 w4 = reinterpret_cast<const float4*>(w)[q];
        const float4 v4 = reinterpret_cast<const float4*>(v)[q];
        float4 u4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (HAS_U) u4 = reinterpret_cast<const float4*>(u)[q];
        loads_issued();
        float4 o4;
        o4.x = close_one<HAS_U>(w4.x, v4.x, u4.x, a, b, sq, ov);
        o4.y = close_one<HAS_U>(w4.y, v4.y, u4.y, a, b, sq, ov);
        o4.z = close_one<HAS_U>(w4.z, v4.z, u4.z, a, b, sq, ov);
        o4.w = close_one<HAS_U>(w4.w, v4.w, u4.w, a, b, sq, ov);
        reinterpret_cast<float4*>(out)[q] = o4;
        if (HAS_BASIS) {
            float* row = basis + (4 * q) * (int64_t)ld + col;
            row[0] = o4.x;
            row[ld] = o4.y;
            row[2 * (int64_t)ld] = o4.z;
            row[3 * (int64_t)ld] = o4.w;
        }
    }
    for (int64_t i = 4 * nvec + gtid; i < n; i += stride) {
        const float o = close_one<HAS_U>(w[i], v[i], HAS_U ? u[i] : 0.f, a, b, sq, ov);
        out[i] = o;
        if (HAS_BASIS) basis[i * (int64_t)ld + col] = o;
    }
    sq = block_reduce_256<0>(sq, s_red);
    ov = block_reduce_256<0>(ov, s_red);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = sq;
        partials[kMaxPartials + blockIdx.x] = ov;
    }
}

// part[block][0 .. probes) = sum |r[i, t]|, part[block][probes .. 2 probes) = max |r[i, t]| over the rows of this workgroup
template <int LPR>
__global__ __launch_bounds__(kSlabBlock) void k_krylov_residuals(const float* __restrict__ m, int64_t n, int b, const double* __restrict__ deltas,
                                                                  int count, int probes, double* __restrict__ part) {
#pragma clang fp contract(fast)      // (one rounding per multiply-add: half the f64 instructions, and nothing here cancels)
    __shared__ double s_c[PGH_KRYLOV_MAX_DIMS * PGH_KRYLOV_MAX_PROBES];
    __shared__ double s_sum[kSlabBlock * 4];
    __shared__ double s_max[kSlabBlock * 4];
    for (int j = threadIdx.x; j < count * probes; j += kSlabBlock) s_c[j] = deltas[j];
    __syncthreads();
    constexpr int ROWS = kSlabBlock / LPR;
    const int q0 = (threadIdx.x % LPR) * 4, r_in = threadIdx.x / LPR;
    double sum[4] = {0.0, 0.0, 0.0, 0.0}, top[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = blockIdx.x * (int64_t)ROWS + r_in; i < n; i += (int64_t)gridDim.x * ROWS) {
        const float* __restrict__ row = m + i * b;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        int j = 0;
        for (; j + 4 <= count; j += 4) {                   // four independent loads per round
            const float a0 = row[j], a1 = row[j + 1], a2 = row[j + 2], a3 = row[j + 3];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (q0 + u < probes) {
                    acc[u] += (double)a0 * s_c[j * probes + q0 + u];
                    acc[u] += (double)a1 * s_c[(j + 1) * probes + q0 + u];
                    acc[u] += (double)a2 * s_c[(j + 2) * probes + q0 + u];
                    acc[u] += (double)a3 * s_c[(j + 3) * probes + q0 + u];
                }
        }
        for (; j < count; ++j) {
            const double a = (double)row[j];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (q0 + u < probes) acc[u] += a * s_c[j * probes + q0 + u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double mag = fabs(acc[u]);
            sum[u] += mag;
            top[u] = fmax(top[u], mag);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        s_sum[r_in * (LPR * 4) + q0 + u] = sum[u];
        s_max[r_in * (LPR * 4) + q0 + u] = top[u];
    }
    __syncthreads();
    if ((int)threadIdx.x < probes) {
        double s = 0.0, t = 0.0;
        for (int r = 0; r < ROWS; ++r) {
            s += s_sum[r * (LPR * 4) + threadIdx.x];
            t = fmax(t, s_max[r * (LPR * 4) + threadIdx.x]);
        }
        part[(size_t)blockIdx.x * (2 * probes) + threadIdx.x] = s;
        part[(size_t)blockIdx.x * (2 * probes) + probes + threadIdx.x] = t;
    }
}

// out[t] = sum over the blocks, out[probes + t] = max over the blocks: wavefront w takes probes w, w + 4, ..., its lanes the blocks
// l, l + 64, ... in order, then the wavefront reduction
__global__ __launch_bounds__(kSlabBlock) void k_krylov_fold_probes(const double* __restrict__ part, int blocks, int probes, double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < probes; t += 4) {
        double s = 0.0, top = 0.0;
        for (int k = lane; k < blocks; k += 64) {
            s += part[(size_t)k * (2 * probes) + t];
            top = fmax(top, part[(size_t)k * (2 * probes) + probes + t]);
        }
        s = wave_reduce_sum(s);
        top = wave_reduce_max(top);
        if (lane == 0) {
            out[t] = s;
            out[probes + t] = top;
        }
    }
}
}  // namespace

PGH_WARM_KERNEL(k_krylov_fold_probes)

extern "C" int pgh_lanczos_close(pgh_vec_t w, pgh_vec_t v, double a, pgh_vec_t u, double b, pgh_vec_t out, pgh_mat_t basis, int32_t col,
                                 double* sums_host) {
    PGH_CHECK(w && v && out && sums_host, "pgh_lanczos_close: null argument");
    const int64_t n = w->n;
    PGH_CHECK(v->n == n && out->n == n && (u == nullptr || u->n == n), "pgh_lanczos_close: the vectors differ in length");
    PGH_CHECK(basis == nullptr || basis->n == n, "pgh_lanczos_close: the slab and the vectors differ in length");
    PGH_CHECK(basis == nullptr || (col >= 0 && col < basis->b), "pgh_lanczos_close: col lies outside the slab");
    if (n > 0)
        PGH_CHECK(out->data != w->data && out->data != v->data && (u == nullptr || out->data != u->data),
                  "pgh_lanczos_close: out shares its memory with an input");
    if (!(std::isfinite(a) && std::isfinite(b))) return declined(PGH_KRYLOV_DECLINED, "pgh_lanczos_close", "a coefficient is not finite");
    if (n == 0) {
        sums_host[0] = sums_host[1] = 0.0;
        return 0;
    }
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const bool ok16 = aligned16(w->data) && aligned16(v->data) && aligned16(out->data) && (u == nullptr || aligned16(u->data));
    const int64_t nvec = ok16 ? n / 4 : 0;
    const int64_t lanes = nvec + (n - 4 * nvec);
    const int grid = grid_capped(lanes, kSlabBlock);
    const float* up = u ? u->data : v->data;
    float* bp = basis ? basis->data : nullptr;
    const int ld = basis ? basis->b : 0;
#define PGH_CLOSE(U, B) \
    k_lanczos_close<U, B><<<grid, kSlabBlock, 0, r.stream>>>(w->data, v->data, a, up, b, n, nvec, out->data, bp, ld, col, r.d_partials)
    if (u != nullptr && basis != nullptr) PGH_CLOSE(true, true);
    else if (u != nullptr) PGH_CLOSE(true, false);
    else if (basis != nullptr) PGH_CLOSE(false, true);
    else PGH_CLOSE(false, false);
#undef PGH_CLOSE
    PGH_HIP(hipGetLastError());
    return fold_regions_to_host(grid, 2, -1, sums_host);
}

extern "C" int pgh_krylov_residuals(pgh_mat_t basis, const double* deltas_host, int32_t count, int32_t probes, double* abssum_host,
                                    double* absmax_host) {
    PGH_CHECK(basis && deltas_host && abssum_host && absmax_host, "pgh_krylov_residuals: null argument");
    PGH_CHECK(basis->b >= 1 && basis->b <= PGH_KRYLOV_MAX_DIMS && count >= 1 && count <= basis->b,
              "pgh_krylov_residuals: 1 <= count <= basis.b <= 64");
    PGH_CHECK(probes >= 1 && probes <= PGH_KRYLOV_MAX_PROBES, "pgh_krylov_residuals: 1 <= probes <= 64");
    for (int64_t k = 0; k < (int64_t)count * probes; ++k)
        if (!std::isfinite(deltas_host[k])) return declined(PGH_KRYLOV_DECLINED, "pgh_krylov_residuals", "a coefficient is not finite");
    const int64_t n = basis->n;
    if (n == 0) {
        for (int t = 0; t < probes; ++t) abssum_host[t] = absmax_host[t] = 0.0;
        return 0;
    }
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const int lpr = lpr_for(probes);
    const int rows = kSlabBlock / lpr;
    int64_t g = (n + rows - 1) / rows;
    if (g > kMaxResGrid) g = kMaxResGrid;
    const int grid = (int)g;
    const size_t coeffs = (size_t)count * probes;
    double* d = nullptr;      // [count * probes] coefficients | [grid][2 probes] block partials | [2 probes] results
    PGH_TRY(pool_alloc(sizeof(double) * (coeffs + (size_t)grid * 2 * probes + 2 * (size_t)probes), (void**)&d));
    double* part = d + coeffs;
    double* folded = part + (size_t)grid * 2 * probes;
    std::vector<double> host(2 * (size_t)probes);
    hipError_t e = hipMemcpyAsync(d, deltas_host, sizeof(double) * coeffs, hipMemcpyHostToDevice, r.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r.stream);           // the caller's array may go away
    if (e == hipSuccess) {
#define PGH_RES(LPR) k_krylov_residuals<LPR><<<grid, kSlabBlock, 0, r.stream>>>(basis->data, n, basis->b, d, count, probes, part)
        switch (lpr) {
            case 16: PGH_RES(16); break;
            case 8: PGH_RES(8); break;
            case 4: PGH_RES(4); break;
            case 2: PGH_RES(2); break;
            default: PGH_RES(1); break;
        }
#undef PGH_RES
        k_krylov_fold_probes<<<1, kSlabBlock, 0, r.stream>>>(part, grid, probes, folded);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), folded, sizeof(double) * 2 * probes, hipMemcpyDeviceToHost, r.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r.stream);
    pool_free(d);
    PGH_HIP(e);
    for (int t = 0; t < probes; ++t) {
        abssum_host[t] = host[t];
        absmax_host[t] = host[probes + t];
    }
    return 0;
}
