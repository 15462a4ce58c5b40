// include/pgh_measure.h: the cut forms of up to 64 score columns in one pass over the adjacency per slab, and the column statistics
// the measures' decisions are taken from.
//
// Reference counterparts: pygrank/measures/unsupervised.py:91-111 (Conductance: two conv and four dot per column) and :138-145
// (Density: one conv, one dot, two sums).
//
// pgh_cut_forms, per chunk of up to 32 score columns (64 with PGH_CUT_INTERNAL), all on the engine's stream:
//   k_cut_pack     X = [s | c], [n, 2 bp] with bp = the chunk's columns rounded up to whole float4s (the columns bc .. bp - 1 of either half
//                  are written as zeros: a row is whole 16-byte words and the slab's width is its own leading dimension)
//   pgh_spmm       Y = M^T X, the multi-seed pass as it stands
//   k_cut_forms    every row of X and Y once: the lanes of a row hold four score columns each (the mapping of k_mat_gemm, pgh_runtime.hip)
//                  and add y_s x_s, y_s x_c, y_c x_s, y_c x_c into f64 registers
//   k_fold_fields  the partial sums of the kSlabParts row parts, added in index order (pgh_slab.h)
// A row belongs to part (row / rows per workgroup) % kSlabParts whatever the launch: the grid only decides which workgroup walks which
// parts.  Lanes -> wavefront (shuffles) -> workgroup (LDS, wavefront order) -> parts (index order) are all fixed orders, so the forms
// are the same bits on every call and for every grid.  No atomics.
//
// C = M^T c is computed, not derived as max_rank * (M^T 1) - N: that difference cancels in f32 exactly where Conductance looks, the
// complement's internal weight <C, c> of a community that nearly fills the graph.
#include "pgh_slab.h"
#include "pgh_measure.h"

#include <cmath>

using namespace pgh;

namespace {
struct ColFactors {
    float f[kSlabMaxCols];
};

// Every virtual thread v < stride of the kSlabParts * kSlabBlock keeps ONE column (the stride is a multiple of b) and walks the slab with it;
// the threads of a part that share a column are folded through LDS in thread order.  partial: [kSlabParts][b][4] = sum, sum of squares,
// max, min.
__global__ __launch_bounds__(kSlabBlock) void k_col_stats(const float* __restrict__ m, int64_t n, int b, double* __restrict__ partial) {
    __shared__ double s_sum[kSlabBlock], s_sq[kSlabBlock];
    __shared__ float s_max[kSlabBlock], s_min[kSlabBlock];
    const int64_t total = n * b;
    const int64_t stride = ((int64_t)kSlabParts * kSlabBlock) / b * b;
    for (int part = blockIdx.x; part < kSlabParts; part += gridDim.x) {
        const int64_t first = (int64_t)part * kSlabBlock;
        double sum = 0.0, sq = 0.0;
        float mx = -INFINITY, mn = INFINITY;
        if (first + threadIdx.x < stride) {
            int64_t i = first + threadIdx.x;
            for (; i + 3 * stride < total; i += 4 * stride) {  // four independent loads per round
                const float v[4] = {m[i], m[i + stride], m[i + 2 * stride], m[i + 3 * stride]};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    sum += (double)v[u];
                    sq += (double)v[u] * (double)v[u];
                    mx = fmaxf(mx, v[u]);
                    mn = fminf(mn, v[u]);
                }
            }
            for (; i < total; i += stride) {
                const float v = m[i];
                sum += (double)v;
                sq += (double)v * (double)v;
                mx = fmaxf(mx, v);
                mn = fminf(mn, v);
            }
        }
        s_sum[threadIdx.x] = sum;
        s_sq[threadIdx.x] = sq;
        s_max[threadIdx.x] = mx;
        s_min[threadIdx.x] = mn;
        __syncthreads();
        for (int j = threadIdx.x; j < b; j += kSlabBlock) {
            const int start = (int)(((int64_t)j - first % b + b) % b);     // first thread of this part that owns column j
            double t = 0.0, q = 0.0;
            float hi = -INFINITY, lo = INFINITY;
            for (int k = start; k < kSlabBlock; k += b) {
                t += s_sum[k];
                q += s_sq[k];
                hi = fmaxf(hi, s_max[k]);
                lo = fminf(lo, s_min[k]);
            }
            double* o = partial + ((int64_t)part * b + j) * 4;
            o[0] = t;
            o[1] = q;
            o[2] = (double)hi;
            o[3] = (double)lo;
        }
        __syncthreads();
    }
}

// X[i, q] = s, X[i, bp + q] = c (BOTH) for the score columns first .. first + bc of `scores` ([n, b], rows of b floats); a thread
// writes one float4 of either half.  The products and differences are single f32 operations (no contraction into an fma: c is
// max_rank minus the ROUNDED s, what two vector-scalar calls of the engine store).
template <bool BOTH>
__global__ __launch_bounds__(kSlabBlock) void k_cut_pack(const float* __restrict__ scores, int64_t n, int b, int first, int bc, int bp, ColFactors factors,
                                                          float max_rank, float* __restrict__ X) {
    const int quads = bp >> 2, W = BOTH ? 2 * bp : bp;
    const int64_t total = n * quads;
    for (int64_t w = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; w < total; w += (int64_t)gridDim.x * kSlabBlock) {
        const int64_t i = w / quads;
        const int q0 = (int)(w - i * quads) * 4;
        const float* __restrict__ row = scores + i * b + first;
        float s[4], c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool live = q0 + u < bc;
            const int col = live ? q0 + u : 0;               // (a clamped index, then a select: no load under a branch)
            const float x = row[col];
            s[u] = live ? __fmul_rn(x, factors.f[first + col]) : 0.f;
            c[u] = live ? __fsub_rn(max_rank, s[u]) : 0.f;
        }
        float* __restrict__ o = X + i * W + q0;
        *reinterpret_cast<float4*>(o) = make_float4(s[0], s[1], s[2], s[3]);
        if (BOTH) *reinterpret_cast<float4*>(o + bp) = make_float4(c[0], c[1], c[2], c[3]);
    }
}

// X = [s | c] and Y = M^T X, both [n, W] with W = 2 bp (ALL) or bp (only s, only <N, s>).  lpr lanes (a power of two >= bp / 4) share a row;
// lane l of them holds the score columns 4 l .. 4 l + 3 and reads its float4 of either half of the row of X and of Y: every element of
// both slabs is read once, by one lane, as part of a 16-byte word.  The columns bc .. bp - 1 are zeros in X, so is their product.
// partial: [kSlabParts][bp][4] = <N, s>, <N, c>, <C, s>, <C, c>.
template <bool ALL>
__global__ __launch_bounds__(kSlabBlock) void k_cut_forms(const float* __restrict__ X, const float* __restrict__ Y, int64_t n, int bp, int lpr,
                                                           double* __restrict__ partial) {
    constexpr int F = ALL ? 4 : 1;
    __shared__ double s_red[kSlabBlock / 64][16][4 * F];
    const int W = ALL ? 2 * bp : bp;
    const int rows = kSlabBlock / lpr;
    const int l = threadIdx.x & (lpr - 1), r_in = threadIdx.x / lpr;
    const int q0 = 4 * l;
    const bool live = q0 < bp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t step = (int64_t)kSlabParts * rows;
    for (int part = blockIdx.x; part < kSlabParts; part += gridDim.x) {
        double a[4 * F];
#pragma unroll
        for (int k = 0; k < 4 * F; ++k) a[k] = 0.0;
        if (live) {
#pragma unroll 2
            for (int64_t i = (int64_t)part * rows + r_in; i < n; i += step) {
                const float* __restrict__ x = X + i * W + q0;
                const float* __restrict__ y = Y + i * W + q0;
                const float4 xs4 = *reinterpret_cast<const float4*>(x), ys4 = *reinterpret_cast<const float4*>(y);
                const float xs[4] = {xs4.x, xs4.y, xs4.z, xs4.w}, ys[4] = {ys4.x, ys4.y, ys4.z, ys4.w};
                if (ALL) {
                    const float4 xc4 = *reinterpret_cast<const float4*>(x + bp), yc4 = *reinterpret_cast<const float4*>(y + bp);
                    const float xc[4] = {xc4.x, xc4.y, xc4.z, xc4.w}, yc[4] = {yc4.x, yc4.y, yc4.z, yc4.w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const double ns = (double)ys[u], cs = (double)yc[u], sv = (double)xs[u], cv = (double)xc[u];
                        a[4 * u + 0] += ns * sv;
                        a[4 * u + 1] += ns * cv;
                        a[4 * u + 2] += cs * sv;
                        a[4 * u + 3] += cs * cv;
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) a[u] += (double)ys[u] * (double)xs[u];
                }
            }
        }
        // lanes of one residue mod lpr hold the same columns
#pragma unroll
        for (int k = 0; k < 4 * F; ++k) {
            double v = a[k];
            for (int off = 32; off >= lpr; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane < lpr) s_red[wave][lane][k] = v;
        }
        __syncthreads();
        for (int o = threadIdx.x; o < bp * 4; o += kSlabBlock) {
            const int col = o >> 2, f = o & 3;
            double r = 0.0;
            if (ALL || f == 0) {
                const int slot = ALL ? 4 * (col & 3) + f : (col & 3);
#pragma unroll
                for (int w = 0; w < kSlabBlock / 64; ++w) r += s_red[w][col >> 2][slot];
            }
            partial[((int64_t)part * bp + col) * 4 + f] = r;
        }
        __syncthreads();
    }
}

const char* const kCut = "pgh_cut_forms";
}  // namespace

PGH_WARM_KERNEL(k_col_stats)

extern "C" int pgh_mat_col_stats(pgh_mat_t m, double* out_host) {
    PGH_CHECK(m && out_host, "pgh_mat_col_stats: null argument");
    PGH_CHECK(m->b >= 1 && m->b <= 1024, "pgh_mat_col_stats: 1 to 1024 columns expected");
    const int b = m->b;
    if (m->n == 0) {
        for (int j = 0; j < b; ++j) {
            out_host[4 * j] = out_host[4 * j + 1] = 0.0;
            out_host[4 * j + 2] = -INFINITY;
            out_host[4 * j + 3] = INFINITY;
        }
        return 0;
    }
    Runtime& r = rt();
    PoolBuf partial;
    PGH_TRY(partial.alloc(sizeof(double) * (size_t)kSlabParts * b * 4));
    k_col_stats<<<parts_grid(), kSlabBlock, 0, r.stream>>>(m->data, m->n, b, partial.as<double>());
    PGH_HIP(hipGetLastError());
    return fold_fields_to_host<fold_kinds(kFoldSum, kFoldSum, kFoldMax, kFoldMin)>(partial.as<double>(), kSlabParts, b, b, out_host);
}

extern "C" int pgh_cut_forms(pgh_graph_t g, pgh_mat_t scores, const double* factors_host, double max_rank, int32_t forms,
                             double* out_host) {
    PGH_CHECK(g && scores && out_host, "pgh_cut_forms: null argument");
    PGH_CHECK(forms == PGH_CUT_ALL || forms == PGH_CUT_INTERNAL, "pgh_cut_forms: unknown forms");
    PGH_CHECK(scores->b >= 1, "pgh_cut_forms: at least one column expected");
    if (scores->b > kSlabMaxCols) return declined(PGH_MEASURE_DECLINED, kCut, "more than 64 columns");
    if (!std::isfinite((float)max_rank)) return declined(PGH_MEASURE_DECLINED, kCut, "non-finite max_rank");
    const int b = scores->b;
    ColFactors factors;
    for (int j = 0; j < kSlabMaxCols; ++j) factors.f[j] = 1.f;
    if (factors_host != nullptr)
        for (int j = 0; j < b; ++j) {
            factors.f[j] = (float)factors_host[j];
            if (!std::isfinite(factors.f[j])) return declined(PGH_MEASURE_DECLINED, kCut, "non-finite factor");
        }
    if (g->n_rows != g->n_cols) return declined(PGH_MEASURE_DECLINED, kCut, "the multi-seed pass needs a square matrix");
    if (!g->bsf.enabled || g->part_perm != nullptr) return declined(PGH_MEASURE_DECLINED, kCut, "the graph has no multi-seed layout");
    PGH_CHECK(scores->n == g->n_cols, "pgh_cut_forms: shape mismatch");
    const int64_t n = scores->n;
    const bool all = forms == PGH_CUT_ALL;
    double result[4 * kSlabMaxCols];
    for (int k = 0; k < 4 * kSlabMaxCols; ++k) result[k] = 0.0;
    if (n > 0 && g->nnz > 0) {
        Runtime& r = rt();
        const int per = all ? kSlabMaxCols / 2 : kSlabMaxCols;       // score columns per slab of <= 64
        const int bp0 = ((b < per ? b : per) + 3) & ~3;
        const size_t slab = sizeof(float) * (size_t)n * (size_t)(all ? 2 * bp0 : bp0);      // the first chunk is the widest
        // same-sized blocks come back from the runtime's pool on the next call: no allocation after the first
        PoolBuf X, Y, partial;
        PGH_TRY(X.alloc(slab));
        PGH_TRY(Y.alloc(slab));
        PGH_TRY(partial.alloc(sizeof(double) * (size_t)kSlabParts * bp0 * 4));
        const int grid = parts_grid();
        for (int first = 0; first < b; first += per) {
            const int bc = b - first < per ? b - first : per;
            const int bp = (bc + 3) & ~3, W = all ? 2 * bp : bp;
            const int lpr = lpr_for(bp);
            if (all) k_cut_pack<true><<<grid, kSlabBlock, 0, r.stream>>>(scores->data, n, b, first, bc, bp, factors, (float)max_rank, X.as<float>());
            else k_cut_pack<false><<<grid, kSlabBlock, 0, r.stream>>>(scores->data, n, b, first, bc, bp, factors, (float)max_rank, X.as<float>());
            PGH_HIP(hipGetLastError());
            pgh_mat_s mx, my;
            mx.data = X.as<float>();
            my.data = Y.as<float>();
            mx.n = my.n = n;
            mx.b = my.b = W;
            PGH_TRY(pgh_spmm(g, &mx, &my));
            if (all) k_cut_forms<true><<<grid, kSlabBlock, 0, r.stream>>>(X.as<float>(), Y.as<float>(), n, bp, lpr, partial.as<double>());
            else k_cut_forms<false><<<grid, kSlabBlock, 0, r.stream>>>(X.as<float>(), Y.as<float>(), n, bp, lpr, partial.as<double>());
            PGH_HIP(hipGetLastError());
            PGH_TRY(fold_fields_to_host<kFoldSums>(partial.as<double>(), kSlabParts, bp, bc, result + 4 * first));
        }
    }
    for (int k = 0; k < 4 * b; ++k) out_host[k] = result[k];
    return 0;
}
