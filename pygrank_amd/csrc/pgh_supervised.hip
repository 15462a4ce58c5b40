// include/pgh_supervised.h: every sum over (score, known) pairs the closed-form supervised measures are made of, for up to 64 score
// columns in one streaming pass over the slab.
//
// Reference counterparts: pygrank/measures/supervised.py:93-333 (two to six elementwise passes and reductions per measure and column).
//
// pgh_pair_forms, all on the engine's stream:
//   k_pair_rows    b a multiple of 4: the lanes of a row hold four score columns each (the mapping of k_mat_gemm, pgh_runtime.hip, and
//                  k_cut_forms, pgh_measure.hip) and read them as one 16-byte word; every element of the slab is read once
//   k_pair_cols    every other b: a thread keeps ONE column and walks the slab with it (the mapping of k_col_stats, pgh_measure.hip)
//   k_pair_fold    the partial slots of the kSlabParts row parts, folded in a fixed order
// Known scores and exclude values are addressed through a (row stride, column stride) pair -- (1, 0) for a vector shared by the
// columns, (b, 1) for a matrix -- so one kernel body serves a vector, a matrix or (exclude) nothing.  A shared vector is read once
// per row: by the one lane group (k_pair_rows) or by the b threads (k_pair_cols, one 4-byte word of a line they all hit) that hold
// that row.
//
// Both kernels come in two instantiations: MOMENTS keeps 12 f64 accumulators per column and evaluates no logarithm, LOGS keeps 17.
//
// A row belongs to a part whatever the launch: the grid only decides which workgroup walks which parts.  Lanes -> wavefront
// (shuffles) -> workgroup (LDS, wavefront order) -> parts (k_pair_fold) are all fixed orders, so the slots are the same bits on every
// call and for every grid.  No atomics.
#include "pgh_slab.h"
#include "pgh_supervised.h"

#include <cmath>
#include <cstdint>

using namespace pgh;

namespace {
constexpr int kMoments = 12, kAll = 17;     // slots the two instantiations accumulate

struct PairFactors {
    double f[kSlabMaxCols];
};

// known or exclude: element (i, j) is at data[i * rs + j * cs]; data == nullptr (exclude only): nothing is excluded
struct Operand {
    const float* data;
    int64_t rs;
    int cs;
};

__host__ __device__ __forceinline__ constexpr bool slot_is_max(int f) { return f >= 8 && f <= 10; }

template <int NS>
__device__ __forceinline__ void slots_clear(double (&a)[NS]) {
#pragma unroll
    for (int f = 0; f < NS; ++f) a[f] = slot_is_max(f) ? -INFINITY : 0.0;
}

__device__ __forceinline__ double slot_join(int f, double a, double b) { return slot_is_max(f) ? fmax(a, b) : a + b; }

// the logarithms of a row's known score that do not depend on the column
struct KnownLogs {
    double log_k_eps, log_k;
};

__device__ __forceinline__ KnownLogs known_logs(double k, double eps) { return {log(k + eps), log(k)}; }

// score * factor as ONE rounded f64 product: contraction is off for this multiplication, so no sum or difference downstream fuses it
// into an fma and the maxima are exactly those of the products
__device__ __forceinline__ double rounded_product(double x, double y) {
#pragma clang fp contract(off)
    return x * y;
}

// one kept (s, k) pair into the slots of its column; s arrives as rounded_product(score, factor)
template <bool LOGS, int NS>
__device__ __forceinline__ void slots_add(double (&a)[NS], double s, double k, double eps, const KnownLogs& kl) {
    const double d = k - s, ad = fabs(d);
    a[0] += 1.0;
    a[1] += s;
    a[2] += s * s;
    a[3] += k;
    a[4] += k * k;
    a[5] += k * s;
    a[6] += ad;
    a[7] += d * d;
    a[8] = fmax(a[8], ad);
    a[9] = fmax(a[9], s);
    a[10] = fmax(a[10], k);
    a[11] += fabs(k);
    if constexpr (LOGS) {
        const double se = s + eps, lse = log(se);
        a[12] += k * lse;
        a[13] += (1.0 - k) * log(1.0 - s + eps);
        a[14] += se * lse;
        a[15] += se * kl.log_k_eps;
        a[16] += s * kl.log_k;
    }
}

// lpr lanes (a power of two >= b / 4, at most 16) share a row; lane l of them holds the score columns 4 l .. 4 l + 3.  Part p owns the
// rows i with (i / rows per workgroup) % kSlabParts == p.  partial: [kSlabParts][b][NS].
template <bool LOGS>
__global__ __launch_bounds__(kSlabBlock) void k_pair_rows(const float* __restrict__ S, int64_t n, int b, int lpr, Operand known, Operand exclude,
                                                           PairFactors factors, double eps, double* __restrict__ partial) {
    constexpr int NS = LOGS ? kAll : kMoments;
    __shared__ double s_red[kSlabBlock / 64][16][4 * NS];
    const int rows = kSlabBlock / lpr;
    const int l = threadIdx.x & (lpr - 1), r_in = threadIdx.x / lpr;
    const int q0 = 4 * l;
    const bool live = q0 < b;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t step = (int64_t)kSlabParts * rows;
    double fac[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) fac[u] = live ? factors.f[q0 + u] : 1.0;
    for (int part = blockIdx.x; part < kSlabParts; part += gridDim.x) {
        double a[4][NS];
#pragma unroll
        for (int u = 0; u < 4; ++u) slots_clear(a[u]);
        if (live) {
            for (int64_t i = (int64_t)part * rows + r_in; i < n; i += step) {
                const float4 s4 = *reinterpret_cast<const float4*>(S + i * b + q0);
                const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
                float kv[4], ev[4] = {0.f, 0.f, 0.f, 0.f};
                if (known.cs != 0) {
                    const float4 k4 = *reinterpret_cast<const float4*>(known.data + i * known.rs + q0);
                    kv[0] = k4.x, kv[1] = k4.y, kv[2] = k4.z, kv[3] = k4.w;
                } else {
                    kv[0] = kv[1] = kv[2] = kv[3] = known.data[i * known.rs];
                }
                if (exclude.data != nullptr) {
                    if (exclude.cs != 0) {
                        const float4 e4 = *reinterpret_cast<const float4*>(exclude.data + i * exclude.rs + q0);
                        ev[0] = e4.x, ev[1] = e4.y, ev[2] = e4.z, ev[3] = e4.w;
                    } else {
                        ev[0] = ev[1] = ev[2] = ev[3] = exclude.data[i * exclude.rs];
                    }
                }
                KnownLogs kl = {0.0, 0.0};
                if (LOGS && known.cs == 0) kl = known_logs((double)kv[0], eps);          // once per row, not per column
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (ev[u] == 0.f) {
                        const double k = (double)kv[u];
                        if (LOGS && known.cs != 0) kl = known_logs(k, eps);
                        slots_add<LOGS>(a[u], rounded_product((double)sv[u], fac[u]), k, eps, kl);
                    }
                }
            }
        }
        // lanes of one residue mod lpr hold the same columns
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int f = 0; f < NS; ++f) {
                double v = a[u][f];
                for (int off = 32; off >= lpr; off >>= 1) v = slot_join(f, v, __shfl_down(v, off, 64));
                if (lane < lpr) s_red[wave][lane][u * NS + f] = v;
            }
        }
        __syncthreads();
        for (int o = threadIdx.x; o < b * NS; o += kSlabBlock) {
            const int col = o / NS, f = o - col * NS;
            double r = s_red[0][col >> 2][(col & 3) * NS + f];
#pragma unroll
            for (int w = 1; w < kSlabBlock / 64; ++w) r = slot_join(f, r, s_red[w][col >> 2][(col & 3) * NS + f]);
            partial[((int64_t)part * b + col) * NS + f] = r;
        }
        __syncthreads();
    }
}

// Every virtual thread v < stride of the kSlabParts * kSlabBlock keeps ONE column (the stride is a multiple of b) and walks the slab with it;
// the threads of a part that share a column are folded through LDS in thread order, one slot at a time.  partial: [kSlabParts][b][NS].
template <bool LOGS>
__global__ __launch_bounds__(kSlabBlock) void k_pair_cols(const float* __restrict__ S, int64_t n, int b, Operand known, Operand exclude,
                                                           PairFactors factors, double eps, double* __restrict__ partial) {
    constexpr int NS = LOGS ? kAll : kMoments;
    __shared__ double s_v[kSlabBlock];
    const int64_t total = n * b;
    const int64_t stride = ((int64_t)kSlabParts * kSlabBlock) / b * b;
    const int64_t row_step = stride / b;
    for (int part = blockIdx.x; part < kSlabParts; part += gridDim.x) {
        const int64_t first = (int64_t)part * kSlabBlock;
        const int64_t v = first + threadIdx.x;
        double a[NS];
        slots_clear(a);
        if (v < stride) {
            int64_t row = v / b;
            const int col = (int)(v - row * b);
            const double fac = factors.f[col];
            const float* __restrict__ kp = known.data + (int64_t)col * known.cs;
            const float* __restrict__ ep = exclude.data != nullptr ? exclude.data + (int64_t)col * exclude.cs : nullptr;
            for (int64_t e = v; e < total; e += stride, row += row_step) {
                const float sv = S[e];
                const float kv = kp[row * known.rs];
                const float ev = ep != nullptr ? ep[row * exclude.rs] : 0.f;
                if (ev == 0.f) {
                    const double k = (double)kv;
                    KnownLogs kl = {0.0, 0.0};
                    if (LOGS) kl = known_logs(k, eps);
                    slots_add<LOGS>(a, rounded_product((double)sv, fac), k, eps, kl);
                }
            }
        }
        const int start = (int)(((int64_t)threadIdx.x - first % b + b) % b);     // first thread of this part that owns column threadIdx.x
#pragma unroll
        for (int f = 0; f < NS; ++f) {
            s_v[threadIdx.x] = a[f];
            __syncthreads();
            if (threadIdx.x < b) {
                double r = s_v[start];
                for (int k = start + b; k < kSlabBlock; k += b) r = slot_join(f, r, s_v[k]);
                partial[((int64_t)part * b + threadIdx.x) * NS + f] = r;
            }
            __syncthreads();
        }
    }
}

// out[PGH_PAIR_SLOTS j + f] = the parts' partial[.][j][f]: workgroup j; per slot, thread t joins the parts t, t + 256, ... in index
// order, a wavefront joins its lanes with shuffles, and the wavefronts are joined in wavefront order.  The slots ns .. 19 are zeros.
__global__ __launch_bounds__(kSlabBlock) void k_pair_fold(const double* __restrict__ partial, int cols, int ns, double* __restrict__ out) {
    __shared__ double s_w[kSlabBlock / 64];
    const int j = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int f = 0; f < ns; ++f) {
        double acc = partial[((int64_t)threadIdx.x * cols + j) * ns + f];
        for (int p = threadIdx.x + kSlabBlock; p < kSlabParts; p += kSlabBlock) acc = slot_join(f, acc, partial[((int64_t)p * cols + j) * ns + f]);
        for (int off = 32; off >= 1; off >>= 1) acc = slot_join(f, acc, __shfl_down(acc, off, 64));
        if (lane == 0) s_w[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            double r = s_w[0];
            for (int w = 1; w < kSlabBlock / 64; ++w) r = slot_join(f, r, s_w[w]);
            out[j * PGH_PAIR_SLOTS + f] = r;
        }
        __syncthreads();
    }
    if (threadIdx.x >= ns && threadIdx.x < PGH_PAIR_SLOTS) out[j * PGH_PAIR_SLOTS + threadIdx.x] = 0.0;
}

const char* const kPair = "pgh_pair_forms";
}  // namespace

extern "C" int pgh_pair_forms(pgh_mat_t scores, pgh_vec_t known_vec, pgh_mat_t known_mat, pgh_vec_t exclude_vec, pgh_mat_t exclude_mat,
                              const double* factors_host, double eps, int32_t groups, double* out_host) {
    PGH_CHECK(scores && out_host, "pgh_pair_forms: null argument");
    PGH_CHECK(groups == PGH_PAIR_MOMENTS || groups == PGH_PAIR_LOGS, "pgh_pair_forms: unknown groups");
    PGH_CHECK((known_vec != nullptr) != (known_mat != nullptr), "pgh_pair_forms: exactly one of known_vec and known_mat expected");
    PGH_CHECK(!(exclude_vec && exclude_mat), "pgh_pair_forms: at most one of exclude_vec and exclude_mat expected");
    PGH_CHECK(scores->b >= 1 && scores->n >= 0, "pgh_pair_forms: at least one column expected");
    if (scores->b > kSlabMaxCols) return declined(PGH_PAIR_DECLINED, kPair, "more than 64 columns");
    const int b = scores->b;
    const int64_t n = scores->n;
    PGH_CHECK(known_vec == nullptr || known_vec->n == n, "pgh_pair_forms: shape mismatch (known_vec)");
    PGH_CHECK(known_mat == nullptr || (known_mat->n == n && known_mat->b == b), "pgh_pair_forms: shape mismatch (known_mat)");
    PGH_CHECK(exclude_vec == nullptr || exclude_vec->n == n, "pgh_pair_forms: shape mismatch (exclude_vec)");
    PGH_CHECK(exclude_mat == nullptr || (exclude_mat->n == n && exclude_mat->b == b), "pgh_pair_forms: shape mismatch (exclude_mat)");
    if (!std::isfinite(eps)) return declined(PGH_PAIR_DECLINED, kPair, "non-finite eps");
    PairFactors factors;
    for (int j = 0; j < kSlabMaxCols; ++j) factors.f[j] = 1.0;
    if (factors_host != nullptr)
        for (int j = 0; j < b; ++j) {
            factors.f[j] = factors_host[j];
            if (!std::isfinite(factors.f[j])) return declined(PGH_PAIR_DECLINED, kPair, "non-finite factor");
        }
    const bool logs = groups == PGH_PAIR_LOGS;
    const int ns = logs ? kAll : kMoments;
    double result[PGH_PAIR_SLOTS * kSlabMaxCols];
    for (int j = 0; j < b; ++j)
        for (int f = 0; f < PGH_PAIR_SLOTS; ++f) result[PGH_PAIR_SLOTS * j + f] = slot_is_max(f) ? -INFINITY : 0.0;
    if (n > 0) {
        Runtime& r = rt();
        Operand known, exclude;
        known.data = known_vec ? known_vec->data : known_mat->data;
        known.rs = known_vec ? 1 : b;
        known.cs = known_vec ? 0 : 1;
        exclude.data = exclude_vec ? exclude_vec->data : (exclude_mat ? exclude_mat->data : nullptr);
        exclude.rs = exclude_mat ? b : 1;
        exclude.cs = exclude_mat ? 1 : 0;
        // same-sized blocks come back from the runtime's pool on the next call: no allocation after the first
        PoolBuf partial, folded;
        PGH_TRY(partial.alloc(sizeof(double) * (size_t)kSlabParts * b * ns));
        PGH_TRY(folded.alloc(sizeof(double) * (size_t)b * PGH_PAIR_SLOTS));
        const int grid = parts_grid();
        const bool words = b % 4 == 0 && aligned16(scores->data) && (known_mat == nullptr || aligned16(known.data)) &&
                           (exclude_mat == nullptr || aligned16(exclude.data));
        if (words) {
            const int lpr = lpr_for(b);
            if (logs) k_pair_rows<true><<<grid, kSlabBlock, 0, r.stream>>>(scores->data, n, b, lpr, known, exclude, factors, eps, partial.as<double>());
            else k_pair_rows<false><<<grid, kSlabBlock, 0, r.stream>>>(scores->data, n, b, lpr, known, exclude, factors, eps, partial.as<double>());
        } else {
            if (logs) k_pair_cols<true><<<grid, kSlabBlock, 0, r.stream>>>(scores->data, n, b, known, exclude, factors, eps, partial.as<double>());
            else k_pair_cols<false><<<grid, kSlabBlock, 0, r.stream>>>(scores->data, n, b, known, exclude, factors, eps, partial.as<double>());
        }
        k_pair_fold<<<b, kSlabBlock, 0, r.stream>>>(partial.as<double>(), b, ns, folded.as<double>());
        PGH_HIP(hipGetLastError());
        PGH_HIP(hipMemcpyAsync(result, folded.p, sizeof(double) * (size_t)b * PGH_PAIR_SLOTS, hipMemcpyDeviceToHost, r.stream));
        PGH_HIP(hipStreamSynchronize(r.stream));
    }
    for (int k = 0; k < PGH_PAIR_SLOTS * b; ++k) out_host[k] = result[k];
    return 0;
}
