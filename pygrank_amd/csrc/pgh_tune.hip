// include/pgh_tune.h: the AUC of up to 64 probes of a closed-form filter in one streaming pass over the stored powers.
//
// Reference counterparts: the inner evaluation of the tuner (pygrank/algorithms/autotune/parameterized.py:135-145: one rank() and one
// AUC per candidate) and measures/supervised.py:255-263 (sklearn roc_curve + auc: ties at their mid-rank).
//
// Three kernels per call, all on the engine's stream:
//   k_probe_positives  one workgroup per probe: the scores of the plan's positives (the arithmetic of k_mat_gemm, pgh_runtime.hip),
//                      sorted ascending in LDS (bitonic), stored as sorted[probe][num_positive]
//   k_probe_stream     every negative row once: its scores for all probes, two binary searches per probe in that probe's sorted
//                      positives, lb = positives below the score and ub = positives not above it: g = m - ub positives are
//                      strictly above the row, e = ub - lb tie with it, and 2 g + e = 2 m - (ub + lb).
//                      Lanes add ub + lb into 64-bit integers; wavefronts (shuffles), workgroups (LDS) and the device (one integer
//                      atomic per workgroup and probe) sum integers, so nothing depends on the grid or on arrival order.
//   the host forms     auc[q] = (2 m n_neg - T_q) / (2 m n_neg)
#include "pgh_slab.h"
#include "pgh_tune.h"

#include <cmath>
#include <memory>

using namespace pgh;

struct pgh_probe_plan_s {
    uint8_t* cls = nullptr;      // [n] 0 excluded, 1 negative, 2 positive
    int32_t* pos_idx = nullptr;  // [n_pos] rows of the positives (any order: their scores are sorted per probe)
    int64_t  n = 0, n_pos = 0, n_neg = 0;
};

namespace {
// rows of the positives, appended in arrival order (the slot counter never passes n_pos: the same predicate counted them)
__global__ __launch_bounds__(kSlabBlock) void k_plan_positives(const uint8_t* __restrict__ cls, int64_t n, int64_t n_pos, int32_t* __restrict__ pos_idx,
                                                                unsigned long long* __restrict__ cursor) {
    for (int64_t i = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSlabBlock) {
        if (cls[i] != 2) continue;
        const unsigned long long slot = atomicAdd(cursor, 1ull);
        if (slot < (unsigned long long)n_pos) pos_idx[slot] = (int32_t)i;
    }
}

// sorted[q][0 .. m): the scores of the positives under probe q, ascending.  m <= PGH_TUNE_MAX_POSITIVES.
__global__ __launch_bounds__(kSlabBlock) void k_probe_positives(const float* __restrict__ slab, int b, const double* __restrict__ coeffs, int terms, int probes,
                                                                 const int32_t* __restrict__ pos_idx, int m, int padded /* power of two >= m */,
                                                                 float* __restrict__ sorted) {
    __shared__ float s_v[PGH_TUNE_MAX_POSITIVES];
    const int q = blockIdx.x;
    for (int k = threadIdx.x; k < padded; k += kSlabBlock) {
        float v = INFINITY;                                  // padding sorts last
        if (k < m) {
            const float* __restrict__ row = slab + (int64_t)pos_idx[k] * b;
            double acc = 0.0;
            for (int j = 0; j < terms; ++j) acc += (double)row[j] * coeffs[j * probes + q];
            v = (float)acc;
        }
        s_v[k] = v;
    }
    __syncthreads();
    bitonic_sort_lds<kSlabBlock>(
        padded, [&](int i, int j) { return s_v[i] < s_v[j]; },
        [&](int i, int j) {
            const float x = s_v[i];
            s_v[i] = s_v[j];
            s_v[j] = x;
        });
    for (int k = threadIdx.x; k < m; k += kSlabBlock) sorted[(int64_t)q * m + k] = s_v[k];
}

// first index of the ascending run s[0 .. m) whose value is not below v (STRICT = false) or is above v (STRICT = true)
template <bool STRICT>
__device__ __forceinline__ int bound(const float* s, int m, float v) {
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float x = s[mid];
        if (STRICT ? (x <= v) : (x < v)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// LPR lanes share a row and hold four probes each (the mapping of k_mat_gemm); a row's leading `terms` floats arrive as 16-byte
// loads when the slab's rows are 16-byte aligned.  IN_LDS: the sorted positives were copied into LDS behind the coefficients.
template <int LPR, bool IN_LDS>
__global__ __launch_bounds__(kSlabBlock) void k_probe_stream(const float* __restrict__ slab, int64_t n, int b, int vec_ok, const double* __restrict__ coeffs,
                                                              int terms, int probes, const uint8_t* __restrict__ cls,
                                                              const float* __restrict__ sorted, int m, unsigned long long* __restrict__ totals) {
    extern __shared__ double s_dyn[];
    __shared__ unsigned long long s_tot[64];
    double* s_c = s_dyn;                                     // [terms * probes]
    float* s_pos = reinterpret_cast<float*>(s_dyn + terms * probes);   // [probes * m] when IN_LDS
    for (int j = threadIdx.x; j < terms * probes; j += kSlabBlock) s_c[j] = coeffs[j];
    if (IN_LDS)
        for (int j = threadIdx.x; j < probes * m; j += kSlabBlock) s_pos[j] = sorted[j];
    if (threadIdx.x < 64) s_tot[threadIdx.x] = 0;
    __syncthreads();
    constexpr int ROWS = kSlabBlock / LPR;
    const int q0 = (threadIdx.x % LPR) * 4, r_in = threadIdx.x / LPR;
    const float* __restrict__ pos = IN_LDS ? s_pos : sorted;
    unsigned long long tot[4] = {0, 0, 0, 0};
    for (int64_t i = blockIdx.x * (int64_t)ROWS + r_in; i < n; i += (int64_t)gridDim.x * ROWS) {
        if (cls[i] != 1) continue;
        const float* __restrict__ row = slab + i * b;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < terms; j += 4) {
            float a[4];
            if (vec_ok) {                                    // b % 4 == 0 and terms <= b: the whole quad lies inside the row
                const float4 v = *reinterpret_cast<const float4*>(row + j);
                a[0] = v.x, a[1] = v.y, a[2] = v.z, a[3] = v.w;
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) a[t] = j + t < terms ? row[j + t] : 0.f;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (j + t < terms) {
                    const double x = (double)a[t];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (q0 + u < probes) acc[u] += x * s_c[(j + t) * probes + q0 + u];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (q0 + u < probes) {
                const float v = (float)acc[u];
                const float* s = pos + (int64_t)(q0 + u) * m;
                tot[u] += (unsigned long long)(bound<false>(s, m, v) + bound<true>(s, m, v));
            }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned long long w = wave_sum_u64(tot[u], LPR);          // lanes of one residue mod LPR hold the same probes
        if ((threadIdx.x & 63) < LPR && q0 + u < probes && w != 0) atomicAdd(&s_tot[q0 + u], w);
    }
    __syncthreads();
    if (threadIdx.x < probes && s_tot[threadIdx.x] != 0) atomicAdd(&totals[threadIdx.x], s_tot[threadIdx.x]);
}

const char* const kAuc = "pgh_probe_auc";
}  // namespace

PGH_WARM_KERNEL(k_plan_positives)

extern "C" int pgh_probe_plan_create(pgh_vec_t known, pgh_vec_t exclude, pgh_probe_plan_t* out) {
    PGH_CHECK(known && out, "pgh_probe_plan_create: null argument");
    PGH_CHECK(exclude == nullptr || exclude->n == known->n, "pgh_probe_plan_create: known and exclude differ in length");
    PGH_CHECK(known->n < 2147483647LL, "pgh_probe_plan_create: vector too long");
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const int64_t n = known->n;
    std::unique_ptr<pgh_probe_plan_s, int (*)(pgh_probe_plan_t)> plan(new pgh_probe_plan_s(), pgh_probe_plan_destroy);
    plan->n = n;
    PGH_TRY(pool_alloc((size_t)(n > 0 ? n : 1), (void**)&plan->cls));
    unsigned long long counts[4];
    PGH_TRY(classify_labels(known, exclude, plan->cls, counts));
    plan->n_pos = (int64_t)counts[1];
    plan->n_neg = (int64_t)counts[2];
    PGH_TRY(pool_alloc(sizeof(int32_t) * (size_t)(plan->n_pos > 0 ? plan->n_pos : 1), (void**)&plan->pos_idx));
    if (plan->n_pos > 0) {
        PoolBuf cursor;
        PGH_TRY(cursor.alloc(sizeof(unsigned long long)));
        PGH_HIP(hipMemsetAsync(cursor.p, 0, sizeof(unsigned long long), r.stream));
        k_plan_positives<<<grid_capped(n, kSlabBlock * 8), kSlabBlock, 0, r.stream>>>(plan->cls, n, plan->n_pos, plan->pos_idx,
                                                                             cursor.as<unsigned long long>());
        PGH_HIP(hipGetLastError());
        PGH_HIP(hipStreamSynchronize(r.stream));
    }
    *out = plan.release();
    return 0;
}

extern "C" int pgh_probe_plan_info(pgh_probe_plan_t plan, int64_t* num_positive, int64_t* num_negative) {
    PGH_CHECK(plan, "pgh_probe_plan_info: null plan");
    if (num_positive) *num_positive = plan->n_pos;
    if (num_negative) *num_negative = plan->n_neg;
    return 0;
}

extern "C" int pgh_probe_plan_destroy(pgh_probe_plan_t plan) {
    if (!plan) return 0;
    if (plan->cls) pool_free(plan->cls);
    if (plan->pos_idx) pool_free(plan->pos_idx);
    delete plan;
    return 0;
}

extern "C" int pgh_probe_auc(pgh_mat_t slab, const double* coeffs_host, int32_t terms, int32_t probes, pgh_probe_plan_t plan,
                             double* auc_host) {
    PGH_CHECK(slab && coeffs_host && plan && auc_host, "pgh_probe_auc: null argument");
    PGH_CHECK(probes >= 1 && probes <= 64 && terms >= 1, "pgh_probe_auc: 1 <= probes <= 64 and terms >= 1 expected");
    if (terms > 64) return declined(PGH_TUNE_DECLINED, kAuc, "more than 64 terms (more than one slab)");
    PGH_CHECK(terms <= slab->b && slab->n == plan->n, "pgh_probe_auc: shape mismatch");
    if (plan->n_pos == 0 || plan->n_neg == 0) return declined(PGH_TUNE_DECLINED, kAuc, "all labels are the same");
    if (plan->n_pos > PGH_TUNE_MAX_POSITIVES) return declined(PGH_TUNE_DECLINED, kAuc, "more positives than the per-probe sort holds");
    for (int64_t j = 0; j < (int64_t)terms * probes; ++j)
        if (!std::isfinite(coeffs_host[j])) return declined(PGH_TUNE_DECLINED, kAuc, "non-finite coefficient");
    Runtime& r = rt();
    const int m = (int)plan->n_pos;
    int padded = 1;
    while (padded < m) padded <<= 1;
    const size_t coeff_bytes = sizeof(double) * (size_t)terms * probes;
    PoolBuf d_c, sorted, totals;
    PGH_TRY(d_c.alloc(coeff_bytes));
    PGH_TRY(sorted.alloc(sizeof(float) * (size_t)probes * m));
    PGH_TRY(totals.alloc(sizeof(unsigned long long) * 64));
    StreamFence fence;                                       // the caller's coefficient array may go away
    PGH_HIP(hipMemcpyAsync(d_c.p, coeffs_host, coeff_bytes, hipMemcpyHostToDevice, r.stream));
    PGH_HIP(hipMemsetAsync(totals.p, 0, sizeof(unsigned long long) * 64, r.stream));
    k_probe_positives<<<probes, kSlabBlock, 0, r.stream>>>(slab->data, slab->b, d_c.as<double>(), terms, probes, plan->pos_idx, m, padded,
                                                       sorted.as<float>());
    const size_t lds_all = coeff_bytes + sizeof(float) * (size_t)probes * m;
    const bool in_lds = lds_all <= PGH_TUNE_LDS_BYTES;
    const size_t lds = in_lds ? lds_all : coeff_bytes;
    const int lpr = lpr_for(probes);
    const int grid = grid_capped(slab->n, kSlabBlock / lpr);
    const int vec_ok = slab->b % 4 == 0 && aligned16(slab->data);
#define PGH_STREAM(LPR)                                                                                                                   \
    do {                                                                                                                                  \
        if (in_lds)                                                                                                                       \
            k_probe_stream<LPR, true><<<grid, kSlabBlock, lds, r.stream>>>(slab->data, slab->n, slab->b, vec_ok, d_c.as<double>(), terms, probes, \
                                                                        plan->cls, sorted.as<float>(), m, totals.as<unsigned long long>()); \
        else                                                                                                                              \
            k_probe_stream<LPR, false><<<grid, kSlabBlock, lds, r.stream>>>(slab->data, slab->n, slab->b, vec_ok, d_c.as<double>(), terms, probes, \
                                                                         plan->cls, sorted.as<float>(), m, totals.as<unsigned long long>()); \
    } while (0)
    switch (lpr) {
        case 16: PGH_STREAM(16); break;
        case 8: PGH_STREAM(8); break;
        case 4: PGH_STREAM(4); break;
        case 2: PGH_STREAM(2); break;
        default: PGH_STREAM(1); break;
    }
#undef PGH_STREAM
    PGH_HIP(hipGetLastError());
    unsigned long long host[64];
    PGH_HIP(hipMemcpyAsync(host, totals.p, sizeof(unsigned long long) * probes, hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(fence.wait());
    const unsigned long long full = 2ull * (unsigned long long)m * (unsigned long long)plan->n_neg;
    for (int q = 0; q < probes; ++q) auc_host[q] = (double)(full - host[q]) / (double)full;
    return 0;
}
