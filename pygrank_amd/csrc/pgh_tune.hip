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
#include "pgh_common.h"
#include "pgh_tune.h"

#include <cmath>

using namespace pgh;

struct pgh_probe_plan_s {
    uint8_t* cls = nullptr;      // [n] 0 excluded, 1 negative, 2 positive
    int32_t* pos_idx = nullptr;  // [n_pos] rows of the positives (any order: their scores are sorted per probe)
    int64_t  n = 0, n_pos = 0, n_neg = 0;
};

namespace {
constexpr int kBlock = 256;
constexpr int kMaxGrid = 2048;   // 256 CUs x 8 workgroups, grid-stride beyond

inline int grid_rows(int64_t rows, int rows_per_block) {
    int64_t g = (rows + rows_per_block - 1) / rows_per_block;
    if (g < 1) g = 1;
    return (int)(g > kMaxGrid ? kMaxGrid : g);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v, int stop) {
    for (int off = 32; off >= stop; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// class byte of every node + the two class counts (counts[0] positives, counts[1] negatives)
__global__ __launch_bounds__(kBlock) void k_plan_classify(const float* __restrict__ known, const float* __restrict__ exclude, int64_t n,
                                                           uint8_t* __restrict__ cls, unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long pos = 0, neg = 0;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const bool out = exclude != nullptr && exclude[i] != 0.f;
        const uint8_t c = out ? 0 : (known[i] != 0.f ? 2 : 1);
        cls[i] = c;
        pos += c == 2;
        neg += c == 1;
    }
    pos = wave_sum_u64(pos, 1);
    neg = wave_sum_u64(neg, 1);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_cnt[0], pos);
        atomicAdd(&s_cnt[1], neg);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x] != 0) atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
}

// rows of the positives, appended in arrival order (the slot counter never passes n_pos: the same predicate counted them)
__global__ __launch_bounds__(kBlock) void k_plan_positives(const uint8_t* __restrict__ cls, int64_t n, int64_t n_pos, int32_t* __restrict__ pos_idx,
                                                            unsigned long long* __restrict__ cursor) {
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        if (cls[i] != 2) continue;
        const unsigned long long slot = atomicAdd(cursor, 1ull);
        if (slot < (unsigned long long)n_pos) pos_idx[slot] = (int32_t)i;
    }
}

// sorted[q][0 .. m): the scores of the positives under probe q, ascending.  m <= PGH_TUNE_MAX_POSITIVES.
__global__ __launch_bounds__(kBlock) void k_probe_positives(const float* __restrict__ slab, int b, const double* __restrict__ coeffs, int terms, int probes,
                                                             const int32_t* __restrict__ pos_idx, int m, int padded /* power of two >= m */,
                                                             float* __restrict__ sorted) {
    __shared__ float s_v[PGH_TUNE_MAX_POSITIVES];
    const int q = blockIdx.x;
    for (int k = threadIdx.x; k < padded; k += kBlock) {
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
    for (int size = 2; size <= padded; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < padded; t += kBlock) {
                const int other = t ^ stride;
                if (other > t) {
                    const float a = s_v[t], c = s_v[other];
                    const bool ascending = (t & size) == 0;
                    if ((a > c) == ascending) {
                        s_v[t] = c;
                        s_v[other] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int k = threadIdx.x; k < m; k += kBlock) sorted[(int64_t)q * m + k] = s_v[k];
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
__global__ __launch_bounds__(kBlock) void k_probe_stream(const float* __restrict__ slab, int64_t n, int b, int vec_ok, const double* __restrict__ coeffs,
                                                          int terms, int probes, const uint8_t* __restrict__ cls,
                                                          const float* __restrict__ sorted, int m, unsigned long long* __restrict__ totals) {
    extern __shared__ double s_dyn[];
    __shared__ unsigned long long s_tot[64];
    double* s_c = s_dyn;                                     // [terms * probes]
    float* s_pos = reinterpret_cast<float*>(s_dyn + terms * probes);   // [probes * m] when IN_LDS
    for (int j = threadIdx.x; j < terms * probes; j += kBlock) s_c[j] = coeffs[j];
    if (IN_LDS)
        for (int j = threadIdx.x; j < probes * m; j += kBlock) s_pos[j] = sorted[j];
    if (threadIdx.x < 64) s_tot[threadIdx.x] = 0;
    __syncthreads();
    constexpr int ROWS = kBlock / LPR;
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

int decline(const std::string& why) {
    set_error("pgh_probe_auc declined: " + why);
    return PGH_TUNE_DECLINED;
}
}  // namespace

PGH_WARM_KERNEL(k_plan_classify)

extern "C" int pgh_probe_plan_create(pgh_vec_t known, pgh_vec_t exclude, pgh_probe_plan_t* out) {
    PGH_CHECK(known && out, "pgh_probe_plan_create: null argument");
    PGH_CHECK(exclude == nullptr || exclude->n == known->n, "pgh_probe_plan_create: known and exclude differ in length");
    PGH_CHECK(known->n < 2147483647LL, "pgh_probe_plan_create: vector too long");
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const int64_t n = known->n;
    pgh_probe_plan_s* plan = new pgh_probe_plan_s();
    plan->n = n;
    unsigned long long* counts = nullptr;                  // positives, negatives, append cursor
    int rc = pool_alloc(sizeof(unsigned long long) * 3, (void**)&counts);
    if (rc == 0) rc = pool_alloc((size_t)(n > 0 ? n : 1), (void**)&plan->cls);
    if (rc != 0) {
        if (counts) pool_free(counts);
        delete plan;
        return rc;
    }
    unsigned long long host[3] = {0, 0, 0};
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(unsigned long long) * 3, r.stream);
    if (e == hipSuccess && n > 0) {
        k_plan_classify<<<grid_rows(n, kBlock * 8), kBlock, 0, r.stream>>>(known->data, exclude ? exclude->data : nullptr, n, plan->cls, counts);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host, counts, sizeof(unsigned long long) * 2, hipMemcpyDeviceToHost, r.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r.stream);
    if (e == hipSuccess) {
        plan->n_pos = (int64_t)host[0];
        plan->n_neg = (int64_t)host[1];
        rc = pool_alloc(sizeof(int32_t) * (size_t)(plan->n_pos > 0 ? plan->n_pos : 1), (void**)&plan->pos_idx);
        if (rc == 0 && plan->n_pos > 0) {
            k_plan_positives<<<grid_rows(n, kBlock * 8), kBlock, 0, r.stream>>>(plan->cls, n, plan->n_pos, plan->pos_idx, counts + 2);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(r.stream);
        }
    }
    pool_free(counts);
    if (e != hipSuccess || rc != 0) {
        pgh_probe_plan_destroy(plan);
        return e != hipSuccess ? fail(std::string("pgh_probe_plan_create: ") + hipGetErrorString(e)) : rc;
    }
    *out = plan;
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
    if (terms > 64) return decline("more than 64 terms (more than one slab)");
    PGH_CHECK(terms <= slab->b && slab->n == plan->n, "pgh_probe_auc: shape mismatch");
    if (plan->n_pos == 0 || plan->n_neg == 0) return decline("all labels are the same");
    if (plan->n_pos > PGH_TUNE_MAX_POSITIVES) return decline("more positives than the per-probe sort holds");
    for (int64_t j = 0; j < (int64_t)terms * probes; ++j)
        if (!std::isfinite(coeffs_host[j])) return decline("non-finite coefficient");
    Runtime& r = rt();
    const int m = (int)plan->n_pos;
    int padded = 1;
    while (padded < m) padded <<= 1;
    const size_t coeff_bytes = sizeof(double) * (size_t)terms * probes;
    double* d_c = nullptr;
    float* sorted = nullptr;
    unsigned long long* totals = nullptr;
    PGH_TRY(pool_alloc(coeff_bytes, (void**)&d_c));
    int rc = pool_alloc(sizeof(float) * (size_t)probes * m, (void**)&sorted);
    if (rc == 0) rc = pool_alloc(sizeof(unsigned long long) * 64, (void**)&totals);
    if (rc != 0) {
        pool_free(d_c);
        if (sorted) pool_free(sorted);
        return rc;
    }
    unsigned long long host[64];
    hipError_t e = hipMemcpyAsync(d_c, coeffs_host, coeff_bytes, hipMemcpyHostToDevice, r.stream);
    if (e == hipSuccess) e = hipMemsetAsync(totals, 0, sizeof(unsigned long long) * 64, r.stream);
    if (e == hipSuccess) {
        k_probe_positives<<<probes, kBlock, 0, r.stream>>>(slab->data, slab->b, d_c, terms, probes, plan->pos_idx, m, padded, sorted);
        const size_t lds_all = coeff_bytes + sizeof(float) * (size_t)probes * m;
        const bool in_lds = lds_all <= PGH_TUNE_LDS_BYTES;
        const size_t lds = in_lds ? lds_all : coeff_bytes;
        const int lpr = probes > 32 ? 16 : (probes > 16 ? 8 : (probes > 8 ? 4 : (probes > 4 ? 2 : 1)));
        const int grid = grid_rows(slab->n, kBlock / lpr);
        const int vec_ok = slab->b % 4 == 0 && (reinterpret_cast<uintptr_t>(slab->data) & 15) == 0;
#define PGH_STREAM(LPR)                                                                                                                   \
    do {                                                                                                                                  \
        if (in_lds)                                                                                                                       \
            k_probe_stream<LPR, true><<<grid, kBlock, lds, r.stream>>>(slab->data, slab->n, slab->b, vec_ok, d_c, terms, probes, plan->cls, \
                                                                        sorted, m, totals);                                               \
        else                                                                                                                              \
            k_probe_stream<LPR, false><<<grid, kBlock, lds, r.stream>>>(slab->data, slab->n, slab->b, vec_ok, d_c, terms, probes, plan->cls, \
                                                                         sorted, m, totals);                                              \
    } while (0)
        switch (lpr) {
            case 16: PGH_STREAM(16); break;
            case 8: PGH_STREAM(8); break;
            case 4: PGH_STREAM(4); break;
            case 2: PGH_STREAM(2); break;
            default: PGH_STREAM(1); break;
        }
#undef PGH_STREAM
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host, totals, sizeof(unsigned long long) * probes, hipMemcpyDeviceToHost, r.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r.stream);  // the caller's coefficient array may go away
    pool_free(d_c);
    pool_free(sorted);
    pool_free(totals);
    if (e != hipSuccess) return fail(std::string("pgh_probe_auc: ") + hipGetErrorString(e));
    const unsigned long long full = 2ull * (unsigned long long)m * (unsigned long long)plan->n_neg;
    for (int q = 0; q < probes; ++q) auc_host[q] = (double)(full - host[q]) / (double)full;
    return 0;
}
