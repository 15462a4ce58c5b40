// include/pgh_link.h: the similarities of a fixed list of node pairs under the [n, b] slab of a batch, their AUC against the pairs'
// labels, and the per-row factors of the similarity.
//
// Reference counterpart: LinkAssessment.evaluate (pygrank/measures/multigroup.py:71-104) -- one Python call of _cos_similarity /
// _dot_similarity (:8-27) per pair, each a loop over the groups' dictionaries, then sklearn's roc_curve + auc on the two lists -- and the
// same similarity inside ClusteringCoefficient (:124-143).
//
// Kernels, all on the engine's stream:
//   k_link_rows<FACTORS>  a workgroup takes tiles of 256 rows; per chunk of up to 32 columns the tile is loaded coalesced into LDS (row
//                         stride odd: the lanes' column reads spread over the banks), then lane r adds the squares of ITS row in column
//                         order into one f64 accumulator that lives across the chunks.  The order of the adds is the contract (it is
//                         Python's); a square of an f32 value is exact in f64, so contracting the multiply-add changes nothing.
//                         FACTORS: the lane ends with t = S[r, last] / sqrt(l2), rounded once to f32, instead of storing l2.
//   k_link_pairs<COS>     lane <-> pair, grid-stride: two gathers of the last column, two of l2, the IEEE quotient, the key (or the
//                         prediction itself for pgh_link_predictions).  A NaN raises a flag (integer atomic).
//   hipcub                one radix sort of (key, label) pairs, one inclusive sum of the negatives in sorted order.
//   k_link_count          lane <-> sorted position of a positive: its tie group by two binary searches in the sorted keys, then
//                         2 * negatives_below + negatives_in_group from the prefix counts; 64-bit integer sums, one integer atomic per
//                         wavefront (integer addition is associative: the result does not depend on the order of arrival).
// No grid shape enters a result: a row is summed by one lane alone, a pair is a function of its two rows, the counts are integers.
#include "pgh_slab.h"
#include "pgh_link.h"

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdint>
#include <limits>

using namespace pgh;

// the quotient is formed from individually rounded f64 operations, as numpy forms it
#pragma clang fp contract(off)

struct pgh_link_plan_s {
    int64_t   n = 0, pairs = 0, positives = 0;
    int32_t*  first = nullptr;       // [pairs]
    int32_t*  second = nullptr;      // [pairs]
    uint8_t*  label = nullptr;       // [pairs] 0 / 1
    // scratch, allocated by the first call that needs it
    double*   l2 = nullptr;          // [n]
    unsigned long long* key_in = nullptr;    // [pairs]
    unsigned long long* key_out = nullptr;   // [pairs]
    uint8_t*  label_out = nullptr;   // [pairs]
    uint32_t* neg_before = nullptr;  // [pairs + 1] negatives among the first i sorted pairs
    void*     temp = nullptr;        // the sort's and the scan's temporary
    size_t    temp_bytes = 0;
    unsigned long long* result = nullptr;    // [2] two_wins, NaN flag
};

namespace {
constexpr int kChunk = 32;           // columns of a row tile in LDS at a time
constexpr int kStrideMax = kChunk + 1;

// FACTORS = false: l2[i] = sum_j (double)S[i, j]^2 in ascending j.  FACTORS = true: out[i] = (float)(S[i, b-1] / sqrt(l2[i])), 0 for l2 = 0.
template <bool FACTORS>
__global__ __launch_bounds__(kSlabBlock) void k_link_rows(const float* __restrict__ S, int64_t n, int b, double* __restrict__ l2, float* __restrict__ out) {
    __shared__ float s_tile[kSlabBlock * kStrideMax];
    const int64_t tiles = (n + kSlabBlock - 1) / kSlabBlock;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * kSlabBlock;
        const int rows = (int)((n - r0) < kSlabBlock ? (n - r0) : kSlabBlock);
        double acc = 0.0;
        float last = 0.f;
        for (int c0 = 0; c0 < b; c0 += kChunk) {
            const int w = (b - c0) < kChunk ? (b - c0) : kChunk;
            const int stride = w | 1;
            __syncthreads();                                   // the previous chunk has been read
            for (int t = threadIdx.x; t < rows * w; t += kSlabBlock) {
                const int r = t / w, c = t - r * w;
                s_tile[r * stride + c] = S[(r0 + r) * (int64_t)b + c0 + c];
            }
            __syncthreads();
            if ((int)threadIdx.x < rows) {
                const float* row = s_tile + threadIdx.x * stride;
                for (int c = 0; c < w; ++c) {
                    const double x = (double)row[c];
                    acc += x * x;
                }
                last = row[w - 1];
            }
        }
        if ((int)threadIdx.x < rows) {
            if (FACTORS) {
                const double den = sqrt(acc);
                out[r0 + threadIdx.x] = (float)(den == 0.0 ? 0.0 : (double)last / den);
            } else {
                l2[r0 + threadIdx.x] = acc;
            }
        }
    }
}

__global__ __launch_bounds__(kSlabBlock) void k_link_last_column(const float* __restrict__ S, int64_t n, int b, float* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSlabBlock) out[i] = S[i * b + (b - 1)];
}

// ascending unsigned order of the keys = ascending order of the doubles; both zeros share a key
__device__ __forceinline__ unsigned long long order_key(double x) {
    if (x == 0.0) x = 0.0;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
    return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
}

// pair k = first_pair + i, i < count: keys[i] (when given) and preds[i] (when given)
template <bool COS>
__global__ __launch_bounds__(kSlabBlock) void k_link_pairs(const float* __restrict__ S, int b, const double* __restrict__ l2, const int32_t* __restrict__ first,
                                                            const int32_t* __restrict__ second, int64_t first_pair, int64_t count,
                                                            unsigned long long* __restrict__ keys, double* __restrict__ preds,
                                                            unsigned long long* __restrict__ nan_flag) {
    bool nan = false;
    for (int64_t i = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kSlabBlock) {
        const int64_t v = first[first_pair + i], u = second[first_pair + i];
        const double sv = (double)S[v * b + (b - 1)], su = (double)S[u * b + (b - 1)];
        double pred = su * sv;
        if (COS) {
            const double den = sqrt(l2[u] * l2[v]);
            pred = den == 0.0 ? 0.0 : pred / den;
        }
        nan |= pred != pred;
        if (keys != nullptr) keys[i] = order_key(pred);
        if (preds != nullptr) preds[i] = pred;
    }
    if (nan_flag != nullptr && nan) atomicOr(nan_flag, 1ull);
}

struct IsNegative {
    __host__ __device__ uint32_t operator()(const uint8_t& label) const { return label == 0 ? 1u : 0u; }
};

// result[0] += sum over the positives at sorted positions i of 2 * negatives below key[i] + negatives at key[i]
__global__ __launch_bounds__(kSlabBlock) void k_link_count(const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ labels,
                                                            const uint32_t* __restrict__ neg_before, int64_t count, unsigned long long* __restrict__ result) {
    unsigned long long wins = 0;
    for (int64_t i = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kSlabBlock) {
        if (labels[i] == 0) continue;
        const unsigned long long key = keys[i];
        int64_t lo = 0, hi = i;                   // first position whose key is not below `key`
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        const int64_t begin = lo;
        lo = i + 1, hi = count;                   // first position whose key is above `key`
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] <= key) lo = mid + 1; else hi = mid;
        }
        const unsigned long long below = neg_before[begin], tied = neg_before[lo] - neg_before[begin];
        wins += 2ull * below + tied;
    }
    wins = wave_sum_u64(wins, 1);
    if ((threadIdx.x & 63) == 0 && wins) atomicAdd(&result[0], wins);
}

// pool_alloc that turns a failure into a decline
int scratch(const char* who, size_t bytes, void** p) {
    if (*p != nullptr) return 0;
    if (pool_alloc(bytes > 0 ? bytes : 1, p) != 0) {
        *p = nullptr;
        return declined(PGH_LINK_DECLINED, who, "the plan's scratch does not fit in device memory");
    }
    return 0;
}

int check_call(const char* who, pgh_mat_t scores, pgh_link_plan_t plan, int32_t similarity) {
    PGH_CHECK(scores && plan, std::string(who) + ": null argument");
    PGH_CHECK(similarity == PGH_LINK_COS || similarity == PGH_LINK_DOT, std::string(who) + ": unknown similarity");
    PGH_CHECK(scores->b >= 1, std::string(who) + ": a slab needs a column");
    PGH_CHECK(scores->n == plan->n, std::string(who) + ": the slab holds " + std::to_string(scores->n) + " rows, the plan " + std::to_string(plan->n));
    return 0;
}

int row_sums(const char* who, pgh_mat_t scores, pgh_link_plan_t plan) {
    PGH_TRY(scratch(who, sizeof(double) * (size_t)plan->n, (void**)&plan->l2));
    k_link_rows<false><<<grid_capped(plan->n, kSlabBlock), kSlabBlock, 0, rt().stream>>>(scores->data, plan->n, scores->b, plan->l2, nullptr);
    PGH_HIP(hipGetLastError());
    return 0;
}
}  // namespace

PGH_WARM_KERNEL(k_link_last_column)

extern "C" int pgh_link_plan_destroy(pgh_link_plan_t plan) {
    if (plan == nullptr) return 0;
    for (void* p : {(void*)plan->first, (void*)plan->second, (void*)plan->label, (void*)plan->l2, (void*)plan->key_in, (void*)plan->key_out,
                    (void*)plan->label_out, (void*)plan->neg_before, plan->temp, (void*)plan->result})
        if (p) pool_free(p);
    delete plan;
    return 0;
}

extern "C" int pgh_link_plan_create(int64_t n, int64_t num_pairs, const int32_t* first_host, const int32_t* second_host, const uint8_t* label_host,
                                    pgh_link_plan_t* out) {
    PGH_CHECK(out, "pgh_link_plan_create: null argument");
    PGH_CHECK(n >= 1 && n < 2147483647LL, "pgh_link_plan_create: 1 <= n < 2^31 - 1");
    PGH_CHECK(num_pairs >= 0, "pgh_link_plan_create: a negative number of pairs");
    PGH_CHECK(num_pairs <= (int64_t)PGH_LINK_MAX_PAIRS,
              "pgh_link_plan_create: " + std::to_string(num_pairs) + " pairs exceed PGH_LINK_MAX_PAIRS = 2^27; take smaller samples");
    PGH_CHECK(num_pairs == 0 || (first_host && second_host && label_host), "pgh_link_plan_create: null argument");
    int64_t positives = 0;
    for (int64_t k = 0; k < num_pairs; ++k) {
        PGH_CHECK(first_host[k] >= 0 && first_host[k] < n && second_host[k] >= 0 && second_host[k] < n,
                  "pgh_link_plan_create: pair " + std::to_string(k) + " names a node outside [0, n)");
        positives += label_host[k] != 0;
    }
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    pgh_link_plan_s* plan = new pgh_link_plan_s();
    plan->n = n, plan->pairs = num_pairs, plan->positives = positives;
    if (num_pairs > 0) {
        const size_t count = (size_t)num_pairs;
        int rc = pool_alloc(sizeof(int32_t) * count, (void**)&plan->first);
        if (rc == 0) rc = pool_alloc(sizeof(int32_t) * count, (void**)&plan->second);
        if (rc == 0) rc = pool_alloc(count, (void**)&plan->label);
        hipError_t e = hipSuccess;
        if (rc == 0) {
            // labels travel as 0 / 1
            uint8_t* norm = new uint8_t[count];
            for (size_t k = 0; k < count; ++k) norm[k] = label_host[k] != 0 ? 1 : 0;
            e = hipMemcpyAsync(plan->first, first_host, sizeof(int32_t) * count, hipMemcpyHostToDevice, r.stream);
            if (e == hipSuccess) e = hipMemcpyAsync(plan->second, second_host, sizeof(int32_t) * count, hipMemcpyHostToDevice, r.stream);
            if (e == hipSuccess) e = hipMemcpyAsync(plan->label, norm, count, hipMemcpyHostToDevice, r.stream);
            const hipError_t s = hipStreamSynchronize(r.stream);      // the caller's arrays may go away
            if (e == hipSuccess) e = s;
            delete[] norm;
        }
        if (rc != 0 || e != hipSuccess) {
            pgh_link_plan_destroy(plan);
            return e != hipSuccess ? fail(std::string("pgh_link_plan_create: ") + hipGetErrorString(e)) : rc;
        }
    }
    *out = plan;
    return 0;
}

extern "C" int pgh_link_plan_info(pgh_link_plan_t plan, int64_t* n, int64_t* num_pairs, int64_t* num_positive) {
    PGH_CHECK(plan, "pgh_link_plan_info: null plan");
    if (n) *n = plan->n;
    if (num_pairs) *num_pairs = plan->pairs;
    if (num_positive) *num_positive = plan->positives;
    return 0;
}

extern "C" int pgh_link_auc(pgh_mat_t scores, pgh_link_plan_t plan, int32_t similarity, double* auc, int64_t* num_positive, int64_t* num_negative) {
    static const char* who = "pgh_link_auc";
    PGH_CHECK(auc && num_positive && num_negative, "pgh_link_auc: null argument");
    PGH_TRY(check_call(who, scores, plan, similarity));
    const int64_t count = plan->pairs, P = plan->positives, N = count - P;
    if (P == 0 || N == 0) {
        *auc = std::numeric_limits<double>::quiet_NaN();
        *num_positive = P, *num_negative = N;
        return 0;
    }
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const bool cos = similarity == PGH_LINK_COS;
    // scratch first: a decline leaves nothing written and nothing enqueued
    if (cos) PGH_TRY(scratch(who, sizeof(double) * (size_t)plan->n, (void**)&plan->l2));
    PGH_TRY(scratch(who, sizeof(unsigned long long) * (size_t)count, (void**)&plan->key_in));
    PGH_TRY(scratch(who, sizeof(unsigned long long) * (size_t)count, (void**)&plan->key_out));
    PGH_TRY(scratch(who, (size_t)count, (void**)&plan->label_out));
    PGH_TRY(scratch(who, sizeof(uint32_t) * ((size_t)count + 1), (void**)&plan->neg_before));
    PGH_TRY(scratch(who, sizeof(unsigned long long) * 2, (void**)&plan->result));
    hipcub::TransformInputIterator<uint32_t, IsNegative, const uint8_t*> negatives(plan->label_out, IsNegative());
    if (plan->temp == nullptr) {
        size_t sort_bytes = 0, scan_bytes = 0;
        PGH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, plan->key_in, plan->key_out, plan->label, plan->label_out, (int)count, 0, 64,
                                                   r.stream));
        PGH_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, negatives, plan->neg_before + 1, (int)count, r.stream));
        plan->temp_bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
        PGH_TRY(scratch(who, plan->temp_bytes, &plan->temp));
    }
    if (cos) PGH_TRY(row_sums(who, scores, plan));
    PGH_HIP(hipMemsetAsync(plan->result, 0, sizeof(unsigned long long) * 2, r.stream));
    PGH_HIP(hipMemsetAsync(plan->neg_before, 0, sizeof(uint32_t), r.stream));
    const int grid = grid_capped(count, kSlabBlock);
    if (cos)
        k_link_pairs<true><<<grid, kSlabBlock, 0, r.stream>>>(scores->data, scores->b, plan->l2, plan->first, plan->second, 0, count, plan->key_in, nullptr,
                                                          plan->result + 1);
    else
        k_link_pairs<false><<<grid, kSlabBlock, 0, r.stream>>>(scores->data, scores->b, nullptr, plan->first, plan->second, 0, count, plan->key_in, nullptr,
                                                           plan->result + 1);
    PGH_HIP(hipGetLastError());
    size_t bytes = plan->temp_bytes;
    PGH_HIP(hipcub::DeviceRadixSort::SortPairs(plan->temp, bytes, plan->key_in, plan->key_out, plan->label, plan->label_out, (int)count, 0, 64, r.stream));
    bytes = plan->temp_bytes;
    PGH_HIP(hipcub::DeviceScan::InclusiveSum(plan->temp, bytes, negatives, plan->neg_before + 1, (int)count, r.stream));
    k_link_count<<<grid, kSlabBlock, 0, r.stream>>>(plan->key_out, plan->label_out, plan->neg_before, count, plan->result);
    PGH_HIP(hipGetLastError());
    unsigned long long host[2] = {0, 0};
    PGH_HIP(hipMemcpyAsync(host, plan->result, sizeof(host), hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(hipStreamSynchronize(r.stream));
    *auc = host[1] != 0 ? std::numeric_limits<double>::quiet_NaN() : (double)host[0] / (2.0 * (double)P * (double)N);
    *num_positive = P, *num_negative = N;
    return 0;
}

extern "C" int pgh_link_predictions(pgh_mat_t scores, pgh_link_plan_t plan, int32_t similarity, int64_t first, int64_t count, double* out_host) {
    static const char* who = "pgh_link_predictions";
    PGH_TRY(check_call(who, scores, plan, similarity));
    PGH_CHECK(first >= 0 && count >= 0 && first <= plan->pairs && count <= plan->pairs - first, "pgh_link_predictions: the range leaves the plan's pairs");
    if (count == 0) return 0;
    PGH_CHECK(out_host, "pgh_link_predictions: null argument");
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const bool cos = similarity == PGH_LINK_COS;
    if (cos) PGH_TRY(scratch(who, sizeof(double) * (size_t)plan->n, (void**)&plan->l2));
    PoolBuf preds;
    if (preds.alloc(sizeof(double) * (size_t)count) != 0) return declined(PGH_LINK_DECLINED, who, "the predictions do not fit in device memory");
    if (cos) PGH_TRY(row_sums(who, scores, plan));
    const int grid = grid_capped(count, kSlabBlock);
    if (cos)
        k_link_pairs<true><<<grid, kSlabBlock, 0, r.stream>>>(scores->data, scores->b, plan->l2, plan->first, plan->second, first, count, nullptr,
                                                          preds.as<double>(), nullptr);
    else
        k_link_pairs<false><<<grid, kSlabBlock, 0, r.stream>>>(scores->data, scores->b, nullptr, plan->first, plan->second, first, count, nullptr,
                                                           preds.as<double>(), nullptr);
    PGH_HIP(hipGetLastError());
    PGH_HIP(hipMemcpyAsync(out_host, preds.p, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(hipStreamSynchronize(r.stream));
    return 0;
}

extern "C" int pgh_link_factors(pgh_mat_t scores, int32_t similarity, pgh_vec_t out) {
    PGH_CHECK(scores && out, "pgh_link_factors: null argument");
    PGH_CHECK(similarity == PGH_LINK_COS || similarity == PGH_LINK_DOT, "pgh_link_factors: unknown similarity");
    PGH_CHECK(scores->b >= 1, "pgh_link_factors: a slab needs a column");
    PGH_CHECK(out->n == scores->n, "pgh_link_factors: out and the slab differ in length");
    const int64_t n = scores->n;
    if (n == 0) return 0;
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    if (similarity == PGH_LINK_COS)
        k_link_rows<true><<<grid_capped(n, kSlabBlock), kSlabBlock, 0, r.stream>>>(scores->data, n, scores->b, nullptr, out->data);
    else
        k_link_last_column<<<grid_capped(n, kSlabBlock), kSlabBlock, 0, r.stream>>>(scores->data, n, scores->b, out->data);
    PGH_HIP(hipGetLastError());
    return 0;
}
