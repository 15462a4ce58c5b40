// include/pgh_rank.h: the DCG and Spearman's rho of up to 64 score columns against shared known scores.
//
// Reference counterparts: pygrank/measures/supervised.py:68-90 (NDCG: one host sort of n scores per vector) and :274-279
// (SpearmanCorrelation: scipy.stats.spearmanr on the host).
//
// The plan (pgh_rank_plan_create), once per (known scores, exclude) pair:
//   k_classify_labels   a class byte per row (0 excluded, 1 kept, 2 kept and relevant), the two counts, the negative flag (pgh_slab.h)
//   hipcub select       the kept rows and the relevant rows in ascending row order; k_rank_gather takes their known scores
//   lazily              the kept known scores in descending order (hipcub), d_known by two binary searches per kept row, sum d_known^2
// pgh_ndcg, streaming route, all on the engine's stream:
//   k_ndcg_relevant     one workgroup per column: the (score, relevant index) pairs of the relevant rows, sorted in LDS (bitonic) into
//                       the column's order: score descending, row ascending
//   k_ndcg_stream       every kept element of the slab once, consecutive lanes on consecutive floats (a thread keeps ONE column: the
//                       stride is a multiple of b); one binary search on the composite (score, row) key gives the first relevant
//                       entry t the element precedes, and bin (column, t) counts it: an integer atomic, in LDS while the bins and the entries'
//                       scores of all columns fit there, else in global memory
//   k_ndcg_finish       one workgroup per column: thread t owns a fixed run of entries, a scan over the runs' sums gives every
//                       pos_v = inclusive prefix of the bins, and the terms are summed in f64 in that fixed order
// Sorted route and Spearman, per column: k_rank_keys (canonical keys of the kept rows from the strided column), hipcub radix sort of
// (key, kept position) pairs, k_dcg_parts / k_rho_parts (kRankParts workgroups whatever the device, element i always with the same lane)
// and k_rank_fold.
#include "pgh_slab.h"
#include "pgh_rank.h"

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdint>
#include <memory>

using namespace pgh;

struct pgh_rank_plan_s {
    int64_t  n = 0, n_kept = 0, n_rel = 0;
    int32_t  has_negative = 0;
    uint8_t* cls = nullptr;          // [n] 0 excluded, 1 kept, 2 kept and relevant
    int32_t* kept_row = nullptr;     // [n_kept] ascending
    float*   kept_known = nullptr;   // [n_kept]
    int32_t* rel_row = nullptr;      // [n_rel] ascending
    float*   rel_known = nullptr;    // [n_rel]
    float*   known_desc = nullptr;   // [n_kept] lazily: kept known scores, descending
    int32_t* d_known = nullptr;      // [n_kept] lazily: 2 midrank - (n_kept + 1), ranks from the top
    double   sum_dk2 = 0.0;          // sum d_known^2
};

namespace {
constexpr int kStreamBlock = 512;
constexpr int kRankParts = 256;          // fixed row parts of the f64 sums: the grid of k_dcg_parts / k_rho_parts whatever the device

// -0.0 and +0.0 are one score: a radix key would tell them apart
__device__ __forceinline__ float canonical(float s) { return s == 0.f ? 0.f : s; }

// (a_s, a_r) comes before (b_s, b_r) in a column's order: score descending, row ascending
__device__ __forceinline__ bool before(float a_s, int32_t a_r, float b_s, int32_t b_r) { return a_s > b_s || (a_s == b_s && a_r < b_r); }

struct ClassAtLeast {
    const uint8_t* cls;
    uint8_t least;
    __host__ __device__ bool operator()(const int32_t& i) const { return cls[i] >= least; }
};

__global__ __launch_bounds__(kSlabBlock) void k_rank_gather(const float* __restrict__ src, const int32_t* __restrict__ rows, int64_t count, float* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kSlabBlock) out[i] = canonical(src[rows[i]]);
}

__global__ __launch_bounds__(kSlabBlock) void k_rank_iota(int32_t* __restrict__ p, int64_t count) {
    for (int64_t i = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kSlabBlock) p[i] = (int32_t)i;
}

// keys[p] = the canonical score of kept row p in column `col`; a NaN raises the column's flag
__global__ __launch_bounds__(kSlabBlock) void k_rank_keys(const float* __restrict__ S, int b, int col, const int32_t* __restrict__ kept_row, int64_t count,
                                                           float* __restrict__ keys, int* __restrict__ nan_flag) {
    bool nan = false;
    for (int64_t p = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; p < count; p += (int64_t)gridDim.x * kSlabBlock) {
        const float s = S[(int64_t)kept_row[p] * b + col];
        nan |= s != s;
        keys[p] = canonical(s);
    }
    if (nan) atomicOr(nan_flag, 1);
}

// in a DESCENDING run K[0 .. count): the number of elements above v (STRICT) or not below v (!STRICT)
template <bool STRICT>
__device__ __forceinline__ int64_t count_above(const float* __restrict__ K, int64_t count, float v) {
    int64_t lo = 0, hi = count;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const float x = K[mid];
        if (STRICT ? (x > v) : (x >= v)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// d[p] = lo + hi - count for the value vals[p] among the descending run K (K is a permutation of vals)
__global__ __launch_bounds__(kSlabBlock) void k_rank_dknown(const float* __restrict__ vals, const float* __restrict__ K, int64_t count, int32_t* __restrict__ d) {
    for (int64_t p = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; p < count; p += (int64_t)gridDim.x * kSlabBlock) {
        const float v = vals[p];
        d[p] = (int32_t)(count_above<true>(K, count, v) + count_above<false>(K, count, v) - count);
    }
}

// ---- f64 sums over fixed parts: element i belongs to lane (i % (kRankParts * kSlabBlock)) of the kRankParts workgroups, whatever the device
__device__ __forceinline__ void part_store(double a, double c, double* __restrict__ partial /* [kRankParts][2] */) {
    __shared__ double s_red[4];
    a = block_reduce_256<0>(a, s_red);
    c = block_reduce_256<0>(c, s_red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = a;
        partial[2 * blockIdx.x + 1] = c;
    }
}

// sum over i < count of vals[order ? order[i] : i] / log2(i + 2)
__global__ __launch_bounds__(kSlabBlock) void k_dcg_parts(const float* __restrict__ vals, const int32_t* __restrict__ order, int64_t count, double* __restrict__ partial) {
    double acc = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; i < count; i += (int64_t)kRankParts * kSlabBlock) {
        const float v = vals[order != nullptr ? order[i] : i];
        acc += (double)v / log2((double)i + 2.0);
    }
    part_store(acc, 0.0, partial);
}

// K: a column's keys in descending order, payload: their kept positions; sums d_s d_k and d_s^2.  payload == nullptr: sums d^2 of `dk` alone
__global__ __launch_bounds__(kSlabBlock) void k_rho_parts(const float* __restrict__ K, const int32_t* __restrict__ payload, const int32_t* __restrict__ dk, int64_t count,
                                                           double* __restrict__ partial) {
    double sk = 0.0, ss = 0.0;
    for (int64_t p = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; p < count; p += (int64_t)kRankParts * kSlabBlock) {
        if (payload == nullptr) {
            const double d = (double)dk[p];
            ss += d * d;
        } else {
            const float v = K[p];
            const double ds = (double)(count_above<true>(K, count, v) + count_above<false>(K, count, v) - count);
            sk += ds * (double)dk[payload[p]];
            ss += ds * ds;
        }
    }
    part_store(sk, ss, partial);
}

// out[0], out[1] = the parts' two sums, in part order (one workgroup, thread t holds part t)
static_assert(kRankParts == 256, "k_rank_fold is one block_reduce_256");
__global__ __launch_bounds__(kRankParts) void k_rank_fold(const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ double s_red[4];
    const double a = block_reduce_256<0>(partial[2 * threadIdx.x], s_red);
    const double c = block_reduce_256<0>(partial[2 * threadIdx.x + 1], s_red);
    if (threadIdx.x == 0) {
        out[0] = a;
        out[1] = c;
    }
}

// ---- the streaming route
// Column j = blockIdx.x: the m relevant rows' (canonical score, relevant index) pairs sorted into the column's order; written as
// skey / srow / sknown [j][0 .. m).  m <= PGH_RANK_MAX_RELEVANT, padded = a power of two >= m; the pads sort last.
__global__ __launch_bounds__(kSlabBlock) void k_ndcg_relevant(const float* __restrict__ S, int b, const int32_t* __restrict__ rel_row, const float* __restrict__ rel_known,
                                                               int m, int padded, float* __restrict__ skey, int32_t* __restrict__ srow, float* __restrict__ sknown) {
    __shared__ float s_v[PGH_RANK_MAX_RELEVANT];
    __shared__ int32_t s_r[PGH_RANK_MAX_RELEVANT];
    const int j = blockIdx.x;
    for (int e = threadIdx.x; e < padded; e += kSlabBlock) {
        s_v[e] = e < m ? canonical(S[(int64_t)rel_row[e] * b + j]) : -INFINITY;
        s_r[e] = e < m ? e : 0x7fffffff;
    }
    __syncthreads();
    bitonic_sort_lds<kSlabBlock>(
        padded, [&](int i, int k) { return before(s_v[i], s_r[i], s_v[k], s_r[k]); },
        [&](int i, int k) {
            const float v = s_v[i];
            const int32_t r = s_r[i];
            s_v[i] = s_v[k], s_r[i] = s_r[k];
            s_v[k] = v, s_r[k] = r;
        });
    for (int e = threadIdx.x; e < m; e += kSlabBlock) {
        const int32_t r = s_r[e];
        const bool real = r >= 0 && r < m;               // a NaN score leaves the network's output unordered, never out of range
        skey[(int64_t)j * m + e] = s_v[e];
        srow[(int64_t)j * m + e] = real ? rel_row[r] : 0x7fffffff;
        sknown[(int64_t)j * m + e] = real ? rel_known[r] : 0.f;
    }
}

// bins[j][t] += 1 for every kept element (i, j) whose first preceded entry of column j is t < m (an element that precedes no relevant
// entry changes no position).  IN_LDS: bins and entries of all columns are in LDS, the bins are added to global memory at the end.
template <bool IN_LDS>
__global__ __launch_bounds__(kStreamBlock) void k_ndcg_stream(const float* __restrict__ S, int64_t n, int b, const uint8_t* __restrict__ cls,
                                                               const float* __restrict__ skey, const int32_t* __restrict__ srow, int m,
                                                               unsigned int* __restrict__ bins, int* __restrict__ nan_flags) {
    extern __shared__ unsigned int s_dyn[];
    unsigned int* s_bins = s_dyn;                                        // [b * m]
    float* s_key = reinterpret_cast<float*>(s_dyn + (IN_LDS ? b * m : 0));   // [b * m]; the entries' rows stay in global memory: a
    const int cells = b * m;                                             // row is read only where two scores tie
    if (IN_LDS) {
        for (int c = threadIdx.x; c < cells; c += kStreamBlock) {
            s_bins[c] = 0;
            s_key[c] = skey[c];
        }
        __syncthreads();
    }
    const int64_t total = n * b;
    const int64_t threads = (int64_t)gridDim.x * kStreamBlock;
    const int64_t stride = threads / b * b;                              // a multiple of b: a thread keeps its column
    const int64_t v = blockIdx.x * (int64_t)kStreamBlock + threadIdx.x;
    if (v < stride) {
        int64_t row = v / b;
        const int col = (int)(v - row * b);
        const int64_t row_step = stride / b;
        const float* __restrict__ key = (IN_LDS ? s_key : skey) + (int64_t)col * m;
        const int32_t* __restrict__ rws = srow + (int64_t)col * m;
        unsigned int* cnt = (IN_LDS ? s_bins : bins) + (int64_t)col * m;
        const float last_key = key[m - 1];
        const int32_t last_row = rws[m - 1];
        bool nan = false;
        for (int64_t e = v; e < total; e += stride, row += row_step) {
            if (cls[row] == 0) continue;
            float s = S[e];
            if (s != s) {
                nan = true;
                continue;
            }
            s = canonical(s);
            const int32_t i = (int32_t)row;
            if (!before(s, i, last_key, last_row)) continue;             // precedes no relevant entry
            int lo = 0, hi = m - 1;                                      // entry m - 1 is preceded: the answer is in [0, m - 1]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (before(s, i, key[mid], rws[mid])) hi = mid; else lo = mid + 1;
            }
            atomicAdd(&cnt[lo], 1u);
        }
        if (nan) atomicOr(&nan_flags[col], 1);
    }
    if (IN_LDS) {
        __syncthreads();
        for (int c = threadIdx.x; c < cells; c += kStreamBlock)
            if (s_bins[c] != 0) atomicAdd(&bins[c], s_bins[c]);
    }
}

// Column j = blockIdx.x: pos of entry e = bins[j][0] + .. + bins[j][e]; dcg[j] = sum over the entries with pos < k of known / log2(pos + 2).
// Thread t owns the entries [t * run, t * run + run): a fixed order whatever the launch.
__global__ __launch_bounds__(kSlabBlock) void k_ndcg_finish(const unsigned int* __restrict__ bins, const float* __restrict__ sknown, int m, int64_t k,
                                                             double* __restrict__ dcg) {
    __shared__ unsigned long long s_sum[kSlabBlock];
    __shared__ double s_w[kSlabBlock / 64];
    const int j = blockIdx.x;
    const int run = (m + kSlabBlock - 1) / kSlabBlock;
    const int first = threadIdx.x * run;
    const int stop = first + run < m ? first + run : m;
    const unsigned int* __restrict__ cnt = bins + (int64_t)j * m;
    unsigned long long mine = 0;
    for (int e = first; e < stop; ++e) mine += cnt[e];
    s_sum[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {                                              // exclusive scan of 256 sums
        unsigned long long run_sum = 0;
        for (int t = 0; t < kSlabBlock; ++t) {
            const unsigned long long x = s_sum[t];
            s_sum[t] = run_sum;
            run_sum += x;
        }
    }
    __syncthreads();
    unsigned long long pos = s_sum[threadIdx.x];
    double acc = 0.0;
    for (int e = first; e < stop; ++e) {
        pos += cnt[e];
        if ((long long)pos < k) acc += (double)sknown[(int64_t)j * m + e] / log2((double)pos + 2.0);
    }
    acc = block_reduce_256<0>(acc, s_w);
    if (threadIdx.x == 0) dcg[j] = acc;
}

// keys_in -> (keys_out, order) descending and stable: equal keys keep their kept positions ascending
int sort_pairs_desc(const float* keys_in, float* keys_out, const int32_t* iota, int32_t* order, int64_t count) {
    Runtime& r = rt();
    size_t temp_bytes = 0;
    PGH_HIP(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, temp_bytes, keys_in, keys_out, iota, order, (int)count, 0, 32, r.stream));
    PoolBuf temp;
    PGH_TRY(temp.alloc(temp_bytes));
    PGH_HIP(hipcub::DeviceRadixSort::SortPairsDescending(temp.p, temp_bytes, keys_in, keys_out, iota, order, (int)count, 0, 32, r.stream));
    return 0;
}

// the kept known scores in descending order
int ensure_known_desc(pgh_rank_plan_s* plan) {
    if (plan->known_desc != nullptr || plan->n_kept == 0) return 0;
    Runtime& r = rt();
    PoolBuf out, temp;
    PGH_TRY(out.alloc(sizeof(float) * (size_t)plan->n_kept));
    size_t temp_bytes = 0;
    PGH_HIP(hipcub::DeviceRadixSort::SortKeysDescending(nullptr, temp_bytes, plan->kept_known, out.as<float>(), (int)plan->n_kept, 0, 32, r.stream));
    PGH_TRY(temp.alloc(temp_bytes));
    PGH_HIP(hipcub::DeviceRadixSort::SortKeysDescending(temp.p, temp_bytes, plan->kept_known, out.as<float>(), (int)plan->n_kept, 0, 32, r.stream));
    plan->known_desc = out.release<float>();
    return 0;
}

// partial (kRankParts x 2 doubles) folded into two host doubles
int fold_to_host(double* partial, double* folded, double* host2) {
    Runtime& r = rt();
    k_rank_fold<<<1, kRankParts, 0, r.stream>>>(partial, folded);
    PGH_HIP(hipGetLastError());
    PGH_HIP(hipMemcpyAsync(host2, folded, sizeof(double) * 2, hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(hipStreamSynchronize(r.stream));
    return 0;
}

int ensure_d_known(pgh_rank_plan_s* plan) {
    if (plan->d_known != nullptr || plan->n_kept == 0) return 0;
    PGH_TRY(ensure_known_desc(plan));
    Runtime& r = rt();
    const int64_t count = plan->n_kept;
    PoolBuf d, partial, folded;
    PGH_TRY(d.alloc(sizeof(int32_t) * (size_t)count));
    PGH_TRY(partial.alloc(sizeof(double) * 2 * kRankParts));
    PGH_TRY(folded.alloc(sizeof(double) * 2));
    double host2[2] = {0.0, 0.0};
    k_rank_dknown<<<grid_capped(count, kSlabBlock), kSlabBlock, 0, r.stream>>>(plan->kept_known, plan->known_desc, count, d.as<int32_t>());
    k_rho_parts<<<kRankParts, kSlabBlock, 0, r.stream>>>(nullptr, nullptr, d.as<int32_t>(), count, partial.as<double>());
    PGH_TRY(fold_to_host(partial.as<double>(), folded.as<double>(), host2));
    plan->d_known = d.release<int32_t>();
    plan->sum_dk2 = host2[1];
    return 0;
}

int check_slab(const char* entry, pgh_mat_t scores, pgh_rank_plan_t plan) {
    PGH_CHECK(scores && plan, std::string(entry) + ": null argument");
    PGH_CHECK(scores->b >= 1, std::string(entry) + ": at least one column expected");
    PGH_CHECK(scores->n == plan->n, std::string(entry) + ": the slab's rows differ from the plan's");
    return 0;
}

int ndcg_streaming(pgh_mat_t scores, pgh_rank_plan_s* plan, int64_t k, double* dcg_host) {
    Runtime& r = rt();
    const int b = scores->b, m = (int)plan->n_rel;
    const int64_t n = scores->n;
    int padded = 1;
    while (padded < m) padded <<= 1;
    const size_t cells = (size_t)b * m;
    PoolBuf skey, srow, sknown, bins, flags, dcg;
    PGH_TRY(skey.alloc(sizeof(float) * cells));
    PGH_TRY(srow.alloc(sizeof(int32_t) * cells));
    PGH_TRY(sknown.alloc(sizeof(float) * cells));
    PGH_TRY(bins.alloc(sizeof(unsigned int) * cells));
    PGH_TRY(flags.alloc(sizeof(int) * kSlabMaxCols));
    PGH_TRY(dcg.alloc(sizeof(double) * kSlabMaxCols));
    PGH_HIP(hipMemsetAsync(bins.p, 0, sizeof(unsigned int) * cells, r.stream));
    PGH_HIP(hipMemsetAsync(flags.p, 0, sizeof(int) * kSlabMaxCols, r.stream));
    k_ndcg_relevant<<<b, kSlabBlock, 0, r.stream>>>(scores->data, b, plan->rel_row, plan->rel_known, m, padded, skey.as<float>(), srow.as<int32_t>(),
                                                 sknown.as<float>());
    const size_t lds_all = 8 * cells;
    const bool in_lds = lds_all <= PGH_RANK_LDS_BYTES;
    int grid = grid_capped(n * b, kStreamBlock);
    const int cap = r.num_cus * (in_lds ? 2 : 4);
    if (grid > cap) grid = cap;
    if (in_lds)
        k_ndcg_stream<true><<<grid, kStreamBlock, lds_all, r.stream>>>(scores->data, n, b, plan->cls, skey.as<float>(), srow.as<int32_t>(), m,
                                                                        bins.as<unsigned int>(), flags.as<int>());
    else
        k_ndcg_stream<false><<<grid, kStreamBlock, 0, r.stream>>>(scores->data, n, b, plan->cls, skey.as<float>(), srow.as<int32_t>(), m,
                                                                   bins.as<unsigned int>(), flags.as<int>());
    k_ndcg_finish<<<b, kSlabBlock, 0, r.stream>>>(bins.as<unsigned int>(), sknown.as<float>(), m, k, dcg.as<double>());
    PGH_HIP(hipGetLastError());
    int host_flags[kSlabMaxCols];
    double host_dcg[kSlabMaxCols];
    PGH_HIP(hipMemcpyAsync(host_flags, flags.p, sizeof(int) * b, hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(hipMemcpyAsync(host_dcg, dcg.p, sizeof(double) * b, hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(hipStreamSynchronize(r.stream));
    for (int j = 0; j < b; ++j) dcg_host[j] = host_flags[j] != 0 ? (double)NAN : host_dcg[j];
    return 0;
}

// what the sorted route and Spearman share: per column the canonical keys of the kept rows, sorted descending with their kept positions
struct ColumnSorter {
    PoolBuf keys, sorted, iota, order, partial, folded, flag;
    int64_t count = 0;
    int prepare(int64_t kept) {
        count = kept;
        PGH_TRY(keys.alloc(sizeof(float) * (size_t)kept));
        PGH_TRY(sorted.alloc(sizeof(float) * (size_t)kept));
        PGH_TRY(iota.alloc(sizeof(int32_t) * (size_t)kept));
        PGH_TRY(order.alloc(sizeof(int32_t) * (size_t)kept));
        PGH_TRY(partial.alloc(sizeof(double) * 2 * kRankParts));
        PGH_TRY(folded.alloc(sizeof(double) * 2));
        PGH_TRY(flag.alloc(sizeof(int)));
        k_rank_iota<<<grid_capped(kept, kSlabBlock), kSlabBlock, 0, rt().stream>>>(iota.as<int32_t>(), kept);
        PGH_HIP(hipGetLastError());
        return 0;
    }
    int sort_column(pgh_mat_t scores, const pgh_rank_plan_s* plan, int col) {
        Runtime& r = rt();
        PGH_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), r.stream));
        k_rank_keys<<<grid_capped(count, kSlabBlock), kSlabBlock, 0, r.stream>>>(scores->data, scores->b, col, plan->kept_row, count, keys.as<float>(), flag.as<int>());
        PGH_HIP(hipGetLastError());
        return sort_pairs_desc(keys.as<float>(), sorted.as<float>(), iota.as<int32_t>(), order.as<int32_t>(), count);
    }
    // the two folded sums of the column, and whether it held a NaN
    int finish(double* host2, int* nan) {
        Runtime& r = rt();
        PGH_HIP(hipMemcpyAsync(nan, flag.p, sizeof(int), hipMemcpyDeviceToHost, r.stream));
        return fold_to_host(partial.as<double>(), folded.as<double>(), host2);
    }
};

int ndcg_sorted(pgh_mat_t scores, pgh_rank_plan_s* plan, int64_t k, double* dcg_host) {
    Runtime& r = rt();
    const int64_t top = k < plan->n_kept ? k : plan->n_kept;
    ColumnSorter sorter;
    PGH_TRY(sorter.prepare(plan->n_kept));
    for (int j = 0; j < scores->b; ++j) {
        PGH_TRY(sorter.sort_column(scores, plan, j));
        k_dcg_parts<<<kRankParts, kSlabBlock, 0, r.stream>>>(plan->kept_known, sorter.order.as<int32_t>(), top, sorter.partial.as<double>());
        double host2[2];
        int nan = 0;
        PGH_TRY(sorter.finish(host2, &nan));
        dcg_host[j] = nan != 0 ? (double)NAN : host2[0];
    }
    return 0;
}

int ndcg_impl(pgh_mat_t scores, pgh_rank_plan_t plan, int64_t k, int32_t route, double* dcg_host, double* idcg_host) {
    PGH_TRY(check_slab("pgh_ndcg", scores, plan));
    PGH_CHECK(dcg_host && idcg_host, "pgh_ndcg: null argument");
    PGH_CHECK(k >= 1, "pgh_ndcg: k >= 1 expected");
    PGH_CHECK(route == PGH_RANK_AUTO || route == PGH_RANK_STREAMING || route == PGH_RANK_SORTED, "pgh_ndcg: unknown route");
    if (scores->b > kSlabMaxCols) return declined(PGH_RANK_DECLINED, "pgh_ndcg", "more than 64 columns");
    const bool too_many = plan->n_rel > PGH_RANK_MAX_RELEVANT;
    bool streaming = route != PGH_RANK_SORTED;
    if (streaming && (too_many || plan->has_negative)) {
        if (route == PGH_RANK_STREAMING)
            return declined(PGH_RANK_DECLINED, "pgh_ndcg", too_many ? "more relevant rows than the per-column sort holds" : "a negative known score");
        streaming = false;
    }
    PGH_TRY(ensure_init());
    double dcg[kSlabMaxCols];
    double idcg = 0.0;
    if (plan->n_rel == 0) {
        for (int j = 0; j < scores->b; ++j) dcg[j] = 0.0;
    } else {
        PGH_TRY(ensure_known_desc(plan));
        Runtime& r = rt();
        PoolBuf partial, folded;
        PGH_TRY(partial.alloc(sizeof(double) * 2 * kRankParts));
        PGH_TRY(folded.alloc(sizeof(double) * 2));
        const int64_t top = k < plan->n_kept ? k : plan->n_kept;
        k_dcg_parts<<<kRankParts, kSlabBlock, 0, r.stream>>>(plan->known_desc, nullptr, top, partial.as<double>());
        double host2[2];
        PGH_TRY(fold_to_host(partial.as<double>(), folded.as<double>(), host2));
        idcg = host2[0];
        PGH_TRY(streaming ? ndcg_streaming(scores, plan, k, dcg) : ndcg_sorted(scores, plan, k, dcg));
    }
    for (int j = 0; j < scores->b; ++j) dcg_host[j] = dcg[j];
    idcg_host[0] = idcg;
    return 0;
}

int spearman_impl(pgh_mat_t scores, pgh_rank_plan_t plan, double* rho_host) {
    PGH_TRY(check_slab("pgh_spearman", scores, plan));
    PGH_CHECK(rho_host, "pgh_spearman: null argument");
    if (scores->b > kSlabMaxCols) return declined(PGH_RANK_DECLINED, "pgh_spearman", "more than 64 columns");
    PGH_TRY(ensure_init());
    double rho[kSlabMaxCols];
    if (plan->n_kept == 0) {
        for (int j = 0; j < scores->b; ++j) rho[j] = (double)NAN;
    } else {
        PGH_TRY(ensure_d_known(plan));
        Runtime& r = rt();
        ColumnSorter sorter;
        PGH_TRY(sorter.prepare(plan->n_kept));
        for (int j = 0; j < scores->b; ++j) {
            PGH_TRY(sorter.sort_column(scores, plan, j));
            k_rho_parts<<<kRankParts, kSlabBlock, 0, r.stream>>>(sorter.sorted.as<float>(), sorter.order.as<int32_t>(), plan->d_known, plan->n_kept,
                                                          sorter.partial.as<double>());
            double host2[2];
            int nan = 0;
            PGH_TRY(sorter.finish(host2, &nan));
            rho[j] = nan != 0 ? (double)NAN : host2[0] / std::sqrt(host2[1] * plan->sum_dk2);
        }
    }
    for (int j = 0; j < scores->b; ++j) rho_host[j] = rho[j];
    return 0;
}
}  // namespace

PGH_WARM_KERNEL(k_rank_fold)

extern "C" int pgh_rank_plan_destroy(pgh_rank_plan_t plan) {
    if (!plan) return 0;
    for (void* p : {(void*)plan->cls, (void*)plan->kept_row, (void*)plan->kept_known, (void*)plan->rel_row, (void*)plan->rel_known,
                    (void*)plan->known_desc, (void*)plan->d_known})
        if (p) pool_free(p);
    delete plan;
    return 0;
}

extern "C" int pgh_rank_plan_create(pgh_vec_t known, pgh_vec_t exclude, pgh_rank_plan_t* out) {
    PGH_CHECK(known && out, "pgh_rank_plan_create: null argument");
    PGH_CHECK(exclude == nullptr || exclude->n == known->n, "pgh_rank_plan_create: known and exclude differ in length");
    PGH_CHECK(known->n < 2147483647LL, "pgh_rank_plan_create: vector too long");
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const int64_t n = known->n;
    std::unique_ptr<pgh_rank_plan_s, int (*)(pgh_rank_plan_t)> plan(new pgh_rank_plan_s(), pgh_rank_plan_destroy);
    plan->n = n;
    if (n == 0) {
        *out = plan.release();
        return 0;
    }
    PoolBuf selected;
    PGH_TRY(selected.alloc(sizeof(int)));
    PGH_TRY(pool_alloc((size_t)n, (void**)&plan->cls));
    unsigned long long counts[4];
    PGH_TRY(classify_labels(known, exclude, plan->cls, counts));
    plan->n_kept = (int64_t)counts[0];
    plan->n_rel = (int64_t)counts[1];
    plan->has_negative = counts[3] != 0 ? 1 : 0;
    // the rows of class >= least in ascending row order, and their known scores
    auto list_rows = [&](uint8_t least, int64_t count, int32_t** rows, float** values) -> int {
        if (count == 0) return 0;
        PGH_TRY(pool_alloc(sizeof(int32_t) * (size_t)count, (void**)rows));
        PGH_TRY(pool_alloc(sizeof(float) * (size_t)count, (void**)values));
        hipcub::CountingInputIterator<int32_t> ids(0);
        const ClassAtLeast keep{plan->cls, least};
        size_t temp_bytes = 0;
        PGH_HIP(hipcub::DeviceSelect::If(nullptr, temp_bytes, ids, *rows, selected.as<int>(), (int)n, keep, r.stream));
        PoolBuf temp;
        PGH_TRY(temp.alloc(temp_bytes));
        PGH_HIP(hipcub::DeviceSelect::If(temp.p, temp_bytes, ids, *rows, selected.as<int>(), (int)n, keep, r.stream));
        k_rank_gather<<<grid_capped(count, kSlabBlock), kSlabBlock, 0, r.stream>>>(known->data, *rows, count, *values);
        PGH_HIP(hipGetLastError());
        PGH_HIP(hipStreamSynchronize(r.stream));
        return 0;
    };
    PGH_TRY(list_rows(1, plan->n_kept, &plan->kept_row, &plan->kept_known));
    PGH_TRY(list_rows(2, plan->n_rel, &plan->rel_row, &plan->rel_known));
    *out = plan.release();
    return 0;
}

extern "C" int pgh_rank_plan_info(pgh_rank_plan_t plan, int64_t* num_kept, int64_t* num_relevant, int32_t* has_negative) {
    PGH_CHECK(plan, "pgh_rank_plan_info: null plan");
    if (num_kept) *num_kept = plan->n_kept;
    if (num_relevant) *num_relevant = plan->n_rel;
    if (has_negative) *has_negative = plan->has_negative;
    return 0;
}

extern "C" int pgh_ndcg(pgh_mat_t scores, pgh_rank_plan_t plan, int64_t k, int32_t route, double* dcg_host, double* idcg_host) {
    return ndcg_impl(scores, plan, k, route, dcg_host, idcg_host);
}

extern "C" int pgh_spearman(pgh_mat_t scores, pgh_rank_plan_t plan, double* rho_host) { return spearman_impl(scores, plan, rho_host); }

extern "C" int pgh_ndcg_vec(pgh_vec_t scores, pgh_rank_plan_t plan, int64_t k, int32_t route, double* dcg_host, double* idcg_host) {
    PGH_CHECK(scores, "pgh_ndcg_vec: null argument");
    pgh_mat_s view;
    view.data = scores->data, view.n = scores->n, view.b = 1;
    return ndcg_impl(&view, plan, k, route, dcg_host, idcg_host);
}

extern "C" int pgh_spearman_vec(pgh_vec_t scores, pgh_rank_plan_t plan, double* rho_host) {
    PGH_CHECK(scores, "pgh_spearman_vec: null argument");
    pgh_mat_s view;
    view.data = scores->data, view.n = scores->n, view.b = 1;
    return spearman_impl(&view, plan, rho_host);
}
