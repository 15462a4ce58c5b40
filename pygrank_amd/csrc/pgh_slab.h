// What the slab measures share: launch shapes, the refusal helper, the folds of block and part partials, the
// label classification of the plans and the LDS bitonic network.  Header only: the kernels are templates, so every translation unit
// instantiates the ones it launches into its own code object.
// A fold's order is part of its result: a fold lives here only when every user adds in exactly this order.
#pragma once
#include "pgh_common.h"

#include <cmath>

namespace pgh {
namespace {     // internal linkage, like everything else a unit launches: nothing here joins the library's exported symbols

constexpr int kSlabBlock = 256;
constexpr int kSlabParts = 1024;     // row parts of a slab: 256 CUs x 4 workgroups take one each
constexpr int kSlabMaxCols = 64;
constexpr int kSlabMaxGrid = 2048;   // 256 CUs x 8 workgroups, grid-stride beyond
static_assert(kSlabMaxGrid <= kMaxPartials, "a grid-stride kernel leaves one block partial per workgroup in Runtime::d_partials");

// workgroups for `items` at `per_block` each: at least one, at most kSlabMaxGrid
int grid_capped(int64_t items, int per_block) {
    int64_t g = (items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return (int)(g > kSlabMaxGrid ? kSlabMaxGrid : g);
}

// kernels that walk `parts` fixed parts: the grid comes from the device, not from the rows; every workgroup walks parts / grid of them
int parts_grid(int parts = kSlabParts) {
    const int g = rt().num_cus * 4;
    return g < 1 ? 1 : (g > parts ? parts : g);
}

// lanes that share a row when every lane holds four columns: the power of two >= cols / 4
int lpr_for(int cols) {
    int lpr = 1;
    while (lpr * 4 < cols) lpr <<= 1;
    return lpr;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// a refusal: nothing was enqueued, nothing was written
int declined(int status, const char* who, const std::string& why) { return declined(status, who + (" declined: " + why)); }

// Behind the loads of an iteration: neither the optimiser nor the scheduler moves a load below this point, so every load is in flight
// before the first use ("Waits"; without it the compiler sinks each load to its use and waits for them in turn).
// The operands of a kernel that calls it carry no __restrict__: with it the optimiser moves loads past this point to their uses
// (measured in the assembly of k_lfpr_close: 4 + 3 loads with a drained wait between them).
__device__ __forceinline__ void loads_issued() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// the sum of the lanes l, l + stop, l + 2 stop, ... of a wavefront, valid in the lanes below `stop` (a power of two)
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v, int stop) {
    for (int off = 32; off >= stop; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// ---------------------------------------------------------------- partial[parts][cols][4] -> out[cols][4]
enum FoldKind : int { kFoldSum = 0, kFoldMax = 1, kFoldMin = 2, kFoldCount = 3 };   // kFoldCount: 64-bit integers travelling as bit patterns
constexpr int fold_kinds(int f0, int f1, int f2, int f3) { return f0 | f1 << 2 | f2 << 4 | f3 << 6; }
constexpr int kFoldSums = fold_kinds(kFoldSum, kFoldSum, kFoldSum, kFoldSum);

__device__ __forceinline__ double fold_join(int kind, double a, double b) {
    if (kind == kFoldMax) return fmax(a, b);
    if (kind == kFoldMin) return fmin(a, b);
    if (kind == kFoldCount) return __longlong_as_double(__double_as_longlong(a) + __double_as_longlong(b));
    return a + b;
}

// out[4 j + f] = the parts' partial[.][j][f] in index order: workgroup j, thread (slice k, f) folds the parts k, k + 64, ..., then the
// 64 slices are folded in slice order.  Field f is folded as FoldKind (KINDS >> 2 f) & 3.
template <int KINDS>
__global__ __launch_bounds__(kSlabBlock) void k_fold_fields(const double* __restrict__ partial, int parts, int cols, double* __restrict__ out) {
    __shared__ double s_v[kSlabBlock];
    const int j = blockIdx.x, f = threadIdx.x & 3, k = threadIdx.x >> 2;
    const int kind = (KINDS >> (2 * f)) & 3;
    double acc = kind == kFoldMax ? -INFINITY : (kind == kFoldMin ? INFINITY : 0.0);     // (the bits of 0.0 are the integer 0)
    for (int p = k; p < parts; p += kSlabBlock / 4) acc = fold_join(kind, acc, partial[((int64_t)p * cols + j) * 4 + f]);
    s_v[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < 4) {
        double r = s_v[f];
        for (int q = 1; q < kSlabBlock / 4; ++q) r = fold_join(kind, r, s_v[q * 4 + f]);
        out[j * 4 + f] = r;
    }
}

// out_host[4 j + f], j < cols <- the fold of partial[parts][stride][4] (stride >= cols columns are laid out, the first cols are asked
// for); waits for the engine's stream, so whatever the kernels before it read from the caller has been read
template <int KINDS>
int fold_fields_to_host(const double* partial, int parts, int stride, int cols, double* out_host) {
    Runtime& r = rt();
    PoolBuf folded;
    PGH_TRY(folded.alloc(sizeof(double) * (size_t)cols * 4));
    k_fold_fields<KINDS><<<cols, kSlabBlock, 0, r.stream>>>(partial, parts, stride, folded.as<double>());
    PGH_HIP(hipGetLastError());
    PGH_HIP(hipMemcpyAsync(out_host, folded.p, sizeof(double) * (size_t)cols * 4, hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(hipStreamSynchronize(r.stream));
    return 0;
}

// ---------------------------------------------------------------- block partials [regions][STRIDE] -> out[regions]
// out[k] = fold of region k's `count` block partials, k < regions: thread t takes partials t, t + 256, ... in order, then the block
// reduction; region `max_at` (-1: none) is a maximum of non-negative values, the others are sums
template <int STRIDE>
__global__ __launch_bounds__(kSlabBlock) void k_fold_regions(const double* __restrict__ partials, int count, int regions, int max_at,
                                                             double* __restrict__ out) {
    __shared__ double s_red[4];
    for (int k = 0; k < regions; ++k) {
        const double* __restrict__ part = partials + (size_t)k * STRIDE;
        double acc = 0.0;
        if (k == max_at) {
            for (int i = threadIdx.x; i < count; i += kSlabBlock) acc = fmax(acc, part[i]);
            acc = block_reduce_256<1>(acc, s_red);
        } else {
            for (int i = threadIdx.x; i < count; i += kSlabBlock) acc += part[i];
            acc = block_reduce_256<0>(acc, s_red);
        }
        if (threadIdx.x == 0) out[k] = acc;
    }
}

// sums_host[0 .. regions) <- the folds of the first `regions` regions of Runtime::d_partials, `grid` block partials each.  (The host
// wrappers are templates like their kernels: a unit that does not call one does not instantiate its kernel either.)
template <int STRIDE = kMaxPartials>
int fold_regions_to_host(int grid, int regions, int max_at, double* sums_host) {
    Runtime& r = rt();
    k_fold_regions<STRIDE><<<1, kSlabBlock, 0, r.stream>>>(r.d_partials, grid, regions, max_at, r.d_scalars);
    PGH_HIP(hipGetLastError());
    PGH_TRY(scalars_to_host(0, regions));
    for (int k = 0; k < regions; ++k) sums_host[k] = r.h_scalars[k];
    return 0;
}

// ---------------------------------------------------------------- the class byte of a (known, exclude) pair of label vectors
// cls[i] = 0 excluded, 1 kept, 2 kept and known != 0; counts += {kept, class 2, class 1, kept with known < 0}.  Integer sums: lanes
// (shuffles), then one atomic per wavefront and non-zero count, so nothing depends on the grid or on arrival order.
template <bool HAS_EXCLUDE>
__global__ __launch_bounds__(kSlabBlock) void k_classify_labels(const float* __restrict__ known, const float* __restrict__ exclude, int64_t n,
                                                                uint8_t* __restrict__ cls, unsigned long long* __restrict__ counts) {
    unsigned long long c[4] = {0, 0, 0, 0};
    for (int64_t i = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSlabBlock) {
        const bool out = HAS_EXCLUDE && exclude[i] != 0.f;
        const float k = known[i];
        const uint8_t cl = out ? 0 : (k != 0.f ? 2 : 1);
        cls[i] = cl;
        c[0] += cl != 0;
        c[1] += cl == 2;
        c[2] += cl == 1;
        c[3] += cl != 0 && k < 0.f;
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const unsigned long long w = wave_sum_u64(c[f], 1);
        if ((threadIdx.x & 63) == 0 && w != 0) atomicAdd(&counts[f], w);
    }
}

// cls[0 .. n) and counts_host[4] of two label vectors of equal length (exclude may be null); waits for the engine's stream
template <typename Count>
int classify_labels(pgh_vec_t known, pgh_vec_t exclude, uint8_t* cls, Count (&counts_host)[4]) {
    static_assert(sizeof(Count) == sizeof(unsigned long long), "the counts are 64-bit integers");
    Runtime& r = rt();
    const int64_t n = known->n;
    PoolBuf counts;
    PGH_TRY(counts.alloc(sizeof(unsigned long long) * 4));
    PGH_HIP(hipMemsetAsync(counts.p, 0, sizeof(unsigned long long) * 4, r.stream));
    if (n > 0) {
        const int grid = grid_capped(n, kSlabBlock * 8);
        if (exclude != nullptr)
            k_classify_labels<true><<<grid, kSlabBlock, 0, r.stream>>>(known->data, exclude->data, n, cls, counts.as<unsigned long long>());
        else
            k_classify_labels<false><<<grid, kSlabBlock, 0, r.stream>>>(known->data, nullptr, n, cls, counts.as<unsigned long long>());
        PGH_HIP(hipGetLastError());
    }
    PGH_HIP(hipMemcpyAsync(counts_host, counts.p, sizeof(unsigned long long) * 4, hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(hipStreamSynchronize(r.stream));
    return 0;
}

// ---------------------------------------------------------------- the bitonic network over `padded` (a power of two) LDS entries
// before(i, j): entry i belongs in front of entry j; swap(i, j) exchanges them.  Every thread of the BLOCK-thread workgroup calls it,
// behind a barrier that made the entries visible.  Entries that no `before` orders (a NaN key) stay where the exchanges leave them.
template <int BLOCK, typename Before, typename Swap>
__device__ __forceinline__ void bitonic_sort_lds(int padded, Before before, Swap swap) {
    for (int size = 2; size <= padded; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < padded; t += BLOCK) {
                const int other = t ^ stride;
                if (other > t && before(other, t) == ((t & size) == 0)) swap(t, other);
            }
            __syncthreads();
        }
    }
}

}  // namespace
}  // namespace pgh
