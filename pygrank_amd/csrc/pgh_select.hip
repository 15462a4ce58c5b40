// include/pgh_select.h: node selections that leave the device as lists, and the slab passes of MabsMaintain and SeparateNormalization.
//
// Reference counterpart: Subgraph.transform / Supergraph.transform (pygrank/algorithms/postprocess/subgraph.py:28-32,62-63): a list
// comprehension and a dictionary over all nodes.
//
// The row test (pgh_vec_select), DESIGN.md section 22:
//   k_pick_count   workgroup w owns the rows [4096 w, 4096 w + 4096): four 16-byte loads per lane, one integer count per workgroup
//   hipcub         the exclusive sum of the workgroup counts (one entry more than workgroups: the last prefix is the total)
//   k_pick_write   the same loads; a lane's place is the workgroup's offset + the segments (iteration, wavefront) in front of its own + the
//                  lanes in front of it inside the segment (mbcnt over the four ballots of a quad's slots)
// Row order is (iteration, wavefront, lane, slot) order, so the list ascends.  Every term is an integer: no grid, no arrival order.
//
// The top k (pgh_mat_topk): lanes lie across the columns as in k_select_count (pgh_post.hip): a wavefront reads W = the largest multiple
// of b that is at most 64 consecutive floats, R = W / b whole rows, and lane l stays on column l % b.  A wavefront owns a stretch of
// steps * R consecutive rows.
//   k_top_count    per stretch and column: rows above the column's cut, rows equal to it (ballots masked to the column's lanes)
//   k_top_scan     per column: the exclusive prefix of the stretch counts, and their totals
//   k_top_place    the same loads: a row above the cut goes to slot (prefix + rank), an equal row with equal-rank q < k - above to slot
//                  above + q; slots are rows of the [k, b] staging pair (value, row)
//   k_top_sort     one workgroup per column: (key, row) pairs through the bitonic network in LDS, key descending, row ascending
// Compiled without contraction: the blend is five rounded f32 operations.
#include "pgh_slab.h"
#include "pgh_post.h"
#include "pgh_select.h"

#include <hipcub/hipcub.hpp>

#include <climits>

using namespace pgh;

#pragma clang fp contract(off)

namespace {
static_assert(PGH_SELECT_MAX_COLS == kSlabMaxCols, "the per-column arguments hold kSlabMaxCols entries");

// ---------------------------------------------------------------- the row test
constexpr int kPickBlock = 256;
constexpr int kPickIters = 4;                                   // quads a lane loads
constexpr int kPickRows = kPickBlock * kPickIters * 4;          // rows of a workgroup's stretch

template <int MODE>
__device__ __forceinline__ bool passes(float x, float cut) {
    if (MODE == PGH_SELECT_NONZERO) return x != 0.f;            // true for a NaN, false for -0.0
    if (MODE == PGH_SELECT_GT) return x > cut;
    return x >= cut;
}

// the quad at element e: its values, and bit u set when element e + u exists and passes
template <int MODE>
__device__ __forceinline__ unsigned quad_flags(const float* __restrict__ x, int64_t n, int vec, int64_t e, float cut, float (&v)[4]) {
    if (vec && e + 4 <= n) {
        const float4 w4 = *reinterpret_cast<const float4*>(x + e);
        v[0] = w4.x, v[1] = w4.y, v[2] = w4.z, v[3] = w4.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = e + u < n ? x[e + u] : 0.f;
    }
    unsigned f = 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (e + u < n && passes<MODE>(v[u], cut)) f |= 1u << u;
    return f;
}

__device__ __forceinline__ int64_t quad_element(int it) {
    return 4 * (((int64_t)blockIdx.x * kPickIters + it) * kPickBlock + threadIdx.x);
}

// set bits of `ballot` in the lanes below this one
__device__ __forceinline__ uint32_t lanes_below(unsigned long long ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

template <int MODE>
__global__ __launch_bounds__(kPickBlock) void k_pick_count(const float* __restrict__ x, int64_t n, int vec, float cut,
                                                           uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_wave[kPickBlock / 64];
    uint32_t c = 0u;
#pragma unroll
    for (int it = 0; it < kPickIters; ++it) {
        float v[4];
        c += (uint32_t)__popc(quad_flags<MODE>(x, n, vec, quad_element(it), cut, v));
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

template <int MODE>
__global__ __launch_bounds__(kPickBlock) void k_pick_write(const float* __restrict__ x, int64_t n, int vec, float cut,
                                                           const uint32_t* __restrict__ offsets, int32_t* __restrict__ idx,
                                                           float* __restrict__ values /* or null */) {
    __shared__ uint32_t s_seg[kPickIters * (kPickBlock / 64)];      // [iteration][wavefront]: rows that pass
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float v[kPickIters][4];
    unsigned f[kPickIters];
    uint32_t before[kPickIters];
#pragma unroll
    for (int it = 0; it < kPickIters; ++it) {
        f[it] = quad_flags<MODE>(x, n, vec, quad_element(it), cut, v[it]);
        uint32_t pre = 0u, all = 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned long long ballot = __ballot((f[it] >> u) & 1u);
            pre += lanes_below(ballot);
            all += (uint32_t)__popcll(ballot);
        }
        before[it] = pre;
        if (lane == 0) s_seg[it * (kPickBlock / 64) + wave] = all;
    }
    __syncthreads();
    const uint32_t base = offsets[blockIdx.x];
#pragma unroll
    for (int it = 0; it < kPickIters; ++it) {
        const int mine = it * (kPickBlock / 64) + wave;
        uint32_t pos = base + before[it];
        for (int s = 0; s < mine; ++s) pos += s_seg[s];
        const int64_t e = quad_element(it);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if ((f[it] >> u) & 1u) {
                idx[pos] = (int32_t)(e + u);
                if (values != nullptr) values[pos] = v[it][u];
                ++pos;
            }
        }
    }
}

template <int MODE>
int pick(pgh_vec_t x, float cut, int64_t capacity, int32_t* idx_host, pgh_vec_t values, int64_t* count) {
    Runtime& r = rt();
    const int64_t n = x->n;
    const int grid = (int)((n + kPickRows - 1) / kPickRows);
    const int vec = aligned16(x->data) ? 1 : 0;
    PoolBuf counts, offsets, temp;
    PGH_TRY(counts.alloc(sizeof(uint32_t) * ((size_t)grid + 1)));
    PGH_TRY(offsets.alloc(sizeof(uint32_t) * ((size_t)grid + 1)));
    PGH_HIP(hipMemsetAsync(counts.as<uint32_t>() + grid, 0, sizeof(uint32_t), r.stream));
    k_pick_count<MODE><<<grid, kPickBlock, 0, r.stream>>>(x->data, n, vec, cut, counts.as<uint32_t>());
    PGH_HIP(hipGetLastError());
    size_t bytes = 0;
    PGH_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, counts.as<uint32_t>(), offsets.as<uint32_t>(), grid + 1, r.stream));
    PGH_TRY(temp.alloc(bytes));
    PGH_HIP(hipcub::DeviceScan::ExclusiveSum(temp.p, bytes, counts.as<uint32_t>(), offsets.as<uint32_t>(), grid + 1, r.stream));
    uint32_t total = 0u;
    PGH_HIP(hipMemcpyAsync(&total, offsets.as<uint32_t>() + grid, sizeof(uint32_t), hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(hipStreamSynchronize(r.stream));
    if ((int64_t)total <= capacity && total > 0u) {
        PoolBuf idx;
        PGH_TRY(idx.alloc(sizeof(int32_t) * (size_t)total));
        k_pick_write<MODE><<<grid, kPickBlock, 0, r.stream>>>(x->data, n, vec, cut, offsets.as<uint32_t>(), idx.as<int32_t>(),
                                                              values != nullptr ? values->data : nullptr);
        PGH_HIP(hipGetLastError());
        PGH_HIP(hipMemcpyAsync(idx_host, idx.p, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, r.stream));
        PGH_HIP(hipStreamSynchronize(r.stream));
    }
    *count = (int64_t)total;
    return 0;
}

// ---------------------------------------------------------------- gather and scatter by a checked list
__global__ __launch_bounds__(kSlabBlock) void k_list_gather(const float* __restrict__ x, const int32_t* __restrict__ idx, int64_t count,
                                                            float* __restrict__ out) {
    for (int64_t t = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; t < count; t += (int64_t)gridDim.x * kSlabBlock) out[t] = x[idx[t]];
}

__global__ __launch_bounds__(kSlabBlock) void k_list_scatter(float* __restrict__ dst, const int32_t* __restrict__ idx, int64_t count,
                                                             const float* __restrict__ src) {
    for (int64_t t = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x; t < count; t += (int64_t)gridDim.x * kSlabBlock) dst[idx[t]] = src[t];
}

// the list is inside [0, n) and strictly ascending; 0 or the error status
int list_ready(const char* who, const int32_t* idx_host, int64_t count, int64_t n) {
    int64_t last = -1;
    for (int64_t t = 0; t < count; ++t) {
        const int64_t at = idx_host[t];
        if (at < 0 || at >= n) return fail(std::string(who) + ": index " + std::to_string(at) + " at place " + std::to_string(t) + " lies outside [0, n)");
        if (at <= last) return fail(std::string(who) + ": the indices do not ascend strictly at place " + std::to_string(t));
        last = at;
    }
    return 0;
}

// scatter == false: b[t] = a[idx[t]]; scatter == true: a[idx[t]] = b[t]
int list_move(const char* who, pgh_vec_t a, const int32_t* idx_host, int64_t count, pgh_vec_t b, bool scatter) {
    if (!(a && b)) return fail(std::string(who) + ": null argument");
    if (count < 0 || count > b->n) return fail(std::string(who) + ": count lies outside the operand's length");
    if (count > 0 && idx_host == nullptr) return fail(std::string(who) + ": null argument");
    if (a->data == b->data && a->n > 0) return fail(std::string(who) + ": the operands share their memory");
    PGH_TRY(list_ready(who, idx_host, count, a->n));
    if (count == 0) return 0;
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    PoolBuf idx;
    PGH_TRY(idx.alloc(sizeof(int32_t) * (size_t)count));
    StreamFence fence;                                          // the copy reads the caller's list
    PGH_HIP(hipMemcpyAsync(idx.p, idx_host, sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, r.stream));
    const int grid = grid_capped(count, kSlabBlock * 4);
    if (scatter)
        k_list_scatter<<<grid, kSlabBlock, 0, r.stream>>>(a->data, idx.as<int32_t>(), count, b->data);
    else
        k_list_gather<<<grid, kSlabBlock, 0, r.stream>>>(a->data, idx.as<int32_t>(), count, b->data);
    PGH_HIP(hipGetLastError());
    PGH_HIP(fence.wait());
    return 0;
}

// ---------------------------------------------------------------- the top k of every column
constexpr int kTopBlock = 256;
constexpr int kTopWaves = kTopBlock / 64;
constexpr int kTopUnroll = 4;            // loads a lane has in flight
constexpr int kTopStretches = 4096;      // about as many wavefront stretches as 256 CUs hold at once

struct TopShape {
    int64_t total;       // n * b elements
    int     b;
    int     W;           // lanes of a wavefront that read: the largest multiple of b that is <= 64
    int     R;           // W / b: rows a wavefront reads at once
    int     steps;       // reads of a stretch: it holds steps * R rows
    int     stretches;
    int     k;
};

struct TopCuts {
    float c[kSlabMaxCols];
};

__device__ __forceinline__ uint32_t key_of(float x) {
    uint32_t u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0u;                                   // -0.0 ties with +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the lanes of this lane's column
__device__ __forceinline__ unsigned long long column_lanes(int c, const TopShape& s) {
    unsigned long long mask = 0ull;
    for (int t = 0; t < s.R; ++t) mask |= 1ull << (c + t * s.b);
    return mask;
}

// cnt: [2][b][stretches] -- rows above the cut, rows equal to it
__global__ __launch_bounds__(kTopBlock) void k_top_count(const float* __restrict__ m, TopShape s, TopCuts cuts, uint32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t st = blockIdx.x * (int64_t)kTopWaves + (threadIdx.x >> 6);
    if (st >= s.stretches) return;                                  // (a whole wavefront; no barrier follows)
    const bool on = lane < s.W;
    const int c = lane % s.b;
    const unsigned long long mine = column_lanes(c, s);
    const float cut = cuts.c[c];
    const int64_t e0 = st * (int64_t)s.steps * s.W + lane;
    uint32_t above = 0u, equal = 0u;
    for (int i = 0; i < s.steps; i += kTopUnroll) {
        float x[kTopUnroll];
        bool ok[kTopUnroll];
#pragma unroll
        for (int u = 0; u < kTopUnroll; ++u) {
            const int64_t at = e0 + (int64_t)(i + u) * s.W;
            ok[u] = on && i + u < s.steps && at < s.total;
            x[u] = ok[u] ? m[at] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kTopUnroll; ++u) {
            above += (uint32_t)__popcll(__ballot(ok[u] && x[u] > cut) & mine);
            equal += (uint32_t)__popcll(__ballot(ok[u] && x[u] == cut) & mine);
        }
    }
    if (lane < s.b) {
        cnt[(size_t)c * s.stretches + st] = above;
        cnt[((size_t)s.b + c) * s.stretches + st] = equal;
    }
}

// workgroup q < 2 b: the exclusive prefix of cnt[q][0 .. stretches) in place, its total to tot[q]
__global__ __launch_bounds__(kTopBlock) void k_top_scan(uint32_t* __restrict__ cnt, int stretches, uint32_t* __restrict__ tot) {
    __shared__ uint32_t s_run[kTopBlock];
    uint32_t* __restrict__ col = cnt + (size_t)blockIdx.x * stretches;
    const int run = (stretches + kTopBlock - 1) / kTopBlock;
    const int lo = min((int)threadIdx.x * run, stretches), hi = min(lo + run, stretches);
    uint32_t sum = 0u;
    for (int i = lo; i < hi; ++i) sum += col[i];
    s_run[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0u;
        for (int t = 0; t < kTopBlock; ++t) {
            const uint32_t v = s_run[t];
            s_run[t] = acc;
            acc += v;
        }
        tot[blockIdx.x] = acc;
    }
    __syncthreads();
    uint32_t acc = s_run[threadIdx.x];
    for (int i = lo; i < hi; ++i) {
        const uint32_t v = col[i];
        col[i] = acc;
        acc += v;
    }
}

// off: cnt after k_top_scan.  stage_val / stage_row: [k][b]; every store is guarded by slot < k.
__global__ __launch_bounds__(kTopBlock) void k_top_place(const float* __restrict__ m, TopShape s, TopCuts cuts, const uint32_t* __restrict__ off,
                                                         const uint32_t* __restrict__ tot, float* __restrict__ stage_val,
                                                         int32_t* __restrict__ stage_row) {
    const int lane = threadIdx.x & 63;
    const int64_t st = blockIdx.x * (int64_t)kTopWaves + (threadIdx.x >> 6);
    if (st >= s.stretches) return;
    const bool on = lane < s.W;
    const int c = lane % s.b;
    const unsigned long long mine = column_lanes(c, s);
    const unsigned long long below = mine & ((1ull << lane) - 1ull);
    const float cut = cuts.c[c];
    const uint32_t k = (uint32_t)s.k;
    const uint32_t g = tot[c];                                      // rows above the cut in the whole column: fewer than k
    const uint32_t room = k > g ? k - g : 0u;                       // equal rows that are kept
    uint32_t above = off[(size_t)c * s.stretches + st], equal = off[((size_t)s.b + c) * s.stretches + st];
    const int64_t e0 = st * (int64_t)s.steps * s.W + lane;
    const int64_t row0 = st * (int64_t)s.steps * s.R + lane / s.b;
    for (int i = 0; i < s.steps; i += kTopUnroll) {
        float x[kTopUnroll];
        bool ok[kTopUnroll];
#pragma unroll
        for (int u = 0; u < kTopUnroll; ++u) {
            const int64_t at = e0 + (int64_t)(i + u) * s.W;
            ok[u] = on && i + u < s.steps && at < s.total;
            x[u] = ok[u] ? m[at] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kTopUnroll; ++u) {
            const bool fa = ok[u] && x[u] > cut, fe = ok[u] && x[u] == cut;
            const unsigned long long ba = __ballot(fa), be = __ballot(fe);
            const int32_t row = (int32_t)(row0 + (int64_t)(i + u) * s.R);
            if (fa) {
                const uint32_t slot = above + (uint32_t)__popcll(ba & below);
                if (slot < k) {
                    stage_val[(size_t)slot * s.b + c] = x[u];
                    stage_row[(size_t)slot * s.b + c] = row;
                }
            }
            if (fe) {
                const uint32_t q = equal + (uint32_t)__popcll(be & below);
                if (q < room) {
                    stage_val[(size_t)(g + q) * s.b + c] = x[u];
                    stage_row[(size_t)(g + q) * s.b + c] = row;
                }
            }
            above += (uint32_t)__popcll(ba & mine);
            equal += (uint32_t)__popcll(be & mine);
        }
    }
}

// workgroup j: column j's k staged pairs, sorted; the value of a place is read back from the slab (the stored bits, -0.0 included)
__global__ __launch_bounds__(kTopBlock) void k_top_sort(const float* __restrict__ m, int b, int k, int padded, const float* __restrict__ stage_val,
                                                        const int32_t* __restrict__ stage_row, int32_t* __restrict__ out_row,
                                                        double* __restrict__ out_val) {
    __shared__ uint32_t s_key[PGH_TOPK_MAX_K];
    __shared__ int32_t s_row[PGH_TOPK_MAX_K];
    const int c = blockIdx.x;
    for (int t = threadIdx.x; t < padded; t += kTopBlock) {
        s_key[t] = t < k ? key_of(stage_val[(size_t)t * b + c]) : 0u;      // (padding goes behind every pair: lowest key, highest row)
        s_row[t] = t < k ? stage_row[(size_t)t * b + c] : INT_MAX;
    }
    __syncthreads();
    bitonic_sort_lds<kTopBlock>(
        padded, [&](int i, int j) { return s_key[i] > s_key[j] || (s_key[i] == s_key[j] && s_row[i] < s_row[j]); },
        [&](int i, int j) {
            const uint32_t key = s_key[i];
            const int32_t row = s_row[i];
            s_key[i] = s_key[j], s_row[i] = s_row[j];
            s_key[j] = key, s_row[j] = row;
        });
    for (int t = threadIdx.x; t < k; t += kTopBlock) {
        const int32_t row = s_row[t];
        out_row[(size_t)t * b + c] = row;
        out_val[(size_t)t * b + c] = (double)m[(int64_t)row * b + c];
    }
}

// ---------------------------------------------------------------- the slab passes of MabsMaintain and SeparateNormalization
enum MapOp : int { kMapScale = 0, kMapBlend = 1 };

struct MapShape {
    int64_t total;      // n * b elements
    int64_t quads;      // ceil(total / 4)
    int64_t stride_q;   // virtual lanes that take quads: a multiple of b
    int     b;
    int     vec;        // both slabs are 16-byte aligned: whole quads travel as one word
};

struct ColArgs {
    float a[kSlabMaxCols];
    float d[kSlabMaxCols];
};

// the quad walk of k_post_map (pgh_post.hip): slot u of a lane stays on column (4 lane + u) % b and moves down 4 stride_q / b rows a step
template <int OP>
__global__ __launch_bounds__(kSlabBlock) void k_select_map(const float* __restrict__ m, float* __restrict__ out, MapShape s, ColArgs cols,
                                                           const float* __restrict__ v) {
    const int64_t lane = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x;
    if (lane >= s.stride_q) return;
    float a[4], d[4];
    int64_t row[4];
    const int c0 = (int)((4 * lane) % s.b);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = (c0 + u) % s.b;
        a[u] = cols.a[c];
        d[u] = cols.d[c];
        row[u] = (4 * lane) / s.b + (c0 + u) / s.b;
    }
    const int64_t rows_a_step = 4 * s.stride_q / s.b;
    for (int64_t q = lane; q < s.quads; q += s.stride_q) {
        const int64_t e = 4 * q;
        const bool whole = s.vec && e + 4 <= s.total;
        float x[4], r[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
        if (whole) {
            const float4 w4 = *reinterpret_cast<const float4*>(m + e);
            x[0] = w4.x, x[1] = w4.y, x[2] = w4.z, x[3] = w4.w;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = e + u < s.total ? m[e + u] : 0.f;
        }
        if (OP == kMapBlend) {
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = e + u < s.total ? v[row[u]] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (OP == kMapScale) o[u] = x[u] * a[u];
            if (OP == kMapBlend) {
                const float first = x[u] * r[u];
                const float rest = 1.f - r[u];
                const float second = x[u] * rest;
                const float left = first * a[u], right = second * d[u];
                o[u] = left + right;
            }
            row[u] += rows_a_step;
        }
        if (whole) {
            *reinterpret_cast<float4*>(out + e) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (e + u < s.total) out[e + u] = o[u];
        }
    }
}

// The walk of k_col_stats (pgh_measure.hip): every virtual thread below the stride keeps one column; the threads of a part that share a
// column are folded through LDS in thread order.  partial: [kSlabParts][b][4] = sum m s, sum m (1 - s), 0, 0.
__global__ __launch_bounds__(kSlabBlock) void k_split_sums(const float* __restrict__ m, const float* __restrict__ v, int64_t n, int b,
                                                           double* __restrict__ partial) {
    __shared__ double s_first[kSlabBlock], s_second[kSlabBlock];
    const int64_t total = n * b;
    const int64_t stride = ((int64_t)kSlabParts * kSlabBlock) / b * b;
    const int64_t rows_a_step = stride / b;
    for (int part = blockIdx.x; part < kSlabParts; part += gridDim.x) {
        const int64_t first = (int64_t)part * kSlabBlock;
        double one = 0.0, two = 0.0;
        if (first + threadIdx.x < stride) {
            int64_t i = first + threadIdx.x, row = i / b;
            for (; i < total; i += stride, row += rows_a_step) {
                const float x = m[i], r = v[row];
                const float rest = 1.f - r;
                one += (double)(x * r);
                two += (double)(x * rest);
            }
        }
        s_first[threadIdx.x] = one;
        s_second[threadIdx.x] = two;
        __syncthreads();
        for (int j = threadIdx.x; j < b; j += kSlabBlock) {
            const int start = (int)(((int64_t)j - first % b + b) % b);     // first thread of this part that owns column j
            double t = 0.0, q = 0.0;
            for (int k = start; k < kSlabBlock; k += b) {
                t += s_first[k];
                q += s_second[k];
            }
            double* o = partial + ((int64_t)part * b + j) * 4;
            o[0] = t;
            o[1] = q;
            o[2] = 0.0;
            o[3] = 0.0;
        }
        __syncthreads();
    }
}

// the checks the two maps share; 0: launch, 1: nothing to do (no rows), else the status is in *status
int map_ready(const char* who, pgh_mat_t m, pgh_mat_t out, int* status) {
    if (!(m && out)) return *status = fail(std::string(who) + ": null argument"), -1;
    if (!(m->b >= 1 && m->n >= 0)) return *status = fail(std::string(who) + ": at least one column expected"), -1;
    if (!(m->n == out->n && m->b == out->b)) return *status = fail(std::string(who) + ": m and out differ in shape"), -1;
    if (m->b > kSlabMaxCols) return *status = declined(PGH_SELECT_DECLINED, who, "more than 64 columns"), -1;
    if (m->n == 0) return *status = 0, 1;
    if (out->data == m->data) return *status = fail(std::string(who) + ": out shares its memory with m"), -1;
    return 0;
}

template <int OP>
int launch_map(pgh_mat_t m, pgh_mat_t out, const ColArgs& cols, const float* v) {
    PGH_TRY(ensure_init());
    MapShape s;
    s.total = m->n * m->b;
    s.quads = (s.total + 3) / 4;
    const int grid = grid_capped(s.quads, kSlabBlock * 2);
    s.stride_q = ((int64_t)grid * kSlabBlock) / m->b * m->b;
    s.b = m->b;
    s.vec = aligned16(m->data) && aligned16(out->data) ? 1 : 0;
    k_select_map<OP><<<grid, kSlabBlock, 0, rt().stream>>>(m->data, out->data, s, cols, v);
    PGH_HIP(hipGetLastError());
    return 0;
}
}  // namespace

PGH_WARM_KERNEL(k_top_scan)

extern "C" int pgh_vec_select(pgh_vec_t x, int32_t mode, double cut, int64_t capacity, int32_t* idx_host, pgh_vec_t values, int64_t* count) {
    PGH_CHECK(x && idx_host && count, "pgh_vec_select: null argument");
    PGH_CHECK(mode == PGH_SELECT_NONZERO || mode == PGH_SELECT_GT || mode == PGH_SELECT_GE, "pgh_vec_select: unknown mode");
    PGH_CHECK(capacity >= 0, "pgh_vec_select: negative capacity");
    PGH_CHECK(x->n >= 0 && x->n < 2147483648LL, "pgh_vec_select: more than 2^31 - 1 rows");
    PGH_CHECK(values == nullptr || values->n >= capacity, "pgh_vec_select: values holds fewer than capacity entries");
    PGH_CHECK(values == nullptr || values->data != x->data || x->n == 0, "pgh_vec_select: values shares its memory with x");
    if (x->n == 0) {
        *count = 0;
        return 0;
    }
    PGH_TRY(ensure_init());
    if (mode == PGH_SELECT_NONZERO) return pick<PGH_SELECT_NONZERO>(x, 0.f, capacity, idx_host, values, count);
    if (mode == PGH_SELECT_GT) return pick<PGH_SELECT_GT>(x, (float)cut, capacity, idx_host, values, count);
    return pick<PGH_SELECT_GE>(x, (float)cut, capacity, idx_host, values, count);
}

extern "C" int pgh_vec_gather(pgh_vec_t x, const int32_t* idx_host, int64_t count, pgh_vec_t out) {
    return list_move("pgh_vec_gather", x, idx_host, count, out, false);
}

extern "C" int pgh_vec_scatter(pgh_vec_t dst, const int32_t* idx_host, int64_t count, pgh_vec_t src) {
    return list_move("pgh_vec_scatter", dst, idx_host, count, src, true);
}

extern "C" int pgh_mat_topk(pgh_mat_t m, int64_t k, int32_t* idx_host, double* val_host) {
    PGH_CHECK(m && idx_host && val_host, "pgh_mat_topk: null argument");
    PGH_CHECK(m->b >= 1 && m->n >= 0, "pgh_mat_topk: at least one column expected");
    PGH_CHECK(m->n < 2147483648LL, "pgh_mat_topk: more than 2^31 - 1 rows");
    PGH_CHECK(k >= 1 && k <= m->n, "pgh_mat_topk: k outside [1, n]");
    if (m->b > kSlabMaxCols) return declined(PGH_SELECT_DECLINED, "pgh_mat_topk", "more than 64 columns");
    if (k > PGH_TOPK_MAX_K) return declined(PGH_SELECT_DECLINED, "pgh_mat_topk", "k above PGH_TOPK_MAX_K");
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const int b = m->b;
    double cuts_host[kSlabMaxCols];
    PGH_TRY(pgh_post_kth_largest(m, k, cuts_host));
    TopCuts cuts;
    for (int c = 0; c < kSlabMaxCols; ++c) cuts.c[c] = c < b ? (float)cuts_host[c] : 0.f;
    TopShape s;
    s.total = m->n * b;
    s.b = b;
    s.W = kSlabMaxCols / b * b;
    s.R = s.W / b;
    const int64_t reads = (m->n + s.R - 1) / s.R;                   // wavefront reads that cover the slab
    int64_t steps = (reads + kTopStretches - 1) / kTopStretches;
    if (steps < 2 * kTopUnroll) steps = 2 * kTopUnroll;
    s.steps = (int)steps;
    s.stretches = (int)((reads + steps - 1) / steps);
    s.k = (int)k;
    const int grid = (s.stretches + kTopWaves - 1) / kTopWaves;
    const size_t slots = (size_t)k * b;
    PoolBuf cnt, tot, stage_val, stage_row, out_row, out_val;
    PGH_TRY(cnt.alloc(sizeof(uint32_t) * 2 * (size_t)b * s.stretches));
    PGH_TRY(tot.alloc(sizeof(uint32_t) * 2 * (size_t)b));
    PGH_TRY(stage_val.alloc(sizeof(float) * slots));
    PGH_TRY(stage_row.alloc(sizeof(int32_t) * slots));
    PGH_TRY(out_row.alloc(sizeof(int32_t) * slots));
    PGH_TRY(out_val.alloc(sizeof(double) * slots));
    // (a column with a NaN may leave slots unfilled: they read as row 0)
    PGH_HIP(hipMemsetAsync(stage_val.p, 0, sizeof(float) * slots, r.stream));
    PGH_HIP(hipMemsetAsync(stage_row.p, 0, sizeof(int32_t) * slots, r.stream));
    k_top_count<<<grid, kTopBlock, 0, r.stream>>>(m->data, s, cuts, cnt.as<uint32_t>());
    PGH_HIP(hipGetLastError());
    k_top_scan<<<2 * b, kTopBlock, 0, r.stream>>>(cnt.as<uint32_t>(), s.stretches, tot.as<uint32_t>());
    PGH_HIP(hipGetLastError());
    k_top_place<<<grid, kTopBlock, 0, r.stream>>>(m->data, s, cuts, cnt.as<uint32_t>(), tot.as<uint32_t>(), stage_val.as<float>(),
                                                  stage_row.as<int32_t>());
    PGH_HIP(hipGetLastError());
    int padded = 1;
    while (padded < (int)k) padded <<= 1;
    k_top_sort<<<b, kTopBlock, 0, r.stream>>>(m->data, b, (int)k, padded, stage_val.as<float>(), stage_row.as<int32_t>(),
                                              out_row.as<int32_t>(), out_val.as<double>());
    PGH_HIP(hipGetLastError());
    PGH_HIP(hipMemcpyAsync(idx_host, out_row.p, sizeof(int32_t) * slots, hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(hipMemcpyAsync(val_host, out_val.p, sizeof(double) * slots, hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(hipStreamSynchronize(r.stream));
    return 0;
}

extern "C" int pgh_mat_col_scale(pgh_mat_t m, const double* scale_host, pgh_mat_t out) {
    int status = 0;
    if (map_ready("pgh_mat_col_scale", m, out, &status) != 0) return status;
    PGH_CHECK(scale_host, "pgh_mat_col_scale: null argument");
    ColArgs cols;
    for (int c = 0; c < kSlabMaxCols; ++c) cols.a[c] = c < m->b ? (float)scale_host[c] : 1.f, cols.d[c] = 0.f;
    return launch_map<kMapScale>(m, out, cols, nullptr);
}

extern "C" int pgh_mat_split_sums(pgh_mat_t m, pgh_vec_t s, double* sums_host) {
    PGH_CHECK(m && s && sums_host, "pgh_mat_split_sums: null argument");
    PGH_CHECK(m->b >= 1 && m->n >= 0, "pgh_mat_split_sums: at least one column expected");
    PGH_CHECK(s->n == m->n, "pgh_mat_split_sums: s does not have one entry per row");
    const int b = m->b;
    if (b > kSlabMaxCols) return declined(PGH_SELECT_DECLINED, "pgh_mat_split_sums", "more than 64 columns");
    if (m->n == 0) {
        for (int c = 0; c < 2 * b; ++c) sums_host[c] = 0.0;
        return 0;
    }
    PGH_TRY(ensure_init());
    PoolBuf partial;
    PGH_TRY(partial.alloc(sizeof(double) * (size_t)kSlabParts * b * 4));
    k_split_sums<<<parts_grid(), kSlabBlock, 0, rt().stream>>>(m->data, s->data, m->n, b, partial.as<double>());
    PGH_HIP(hipGetLastError());
    double folded[kSlabMaxCols * 4];
    PGH_TRY(fold_fields_to_host<kFoldSums>(partial.as<double>(), kSlabParts, b, b, folded));
    for (int c = 0; c < b; ++c) sums_host[2 * c] = folded[4 * c], sums_host[2 * c + 1] = folded[4 * c + 1];
    return 0;
}

extern "C" int pgh_mat_split_blend(pgh_mat_t m, pgh_vec_t s, const double* a_host, const double* b_host, pgh_mat_t out) {
    PGH_CHECK(s, "pgh_mat_split_blend: null argument");
    PGH_CHECK(m == nullptr || s->n == m->n, "pgh_mat_split_blend: s does not have one entry per row");
    int status = 0;
    if (map_ready("pgh_mat_split_blend", m, out, &status) != 0) return status;
    PGH_CHECK(a_host && b_host, "pgh_mat_split_blend: null argument");
    ColArgs cols;
    for (int c = 0; c < kSlabMaxCols; ++c) cols.a[c] = c < m->b ? (float)a_host[c] : 0.f, cols.d[c] = c < m->b ? (float)b_host[c] : 0.f;
    return launch_map<kMapBlend>(m, out, cols, s->data);
}
