// include/pgh_post.h: the postprocessors' transformations on [n, b] slabs, for up to 64 columns at once.
//
// Reference counterpart: the _transform of Normalize, Ordinals, Top, Threshold, Sweep and LinearSweep
// (pygrank/algorithms/postprocess/postprocess.py:106-450): dictionary comprehensions over the nodes and one sorted() per rank vector.
//
// The select (pgh_post_kth_largest), DESIGN.md section 20:
//   k_select_count  one pass over the slab: the 8-bit digit `pass` (from the top) of every element whose higher digits equal its
//                   column's prefix is counted in LDS, then the workgroup's counts join the pass's global bins
//   k_select_pick   per column: the digit whose bin holds the k-th largest of the elements still in the race, and the k left inside it
// Keys: the f32 bits with the sign bit flipped (positive) or all bits flipped (negative), -0.0 taken for +0.0: unsigned order is value
// order.  Lanes lie across the columns: global lane g walks the elements g, g + S, g + 2 S, ... of the row-major slab, where S is a
// multiple of W = the largest multiple of b that is at most 64.  So a lane stays on "wide column" w = g % W of column w % b, the 64
// lanes of a wavefront read 256 consecutive bytes, and they count into bins[digit][w]: different LDS banks whatever the digits are
// (W = 63 for b = 3, 7, 9, 21: lanes 0 and 63 share one).  uint32 [256][64] bins are the 64 KiB of static LDS: two workgroups of 1024
// lanes per CU, 32 waves.  Counts are integers: no order of arrival, no grid shape changes them.
//
// The maps (threshold, affine, row_op): one kernel template on the quad walk of pgh_oversample.hip -- virtual lane v takes the quads
// v, v + stride_q, ... and stride_q is a multiple of b, so slot u of a lane stays on column (4 v + u) % b and moves down by
// 4 stride_q / b rows a step: the per-column operands are read once and nothing is divided inside the loop.  They arrive as kernel
// arguments (2 x 64 floats), so no entry waits for the stream.
// Compiled without contraction; the quotients are IEEE divisions like those of pgh_ewise_vs.
//
// The ordinals: k_post_transpose lays the columns out one after the other (64 rows a tile through LDS), every column goes through
// pgh_vec_ordinals itself, and the positions are transposed back.
#include "pgh_slab.h"
#include "pgh_post.h"

#include <cmath>
#include <cstring>

using namespace pgh;

#pragma clang fp contract(off)

namespace {
static_assert(PGH_POST_MAX_COLS == kSlabMaxCols, "the per-column arguments hold kSlabMaxCols entries");

// ---------------------------------------------------------------- the select
constexpr int kSelBlock = 1024;
constexpr int kSelDigits = 256;      // 8 bits a pass, 4 passes
constexpr int kSelPasses = 4;
constexpr int kSelUnroll = 8;        // loads a lane has in flight

struct SelShape {
    int64_t total;      // n * b elements
    int64_t stride;     // global lanes that take elements: grid * kSelBlock rounded down to a multiple of W
    int     b;
    int     W;          // wide columns: the largest multiple of b that is <= 64
};

__device__ __forceinline__ uint32_t key_of(float x) {
    uint32_t u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0u;                                   // -0.0 ties with +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

float value_of(uint32_t key) {
    const uint32_t u = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
    float x;
    std::memcpy(&x, &u, sizeof x);
    return x;
}

__global__ __launch_bounds__(kSelBlock) void k_select_count(const float* __restrict__ m, SelShape s, int pass,
                                                             const uint32_t* __restrict__ prefix /* [b] */,
                                                             uint32_t* __restrict__ bins /* [256][b] of this pass */) {
    __shared__ uint32_t s_bins[kSelDigits * kSlabMaxCols];
    const int W = s.W;
    for (int e = threadIdx.x; e < kSelDigits * W; e += kSelBlock) s_bins[e] = 0u;
    __syncthreads();
    const int64_t g = blockIdx.x * (int64_t)kSelBlock + threadIdx.x;
    if (g < s.stride) {
        const int w = (int)(g % W);
        const int shift = 24 - 8 * pass;
        const uint32_t pre = pass > 0 ? prefix[w % s.b] : 0u;     // the digits above this pass's (none in pass 0: every element matches)
        uint32_t* mine = s_bins + w;
        for (int64_t i = g; i < s.total; i += s.stride * kSelUnroll) {
            float x[kSelUnroll];
#pragma unroll
            for (int u = 0; u < kSelUnroll; ++u) {
                const int64_t at = i + u * s.stride;
                x[u] = at < s.total ? m[at] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kSelUnroll; ++u) {
                const uint32_t top = key_of(x[u]) >> shift;
                if (i + u * s.stride < s.total && (top >> 8) == pre) atomicAdd(&mine[(top & 255u) * W], 1u);
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kSelDigits * W; e += kSelBlock) {
        const uint32_t c = s_bins[e];
        if (c != 0u) atomicAdd(&bins[(e / W) * s.b + (e % W) % s.b], c);
    }
}

// one workgroup: the pass's bins come into LDS, then lane j walks column j's bins from the top digit down
__global__ __launch_bounds__(kSlabBlock) void k_select_pick(const uint32_t* __restrict__ bins /* [256][b] */, int b, int pass, uint32_t k0,
                                                            uint32_t* __restrict__ prefix /* [b] */, uint32_t* __restrict__ left /* [b] */) {
    __shared__ uint32_t s_bins[kSelDigits * kSlabMaxCols];
    for (int e = threadIdx.x; e < kSelDigits * b; e += kSlabBlock) s_bins[e] = bins[e];
    __syncthreads();
    const int j = threadIdx.x;
    if (j >= b) return;
    const uint32_t k = pass > 0 ? left[j] : k0;
    uint32_t above = 0u;
    int d = kSelDigits - 1;
    for (; d > 0; --d) {
        const uint32_t c = s_bins[d * b + j];
        if (above + c >= k) break;
        above += c;
    }
    prefix[j] = ((pass > 0 ? prefix[j] : 0u) << 8) | (uint32_t)d;
    left[j] = k - above;
}

// ---------------------------------------------------------------- the maps
enum MapOp : int { kMapThreshold = 0, kMapAffine = 1, kMapRowSub = 2, kMapRowSweep = 3 };

struct MapShape {
    int64_t total;      // n * b elements
    int64_t quads;      // ceil(total / 4)
    int64_t stride_q;   // virtual lanes that take quads: a multiple of b
    int     b;
    int     vec;        // both slabs are 16-byte aligned: whole quads travel as one word
};

struct ColArgs {
    float a[kSlabMaxCols];      // threshold: the cuts; affine: what is taken off
    float d[kSlabMaxCols];      // affine: the divisors
};

template <int OP>
__global__ __launch_bounds__(kSlabBlock) void k_post_map(const float* __restrict__ m, float* __restrict__ out, MapShape s, ColArgs cols,
                                                         const float* __restrict__ v, float offset, int inclusive) {
    const int64_t lane = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x;
    if (lane >= s.stride_q) return;
    float a[4] = {0.f, 0.f, 0.f, 0.f}, d[4] = {1.f, 1.f, 1.f, 1.f};
    int64_t row[4];
    const int c0 = (int)((4 * lane) % s.b);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = (c0 + u) % s.b;
        if (OP == kMapThreshold || OP == kMapAffine) a[u] = cols.a[c];
        if (OP == kMapAffine) d[u] = cols.d[c];
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
        if (OP == kMapRowSub || OP == kMapRowSweep) {
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = e + u < s.total ? v[row[u]] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (OP == kMapThreshold) o[u] = (inclusive ? x[u] >= a[u] : x[u] > a[u]) ? 1.f : 0.f;
            if (OP == kMapAffine) o[u] = (x[u] - a[u]) / d[u];
            if (OP == kMapRowSub) o[u] = x[u] - r[u];
            if (OP == kMapRowSweep) {
                const float under = r[u] + offset;
                o[u] = x[u] / under;
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

// ---------------------------------------------------------------- [n, b] <-> [b, n], 64 rows a tile through LDS
constexpr int kTileRows = 64;

// TO_COLS: in is the row-major slab [n, b], out holds the columns one after the other [b, n]; otherwise the way back.  Both sides move
// runs of consecutive floats: rows * b of the slab, 64 of a column.
template <bool TO_COLS>
__global__ __launch_bounds__(kSlabBlock) void k_post_transpose(const float* __restrict__ in, float* __restrict__ out, int64_t n, int b) {
    __shared__ float tile[kTileRows][kSlabMaxCols + 1];
    const int64_t tiles = (n + kTileRows - 1) / kTileRows;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r0 = t * kTileRows;
        const int rows = (int)(n - r0 < kTileRows ? n - r0 : kTileRows);
        if (TO_COLS) {
            for (int e = threadIdx.x; e < rows * b; e += kSlabBlock) tile[e / b][e % b] = in[r0 * b + e];
        } else {
            for (int e = threadIdx.x; e < b * kTileRows; e += kSlabBlock) {
                const int c = e / kTileRows, r = e % kTileRows;
                if (r < rows) tile[r][c] = in[(int64_t)c * n + r0 + r];
            }
        }
        __syncthreads();
        if (TO_COLS) {
            for (int e = threadIdx.x; e < b * kTileRows; e += kSlabBlock) {
                const int c = e / kTileRows, r = e % kTileRows;
                if (r < rows) out[(int64_t)c * n + r0 + r] = tile[r][c];
            }
        } else {
            for (int e = threadIdx.x; e < rows * b; e += kSlabBlock) out[r0 * b + e] = tile[e / b][e % b];
        }
        __syncthreads();
    }
}

bool same_shape(pgh_mat_t a, pgh_mat_t b) { return a->n == b->n && a->b == b->b; }

// the checks every map shares; 0: launch, 1: nothing to do (no rows), else the status to return
int map_ready(const char* who, pgh_mat_t m, pgh_mat_t out, int* status) {
    if (!(m && out)) return *status = fail(std::string(who) + ": null argument"), -1;
    if (!(m->b >= 1 && m->n >= 0)) return *status = fail(std::string(who) + ": at least one column expected"), -1;
    if (!same_shape(m, out)) return *status = fail(std::string(who) + ": m and out differ in shape"), -1;
    if (m->b > kSlabMaxCols) return *status = declined(PGH_POST_DECLINED, who, "more than 64 columns"), -1;
    if (m->n == 0) return *status = 0, 1;
    if (out->data == m->data) return *status = fail(std::string(who) + ": out shares its memory with m"), -1;
    return 0;
}

template <int OP>
int launch_map(pgh_mat_t m, pgh_mat_t out, const ColArgs& cols, const float* v, float offset, int inclusive) {
    PGH_TRY(ensure_init());
    MapShape s;
    s.total = m->n * m->b;
    s.quads = (s.total + 3) / 4;
    const int grid = grid_capped(s.quads, kSlabBlock * 2);
    s.stride_q = ((int64_t)grid * kSlabBlock) / m->b * m->b;
    s.b = m->b;
    s.vec = aligned16(m->data) && aligned16(out->data) ? 1 : 0;
    k_post_map<OP><<<grid, kSlabBlock, 0, rt().stream>>>(m->data, out->data, s, cols, v, offset, inclusive);
    PGH_HIP(hipGetLastError());
    return 0;
}
}  // namespace

PGH_WARM_KERNEL(k_select_count)

extern "C" int pgh_post_kth_largest(pgh_mat_t m, int64_t k, double* values_host) {
    PGH_CHECK(m && values_host, "pgh_post_kth_largest: null argument");
    PGH_CHECK(m->b >= 1 && m->n >= 0, "pgh_post_kth_largest: at least one column expected");
    PGH_CHECK(m->n < 2147483648LL, "pgh_post_kth_largest: more than 2^31 - 1 rows");
    PGH_CHECK(k >= 1 && k <= m->n, "pgh_post_kth_largest: k outside [1, n]");
    const int b = m->b;
    if (b > kSlabMaxCols) return declined(PGH_POST_DECLINED, "pgh_post_kth_largest", "more than 64 columns");
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    SelShape s;
    s.total = m->n * b;
    s.b = b;
    s.W = kSlabMaxCols / b * b;
    int64_t want = (s.total + (int64_t)kSelBlock * kSelUnroll - 1) / ((int64_t)kSelBlock * kSelUnroll);
    const int64_t most = (int64_t)(r.num_cus > 0 ? r.num_cus : 1) * 2;      // what the LDS lets a CU hold
    const int grid = (int)(want < 1 ? 1 : (want > most ? most : want));
    s.stride = ((int64_t)grid * kSelBlock) / s.W * s.W;
    // [4][256][b] bins, the prefixes, the k left
    const size_t words = (size_t)kSelPasses * kSelDigits * b + 2 * (size_t)b;
    PoolBuf state;
    PGH_TRY(state.alloc(sizeof(uint32_t) * words));
    PGH_HIP(hipMemsetAsync(state.p, 0, sizeof(uint32_t) * words, r.stream));
    uint32_t* bins = state.as<uint32_t>();
    uint32_t* prefix = bins + (size_t)kSelPasses * kSelDigits * b;
    uint32_t* left = prefix + b;
    for (int pass = 0; pass < kSelPasses; ++pass) {
        uint32_t* mine = bins + (size_t)pass * kSelDigits * b;
        k_select_count<<<grid, kSelBlock, 0, r.stream>>>(m->data, s, pass, prefix, mine);
        PGH_HIP(hipGetLastError());
        k_select_pick<<<1, kSlabBlock, 0, r.stream>>>(mine, b, pass, (uint32_t)k, prefix, left);
        PGH_HIP(hipGetLastError());
    }
    uint32_t keys[kSlabMaxCols];
    PGH_HIP(hipMemcpyAsync(keys, prefix, sizeof(uint32_t) * (size_t)b, hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(hipStreamSynchronize(r.stream));
    for (int c = 0; c < b; ++c) values_host[c] = (double)value_of(keys[c]);
    return 0;
}

extern "C" int pgh_post_col_threshold(pgh_mat_t m, const double* cuts_host, int32_t inclusive, pgh_mat_t out) {
    int status = 0;
    if (map_ready("pgh_post_col_threshold", m, out, &status) != 0) return status;
    PGH_CHECK(cuts_host, "pgh_post_col_threshold: null argument");
    ColArgs cols;
    for (int c = 0; c < kSlabMaxCols; ++c) cols.a[c] = c < m->b ? (float)cuts_host[c] : 0.f, cols.d[c] = 1.f;
    return launch_map<kMapThreshold>(m, out, cols, nullptr, 0.f, inclusive != 0 ? 1 : 0);
}

extern "C" int pgh_post_col_affine(pgh_mat_t m, const double* sub_host, const double* div_host, pgh_mat_t out) {
    int status = 0;
    if (map_ready("pgh_post_col_affine", m, out, &status) != 0) return status;
    PGH_CHECK(sub_host && div_host, "pgh_post_col_affine: null argument");
    ColArgs cols;
    for (int c = 0; c < kSlabMaxCols; ++c) {
        const bool copy = c >= m->b || div_host[c] == 0.0;         // (x - 0) / 1 is x, bit for bit
        cols.a[c] = copy ? 0.f : (float)sub_host[c];
        cols.d[c] = copy ? 1.f : (float)div_host[c];
    }
    return launch_map<kMapAffine>(m, out, cols, nullptr, 0.f, 0);
}

extern "C" int pgh_post_row_op(pgh_mat_t m, pgh_vec_t v, int32_t op, double offset, pgh_mat_t out) {
    PGH_CHECK(v, "pgh_post_row_op: null argument");
    PGH_CHECK(op == PGH_POST_ROW_SUB || op == PGH_POST_ROW_SWEEP, "pgh_post_row_op: unknown op");
    PGH_CHECK(m == nullptr || v->n == m->n, "pgh_post_row_op: v does not have one entry per row");
    int status = 0;
    if (map_ready("pgh_post_row_op", m, out, &status) != 0) return status;
    ColArgs cols;
    for (int c = 0; c < kSlabMaxCols; ++c) cols.a[c] = 0.f, cols.d[c] = 1.f;
    if (op == PGH_POST_ROW_SUB) return launch_map<kMapRowSub>(m, out, cols, v->data, 0.f, 0);
    return launch_map<kMapRowSweep>(m, out, cols, v->data, (float)offset, 0);
}

extern "C" int pgh_post_ordinals(pgh_mat_t m, pgh_mat_t out) {
    int status = 0;
    if (map_ready("pgh_post_ordinals", m, out, &status) != 0) return status;
    PGH_CHECK(m->n < 2147483647LL, "pgh_post_ordinals: more than 2^31 - 2 rows");
    PGH_TRY(ensure_init());
    // One transposition lays the columns out one after the other, each goes through pgh_vec_ordinals itself -- the same sort, the same
    // ties --, one transposition brings the positions back: two slab passes instead of a strided pass out and in per column.
    Runtime& r = rt();
    const int64_t n = m->n;
    const int b = m->b;
    PoolBuf columns, places;
    PGH_TRY(columns.alloc(sizeof(float) * (size_t)n * b));
    PGH_TRY(places.alloc(sizeof(float) * (size_t)n * b));
    const int grid = grid_capped((n + kTileRows - 1) / kTileRows, 1);
    k_post_transpose<true><<<grid, kSlabBlock, 0, r.stream>>>(m->data, columns.as<float>(), n, b);
    PGH_HIP(hipGetLastError());
    pgh_vec_s x, y;
    x.n = y.n = n;
    x.owns = y.owns = false;
    for (int c = 0; c < b; ++c) {
        x.data = columns.as<float>() + (size_t)c * n;
        y.data = places.as<float>() + (size_t)c * n;
        PGH_TRY(pgh_vec_ordinals(&x, &y));
    }
    k_post_transpose<false><<<grid, kSlabBlock, 0, r.stream>>>(places.as<float>(), out->data, n, b);
    PGH_HIP(hipGetLastError());
    return 0;
}
