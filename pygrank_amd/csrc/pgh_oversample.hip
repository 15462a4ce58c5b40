// include/pgh_oversample.h: what lies between two runs of the base ranker in seed oversampling, for up to 64 seed sets at once.
//
// Reference counterpart: SeedOversampling.rank and BoostedSeedOversampling.rank / _boosting_weight
// (pygrank/algorithms/postprocess/oversampling.py:33-58, 95-127): a minimum over the seeds, a dictionary comprehension over the nodes and
// three sums per round and seed set, each one read per node on a device vector.
//
// Four streaming kernels over row-major [n, b] slabs and one fold, all on the engine's stream:
//   k_seed_floor     ranks, seeds  -> per column: min of the seeds' ranks, number of seeds
//   k_seed_resample  ranks (, keep) -> the 0 / 1 slab of the next seeds, per column: ones written
//   k_boost_forms    seeds, fresh, total -> per column: S1, S2, S3
//   k_boost_update   total += w[c] * fresh, then min / count of the new total over the mask's ones
//   k_fold_fields    the parts' partial results, in index order (pgh_slab.h)
// Work shape (the scheme of k_col_stats, pgh_measure.hip, on 16-byte words): the slab is a sequence of quads (four consecutive floats);
// virtual lane v < stride_q takes the quads v, v + stride_q, ... and stride_q is a multiple of b, so slot u of a lane stays on column
// (4 v + u) % b: four private accumulators per sum, no division in the loop.  A part is kSlabBlock consecutive virtual lanes, whatever the
// launch; the grid only decides which workgroup walks which parts.  Inside a part the 4 * kSlabBlock slots are folded per column through
// LDS -- G lanes per column take every G-th slot of that column in slot order, then a halving tree over the G -- and k_fold_fields adds
// the parts in index order: every order is fixed by (n, b) alone, so two calls return the same bits for every grid.  No atomics.
// The last quad of a slab whose n * b is not a multiple of four, and every quad of a slab that is not 16-byte aligned, go element by
// element under a bounds test.
// Per-column host arguments (floors, weights) reach the kernels through a pooled device buffer; a lane reads its four once.
// This file is compiled without contraction into fused multiply-adds (the pragma below), so that total + w * fresh is a rounded
// product and a rounded sum, as in a plain f64 evaluation.
#include "pgh_slab.h"
#include "pgh_oversample.h"

#include <cmath>
#include <cstring>

using namespace pgh;

#pragma clang fp contract(off)

namespace {
constexpr int kSlots = 4 * kSlabBlock;         // accumulator slots of a part
static_assert(PGH_OVERSAMPLE_MAX_COLS == kSlabMaxCols, "the per-column host arrays hold kSlabMaxCols entries");
// the fields of a part's partial result: a minimum or a sum, two sums, the 64-bit count
constexpr int kMinFirst = fold_kinds(kFoldMin, kFoldSum, kFoldSum, kFoldCount), kSumFirst = fold_kinds(kFoldSum, kFoldSum, kFoldSum, kFoldCount);

struct Shape {
    int64_t total;      // n * b elements
    int64_t quads;      // ceil(total / 4)
    int64_t stride_q;   // virtual lanes that take quads: kSlabParts * kSlabBlock rounded down to a multiple of b
    int     parts;      // parts that hold at least one quad
    int     b;
    int     vec;        // every operand is 16-byte aligned: whole quads travel as one word
};

__device__ __forceinline__ void load4(const float* p, int64_t e, const Shape& s, float (&v)[4]) {
    if (s.vec && e + 4 <= s.total) {
        const float4 w = *reinterpret_cast<const float4*>(p + e);
        v[0] = w.x;
        v[1] = w.y;
        v[2] = w.z;
        v[3] = w.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = e + u < s.total ? p[e + u] : 0.f;
    }
}

__device__ __forceinline__ void store4(float* p, int64_t e, const Shape& s, const float (&v)[4]) {
    if (s.vec && e + 4 <= s.total) {
        *reinterpret_cast<float4*>(p + e) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e + u < s.total) p[e + u] = v[u];
    }
}

// Folds the slots of part `part` per column and writes partial[part][column][0 .. 3] = the ND f64 fields (field 0 a minimum when MIN0,
// sums otherwise) and, in word 3, the 64-bit count (its bit pattern).  Every lane of the workgroup calls it.
template <int ND, bool MIN0, bool CNT>
__device__ __forceinline__ void fold_part(const double (&a)[4][ND > 0 ? ND : 1], const long long (&c)[4], int part, int b,
                                          double* __restrict__ partial, double* s_d /* [max(ND, 1)][kSlots] */, long long* s_c /* [kSlots] */) {
    const int t = threadIdx.x;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int f = 0; f < ND; ++f) s_d[f * kSlots + 4 * t + u] = a[u][f];
        if (CNT) s_c[4 * t + u] = c[u];
    }
    __syncthreads();
    int G = 1;
    while (2 * G * b <= kSlabBlock) G *= 2;                      // b <= 64: G >= 4
    const bool on = t < G * b;
    const int j = t % b, g = t / b;
    double r[ND > 0 ? ND : 1];
#pragma unroll
    for (int f = 0; f < ND; ++f) r[f] = (MIN0 && f == 0) ? INFINITY : 0.0;
    long long rc = 0;
    if (on) {
        // slot el of this part is element 4 * part * kSlabBlock + el of the lanes' first quads: its column is (4 * part * kSlabBlock + el) % b
        const int shift = (int)(((int64_t)4 * part * kSlabBlock) % b);
        const int start = ((j - shift) % b + b) % b;
        for (int el = start + g * b; el < kSlots; el += G * b) {
#pragma unroll
            for (int f = 0; f < ND; ++f) r[f] = (MIN0 && f == 0) ? fmin(r[f], s_d[f * kSlots + el]) : r[f] + s_d[f * kSlots + el];
            if (CNT) rc += s_c[el];
        }
    }
    __syncthreads();
    if (on) {
#pragma unroll
        for (int f = 0; f < ND; ++f) s_d[f * kSlots + t] = r[f];
        if (CNT) s_c[t] = rc;
    }
    __syncthreads();
    for (int h = G / 2; h >= 1; h >>= 1) {
        if (on && g < h) {
#pragma unroll
            for (int f = 0; f < ND; ++f) {
                const double x = s_d[f * kSlots + t], y = s_d[f * kSlots + t + h * b];
                s_d[f * kSlots + t] = (MIN0 && f == 0) ? fmin(x, y) : x + y;
            }
            if (CNT) s_c[t] += s_c[t + h * b];
        }
        __syncthreads();
    }
    if (t < b) {
        double* o = partial + ((int64_t)part * b + t) * 4;
#pragma unroll
        for (int f = 0; f < 3; ++f) o[f] = f < ND ? s_d[(f < ND ? f : 0) * kSlots + t] : 0.0;
        o[3] = __longlong_as_double(CNT ? s_c[t] : 0ll);
    }
    __syncthreads();
}

__global__ __launch_bounds__(kSlabBlock) void k_seed_floor(const float* __restrict__ ranks, const float* __restrict__ seeds, Shape s,
                                                            double* __restrict__ partial) {
    __shared__ double s_d[kSlots];
    __shared__ long long s_c[kSlots];
    for (int part = blockIdx.x; part < s.parts; part += gridDim.x) {
        double a[4][1] = {{INFINITY}, {INFINITY}, {INFINITY}, {INFINITY}};
        long long c[4] = {0, 0, 0, 0};
        const int64_t v = (int64_t)part * kSlabBlock + threadIdx.x;
        if (v < s.stride_q) {
            for (int64_t q = v; q < s.quads; q += s.stride_q) {
                float r[4], m[4];
                load4(ranks, 4 * q, s, r);
                load4(seeds, 4 * q, s, m);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool hit = m[u] == 1.f;            // (slots behind the slab's end were loaded as 0)
                    a[u][0] = hit ? fmin(a[u][0], (double)r[u]) : a[u][0];
                    c[u] += hit ? 1 : 0;
                }
            }
        }
        fold_part<1, true, true>(a, c, part, s.b, partial, s_d, s_c);
    }
}

// out may be keep: a quad is read, then written, by the one lane that owns it (no __restrict__ on either)
template <bool KEEP>
__global__ __launch_bounds__(kSlabBlock) void k_seed_resample(const float* ranks, const float* __restrict__ floors /* [b] */, int strict,
                                                               const float* keep, float* out, Shape s, double* __restrict__ partial) {
    __shared__ double s_d[kSlots];
    __shared__ long long s_c[kSlots];
    for (int part = blockIdx.x; part < s.parts; part += gridDim.x) {
        double a[4][1] = {{0.0}, {0.0}, {0.0}, {0.0}};
        long long c[4] = {0, 0, 0, 0};
        const int64_t v = (int64_t)part * kSlabBlock + threadIdx.x;
        if (v < s.stride_q) {
            float fl[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) fl[u] = floors[(4 * v + u) % s.b];
            for (int64_t q = v; q < s.quads; q += s.stride_q) {
                float r[4], k[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
                load4(ranks, 4 * q, s, r);
                if (KEEP) load4(keep, 4 * q, s, k);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool inside = 4 * q + u < s.total;
                    const bool reach = strict ? r[u] > fl[u] : r[u] >= fl[u];
                    const bool one = inside && (reach || (KEEP && k[u] == 1.f));
                    o[u] = one ? 1.f : 0.f;
                    c[u] += one ? 1 : 0;
                }
                store4(out, 4 * q, s, o);
            }
        }
        fold_part<0, false, true>(a, c, part, s.b, partial, s_d, s_c);
    }
}

__global__ __launch_bounds__(kSlabBlock) void k_boost_forms(const float* __restrict__ seeds, const float* __restrict__ fresh,
                                                             const float* __restrict__ total, Shape s, double* __restrict__ partial) {
    __shared__ double s_d[3 * kSlots];
    __shared__ long long s_c[1];
    for (int part = blockIdx.x; part < s.parts; part += gridDim.x) {
        double a[4][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        const long long c[4] = {0, 0, 0, 0};
        const int64_t v = (int64_t)part * kSlabBlock + threadIdx.x;
        if (v < s.stride_q) {
            for (int64_t q = v; q < s.quads; q += s.stride_q) {
                float m[4], r[4], t[4];
                load4(seeds, 4 * q, s, m);
                load4(fresh, 4 * q, s, r);
                load4(total, 4 * q, s, t);
#pragma unroll
                for (int u = 0; u < 4; ++u) {                // (slots behind the slab's end were loaded as 0: they add 0)
                    const double sd = (double)m[u], R = (double)r[u], RN = (double)t[u];
                    const double R2 = R * R;
                    a[u][0] += sd * R2;
                    a[u][1] += R2;
                    a[u][2] += (sd * RN) * R;
                }
            }
        }
        fold_part<3, false, false>(a, c, part, s.b, partial, s_d, s_c);
    }
}

__global__ __launch_bounds__(kSlabBlock) void k_boost_update(float* __restrict__ total, const float* __restrict__ fresh,
                                                              const double* __restrict__ weights /* [b] */, const float* __restrict__ mask, Shape s,
                                                              double* __restrict__ partial) {
    __shared__ double s_d[kSlots];
    __shared__ long long s_c[kSlots];
    for (int part = blockIdx.x; part < s.parts; part += gridDim.x) {
        double a[4][1] = {{INFINITY}, {INFINITY}, {INFINITY}, {INFINITY}};
        long long c[4] = {0, 0, 0, 0};
        const int64_t v = (int64_t)part * kSlabBlock + threadIdx.x;
        if (v < s.stride_q) {
            double w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) w[u] = weights[(4 * v + u) % s.b];
            for (int64_t q = v; q < s.quads; q += s.stride_q) {
                float t[4], r[4], m[4], o[4];
                load4(total, 4 * q, s, t);
                load4(fresh, 4 * q, s, r);
                load4(mask, 4 * q, s, m);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    o[u] = (float)((double)t[u] + w[u] * (double)r[u]);
                    const bool hit = m[u] == 1.f;
                    a[u][0] = hit ? fmin(a[u][0], (double)o[u]) : a[u][0];
                    c[u] += hit ? 1 : 0;
                }
                store4(total, 4 * q, s, o);
            }
        }
        fold_part<1, true, true>(a, c, part, s.b, partial, s_d, s_c);
    }
}

Shape shape_of(int64_t n, int b, bool vec) {
    Shape s;
    s.total = n * b;
    s.quads = (s.total + 3) / 4;
    s.stride_q = ((int64_t)kSlabParts * kSlabBlock) / b * b;
    const int64_t lanes = s.quads < s.stride_q ? s.quads : s.stride_q;
    s.parts = (int)((lanes + kSlabBlock - 1) / kSlabBlock);
    s.b = b;
    s.vec = vec ? 1 : 0;
    return s;
}

int64_t count_of(double word) {
    int64_t c;
    std::memcpy(&c, &word, sizeof c);
    return c;
}

bool same_shape(pgh_mat_t a, pgh_mat_t b) { return a->n == b->n && a->b == b->b; }
}  // namespace

PGH_WARM_KERNEL(k_seed_floor)

extern "C" int pgh_seed_floor(pgh_mat_t ranks, pgh_mat_t seeds, double* floor_host, int64_t* count_host) {
    PGH_CHECK(ranks && seeds && floor_host && count_host, "pgh_seed_floor: null argument");
    PGH_CHECK(ranks->b >= 1 && ranks->n >= 0, "pgh_seed_floor: at least one column expected");
    PGH_CHECK(same_shape(ranks, seeds), "pgh_seed_floor: ranks and seeds differ in shape");
    const int b = ranks->b;
    if (b > kSlabMaxCols) return declined(PGH_OVERSAMPLE_DECLINED, "pgh_seed_floor", "more than 64 columns");
    if (ranks->n == 0) {
        for (int c = 0; c < b; ++c) {
            floor_host[c] = INFINITY;
            count_host[c] = 0;
        }
        return 0;
    }
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const Shape s = shape_of(ranks->n, b, aligned16(ranks->data) && aligned16(seeds->data));
    PoolBuf partial;
    PGH_TRY(partial.alloc(sizeof(double) * (size_t)s.parts * b * 4));
    k_seed_floor<<<parts_grid(s.parts), kSlabBlock, 0, r.stream>>>(ranks->data, seeds->data, s, partial.as<double>());
    PGH_HIP(hipGetLastError());
    double result[4 * kSlabMaxCols];
    PGH_TRY(fold_fields_to_host<kMinFirst>(partial.as<double>(), s.parts, s.b, s.b, result));
    for (int c = 0; c < b; ++c) {
        floor_host[c] = result[4 * c];
        count_host[c] = count_of(result[4 * c + 3]);
    }
    return 0;
}

extern "C" int pgh_seed_resample(pgh_mat_t ranks, const double* floor_host, int32_t strict, pgh_mat_t keep, pgh_mat_t out,
                                 int64_t* count_host) {
    PGH_CHECK(ranks && floor_host && out && count_host, "pgh_seed_resample: null argument");
    PGH_CHECK(ranks->b >= 1 && ranks->n >= 0, "pgh_seed_resample: at least one column expected");
    PGH_CHECK(same_shape(ranks, out) && (keep == nullptr || same_shape(ranks, keep)), "pgh_seed_resample: the slabs differ in shape");
    PGH_CHECK(ranks->n == 0 || out->data != ranks->data, "pgh_seed_resample: out shares its memory with ranks");
    const int b = ranks->b;
    if (b > kSlabMaxCols) return declined(PGH_OVERSAMPLE_DECLINED, "pgh_seed_resample", "more than 64 columns");
    float floors[kSlabMaxCols];
    for (int c = 0; c < b; ++c) {
        if (!std::isfinite(floor_host[c])) return declined(PGH_OVERSAMPLE_DECLINED, "pgh_seed_resample", "a floor is not finite");
        floors[c] = (float)floor_host[c];
    }
    if (ranks->n == 0) {
        for (int c = 0; c < b; ++c) count_host[c] = 0;
        return 0;
    }
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const Shape s = shape_of(ranks->n, b, aligned16(ranks->data) && aligned16(out->data) && (keep == nullptr || aligned16(keep->data)));
    PoolBuf partial, d_floors;
    PGH_TRY(partial.alloc(sizeof(double) * (size_t)s.parts * b * 4));
    PGH_TRY(d_floors.alloc(sizeof(float) * (size_t)b));
    StreamFence fence;                                       // the staged floors go away with this frame
    PGH_HIP(hipMemcpyAsync(d_floors.p, floors, sizeof(float) * (size_t)b, hipMemcpyHostToDevice, r.stream));
    const int grid = parts_grid(s.parts), strictly = strict != 0 ? 1 : 0;
    if (keep != nullptr)
        k_seed_resample<true><<<grid, kSlabBlock, 0, r.stream>>>(ranks->data, d_floors.as<float>(), strictly, keep->data, out->data, s, partial.as<double>());
    else
        k_seed_resample<false><<<grid, kSlabBlock, 0, r.stream>>>(ranks->data, d_floors.as<float>(), strictly, ranks->data, out->data, s, partial.as<double>());
    PGH_HIP(hipGetLastError());
    double result[4 * kSlabMaxCols];
    PGH_TRY(fold_fields_to_host<kSumFirst>(partial.as<double>(), s.parts, s.b, s.b, result));
    fence.passed = true;                                     // (the fold waited)
    for (int c = 0; c < b; ++c) count_host[c] = count_of(result[4 * c + 3]);
    return 0;
}

extern "C" int pgh_boost_forms(pgh_mat_t seeds, pgh_mat_t fresh, pgh_mat_t total, double* forms_host) {
    PGH_CHECK(seeds && fresh && total && forms_host, "pgh_boost_forms: null argument");
    PGH_CHECK(seeds->b >= 1 && seeds->n >= 0, "pgh_boost_forms: at least one column expected");
    PGH_CHECK(same_shape(seeds, fresh) && same_shape(seeds, total), "pgh_boost_forms: the slabs differ in shape");
    const int b = seeds->b;
    if (b > kSlabMaxCols) return declined(PGH_OVERSAMPLE_DECLINED, "pgh_boost_forms", "more than 64 columns");
    if (seeds->n == 0) {
        for (int k = 0; k < 3 * b; ++k) forms_host[k] = 0.0;
        return 0;
    }
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const Shape s = shape_of(seeds->n, b, aligned16(seeds->data) && aligned16(fresh->data) && aligned16(total->data));
    PoolBuf partial;
    PGH_TRY(partial.alloc(sizeof(double) * (size_t)s.parts * b * 4));
    k_boost_forms<<<parts_grid(s.parts), kSlabBlock, 0, r.stream>>>(seeds->data, fresh->data, total->data, s, partial.as<double>());
    PGH_HIP(hipGetLastError());
    double result[4 * kSlabMaxCols];
    PGH_TRY(fold_fields_to_host<kSumFirst>(partial.as<double>(), s.parts, s.b, s.b, result));
    for (int c = 0; c < b; ++c)
        for (int f = 0; f < 3; ++f) forms_host[3 * c + f] = result[4 * c + f];
    return 0;
}

extern "C" int pgh_boost_update(pgh_mat_t total, pgh_mat_t fresh, const double* weights_host, pgh_mat_t mask, double* floor_host,
                                int64_t* count_host) {
    PGH_CHECK(total && fresh && weights_host && mask && floor_host && count_host, "pgh_boost_update: null argument");
    PGH_CHECK(total->b >= 1 && total->n >= 0, "pgh_boost_update: at least one column expected");
    PGH_CHECK(same_shape(total, fresh) && same_shape(total, mask), "pgh_boost_update: the slabs differ in shape");
    PGH_CHECK(total->n == 0 || (total->data != fresh->data && total->data != mask->data),
              "pgh_boost_update: total shares its memory with fresh or mask");
    const int b = total->b;
    if (b > kSlabMaxCols) return declined(PGH_OVERSAMPLE_DECLINED, "pgh_boost_update", "more than 64 columns");
    for (int c = 0; c < b; ++c)
        if (!std::isfinite(weights_host[c])) return declined(PGH_OVERSAMPLE_DECLINED, "pgh_boost_update", "a weight is not finite");
    if (total->n == 0) {
        for (int c = 0; c < b; ++c) {
            floor_host[c] = INFINITY;
            count_host[c] = 0;
        }
        return 0;
    }
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const Shape s = shape_of(total->n, b, aligned16(total->data) && aligned16(fresh->data) && aligned16(mask->data));
    PoolBuf partial, d_weights;
    PGH_TRY(partial.alloc(sizeof(double) * (size_t)s.parts * b * 4));
    PGH_TRY(d_weights.alloc(sizeof(double) * (size_t)b));
    StreamFence fence;                                       // the caller's weights may go away
    PGH_HIP(hipMemcpyAsync(d_weights.p, weights_host, sizeof(double) * (size_t)b, hipMemcpyHostToDevice, r.stream));
    k_boost_update<<<parts_grid(s.parts), kSlabBlock, 0, r.stream>>>(total->data, fresh->data, d_weights.as<double>(), mask->data, s, partial.as<double>());
    PGH_HIP(hipGetLastError());
    double result[4 * kSlabMaxCols];
    PGH_TRY(fold_fields_to_host<kMinFirst>(partial.as<double>(), s.parts, s.b, s.b, result));
    fence.passed = true;                                     // (the fold waited)
    for (int c = 0; c < b; ++c) {
        floor_host[c] = result[4 * c];
        count_host[c] = count_of(result[4 * c + 3]);
    }
    return 0;
}
