// The f64 siblings of the multi-seed loops (include/pgh_batch64.h): Y = M^T X and the device loops of PageRank, the two absorbing
// walks and the closed-form filters' taylor form over [n, ld] slabs of DOUBLES, b <= 64 columns.
//
// They walk the multi-seed stream the f32 loops walk (pgh_spmm.hip ensure_mm_layout: colf, val, close, tile, seg_row, perm): no image
// is built for them.  A group of lanes walks one 512-entry tile and a lane owns TWO columns, so one 16-byte load per lane fetches a
// gathered row: 32 / 16 / 8 / 4 lanes per row for ld <= 64 / 32 / 16 / 8.  The stream words of a round are loaded by the group's lanes
// and handed round with ds_bpermute; `val` and the image's f32 row and source scales are widened to double where they are used.  Row
// sums are stored as doubles, the cross-tile carries are doubles combined in tile order by k_mm64_fixup.
//
// A step of a loop is: product, fix-up, step (epilogue + the next gather slab + per-workgroup partial sums of y), fold, residual (it
// reads the new quotient from the fold's words), fold, close.  Every fold is per column and in a fixed order, nothing adds atomically:
// two calls return the same bits.  Behind a stop every kernel returns at once, and the host drives the loop through the run-ahead
// protocol of the f32 loops (pgh_mm_run.h).  The f32 loops' sparse gate, row-flag skipping and in-kernel residual prediction have
// no counterpart here: every row is processed in every step.
#include "pgh_kernels.h"
#include "pgh_batch64.h"
#include "pgh_mm_run.h"

#include <cmath>

using namespace pgh;

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
constexpr int kTile64 = 64 * PGH_BSF_IPT;        // the tile table of the multi-seed layout

// lanes that move one row of an [n, ld] slab of doubles as 16-byte pairs
__host__ __device__ inline int lanes_per_row64(int ld) { return ld <= 8 ? 4 : (ld <= 16 ? 8 : (ld <= 32 ? 16 : 32)); }

struct MM64View {
    const uint32_t* colf;
    const float*    val;         // or null (value-free stream)
    const int32_t*  seg_row;
    const int32_t*  close;       // [num_entries] closing row of every entry (pgh_spmm.hip k_mm_close_rows)
    const int4*     tile;
    double*         head;        // [num_tiles + 1][ld]
    double*         tail;        // [num_tiles + 1][ld]
    int             num_tiles;
};

// per column: 1 / |p_j| (recursive loops), c_1 (closed form), or 1; kernel arguments
struct ColFactors {
    double v[kLanes];
};

// the row operands of a step in the multi-seed id space: y = a_j * U * (row sum) + V * p, the next gather row = y * G
struct RowOp64 {
    double U, V, G, pad;
};

// mode 0: PageRank (U = alpha * dst scale, V = 1 - alpha); 1: AbsorbingWalks with lam; 2: SymmetricAbsorbingRandomWalks (lam and the
// source factor 1 / lam from the degrees, as k_bsf64_walk_operands forms them); 3: the plain product (U = dst scale, V = 0).
// Padding rows: U = V = 0.  A real row whose weights are not finite (lam + deg == 0) sets *bad (every writer stores the same 1).
__global__ __launch_bounds__(WG) void k_mm64_rowops(int mode, double alpha, const float* __restrict__ dst_scale, const float* __restrict__ src_scale,
                                                     const float* __restrict__ degrees, const float* __restrict__ lam,
                                                     const int32_t* __restrict__ perm, int64_t n_int, int64_t n_valid, RowOp64* __restrict__ out,
                                                     int* __restrict__ bad) {
    for (int64_t r = blockIdx.x * (int64_t)WG + threadIdx.x; r < n_int; r += (int64_t)gridDim.x * WG) {
        const int64_t o = perm ? perm[r] : (r < n_valid ? r : -1);
        const double ds = dst_scale != nullptr ? (double)dst_scale[r] : 1.0;
        const double ss = src_scale != nullptr ? (double)src_scale[r] : 1.0;
        RowOp64 w{0.0, 0.0, ss, 0.0};
        if (o >= 0) {
            if (mode == 0) {
                w.U = alpha * ds;
                w.V = 1.0 - alpha;
            } else if (mode == 3) {
                w.U = ds;
            } else {
                const double d = (double)degrees[o];
                const double l = mode == 1 ? (double)lam[o] : (sqrt(d * 4.0 + 1.0) + 1.0) / 2.0;
                w.U = ds * (d / (l + d));
                w.V = l / (l + d);
                if (mode == 2) w.G = ss * (1.0 / l);
                if (!(isfinite(w.U) && isfinite(w.V) && isfinite(w.G))) *bad = 1;
            }
        }
        out[r] = w;
    }
}

// The product pass: sums[row] <- the row's sum of val * xg[source] over the stream, per column, in f64.  LPR lanes walk one tile, a lane
// holds the columns 2 l and 2 l + 1.  A round is R = max(16, LPR) entries: lane l of the group loads the words of the entries
// l * W .. l * W + W - 1 (W = R / LPR) and entry e of the round is word e % W of lane e / W.  Stream words travel two rounds ahead of
// the gathers, rows are gathered eight entries ahead of the sums that consume them (two register sets).
template <bool HAS_VAL, int LPR>
__global__ __launch_bounds__(WG) void k_mm64_partial(MM64View f, const double* __restrict__ xg, int ld, double* __restrict__ sums,
                                                      const BatchState* __restrict__ state) {
    if (state != nullptr && state->all_done) return;
    constexpr int G = 64 / LPR;                            // tiles in flight per wavefront
    constexpr int R = LPR > 16 ? LPR : 16;                 // entries per round
    constexpr int W = R / LPR;                             // stream words of a round per lane
    constexpr int C = R / 8;                               // chunks of eight entries per round (even)
    constexpr int ROUNDS = kTile64 / R;
    static_assert(kTile64 % R == 0 && C % 2 == 0, "a tile is whole rounds, a round is pairs of chunks");
    const int lane = threadIdx.x & 63;
    const int l = lane & (LPR - 1);
    const int c2 = 2 * l;
    const int pull = (lane & ~(LPR - 1)) << 2;             // ds_bpermute byte index of lane 0 of this group
    const bool live = c2 < ld;
    const int cl = live ? c2 : 0;                          // (a lane beyond the row re-reads the group's first pair: no load under a branch)
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (WG / 64) + (threadIdx.x >> 6)));
    const int stride = gridDim.x * (WG / 64) * G;
    struct Words {
        uint32_t w[W];
        int      c[W];
        float    v[W];
    };
    for (int t0 = wave * G; t0 < f.num_tiles; t0 += stride) {
        const int t = t0 + lane / LPR;
        const bool has = t < f.num_tiles;
        const int64_t base = (int64_t)(has ? t : f.num_tiles - 1) * kTile64;      // tiles are full and consecutive
        auto words = [&](int first, Words& q) __attribute__((always_inline)) {
            const int64_t at = base + first + l * W;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                q.w[k] = __builtin_nontemporal_load(f.colf + at + k);
                const int cw = __builtin_nontemporal_load(f.close + at + k);      // (the tile index is clamped: unconditional, then a select)
                q.c[k] = has ? cw : -1;
                q.v[k] = HAS_VAL ? __builtin_nontemporal_load(f.val + at + k) : 1.f;
            }
        };
        auto gather = [&](const Words& q, int chunk, f64x2 (&x)[8]) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int e = 8 * chunk + j;
                const uint32_t word = (uint32_t)__builtin_amdgcn_ds_bpermute(pull + 4 * (e / W), (int)q.w[e % W]);
                const uint32_t src = word & 0x7fffffffu;
                x[j] = *reinterpret_cast<const f64x2*>(xg + (int64_t)src * ld + cl);
            }
        };
        double a0 = 0.0, a1 = 0.0;
        auto consume = [&](const Words& q, int chunk, const f64x2 (&x)[8]) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int e = 8 * chunk + j;
                const int ends = __builtin_amdgcn_ds_bpermute(pull + 4 * (e / W), q.c[e % W]);
                if (HAS_VAL) {
                    const double v = (double)__int_as_float(__builtin_amdgcn_ds_bpermute(pull + 4 * (e / W), __float_as_int(q.v[e % W])));
                    a0 += v * x[j].x;
                    a1 += v * x[j].y;
                } else {
                    a0 += x[j].x;
                    a1 += x[j].y;
                }
                if (ends != -1) {                          // uniform inside a group
                    if (live) {
                        const f64x2 s = {a0, a1};
                        if (ends == -2) *reinterpret_cast<f64x2*>(f.head + (int64_t)t * ld + c2) = s;
                        else __builtin_nontemporal_store(s, reinterpret_cast<f64x2*>(sums + (int64_t)ends * ld + c2));
                    }
                    a0 = a1 = 0.0;
                }
            }
        };
        Words w0, w1, w2;
        f64x2 xa[8], xb[8];
        words(0, w0);
        words(R < kTile64 ? R : 0, w1);
        gather(w0, 0, xa);
        for (int r = 0; r < ROUNDS; ++r) {
            const int ahead = R * (r + 2);
            words(ahead <= kTile64 - R ? ahead : kTile64 - R, w2);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                f64x2 (&now)[8] = (c & 1) ? xb : xa;
                f64x2 (&next)[8] = (c & 1) ? xa : xb;
                if (c + 1 < C) gather(w0, c + 1, next);
                else if (r + 1 < ROUNDS) gather(w1, 0, next);
                consume(w0, c, now);
            }
            w0 = w1;
            w1 = w2;
        }
        if (has && live) *reinterpret_cast<f64x2*>(f.tail + (int64_t)t * ld + c2) = f64x2{a0, a1};
    }
}

// cross-tile segments: the chain of tail carries + the head piece, added in tile order.  A group of lanes_per_row64(ld) lanes per
// closing tile; eight carries of a hub row's chain travel together.
__global__ __launch_bounds__(WG) void k_mm64_fixup(MM64View f, int ld, double* __restrict__ sums, const BatchState* __restrict__ state) {
    if (state != nullptr && state->all_done) return;
    const int lpr = lanes_per_row64(ld), per_wave = 64 / lpr;
    const int lane = threadIdx.x & 63, l = lane & (lpr - 1), c2 = 2 * l;
    if (c2 >= ld) return;
    const int first = (blockIdx.x * (WG / 64) + (threadIdx.x >> 6)) * per_wave + lane / lpr;
    const int stride = gridDim.x * (WG / 64) * per_wave;
    for (int t = first; t < f.num_tiles; t += stride) {
        const int4 ti = f.tile[t];
        const int row = (ti.w >= 0 && ti.z >= 0) ? f.seg_row[ti.z] : -1;
        if (row < 0) continue;
        double a0 = 0.0, a1 = 0.0;
        int s = ti.w;
        constexpr int UC = 8;
        for (; s + UC <= t; s += UC) {
            f64x2 v[UC];
#pragma unroll
            for (int k = 0; k < UC; ++k) v[k] = *reinterpret_cast<const f64x2*>(f.tail + (int64_t)(s + k) * ld + c2);
#pragma unroll
            for (int k = 0; k < UC; ++k) {
                a0 += v[k].x;
                a1 += v[k].y;
            }
        }
        for (; s < t; ++s) {
            const f64x2 v = *reinterpret_cast<const f64x2*>(f.tail + (int64_t)s * ld + c2);
            a0 += v.x;
            a1 += v.y;
        }
        const f64x2 h = *reinterpret_cast<const f64x2*>(f.head + (int64_t)t * ld + c2);
        a0 += h.x;
        a1 += h.y;
        *reinterpret_cast<f64x2*>(sums + (int64_t)row * ld + c2) = f64x2{a0, a1};
    }
}

// the caller's [n, b] slab (f32 or f64, caller ids) into the id space of the image, as doubles; holes and the columns b .. ld - 1 are
// zero.  out_scaled (or null) <- value * factor of its column; out_raw (or null) <- value; out_xg <- value * G of the row.
template <typename T>
__global__ __launch_bounds__(WG) void k_mm64_way_in(const T* __restrict__ src, const int32_t* __restrict__ perm, int64_t n_int, int64_t n_valid, int b,
                                                     int ld, ColFactors factors, const RowOp64* __restrict__ rowop, double* __restrict__ out_scaled,
                                                     double* __restrict__ out_raw, double* __restrict__ out_xg) {
    const int lpr = lanes_per_row64(ld), rows_per_wave = 64 / lpr;
    const int lane = threadIdx.x & 63, l = lane & (lpr - 1), c2 = 2 * l;
    if (c2 >= ld) return;
    const double f0 = factors.v[c2], f1 = factors.v[c2 + 1];
    const int64_t first = (blockIdx.x * (int64_t)(WG / 64) + (threadIdx.x >> 6)) * rows_per_wave + lane / lpr;
    const int64_t stride = (int64_t)gridDim.x * (WG / 64) * rows_per_wave;
    for (int64_t r = first; r < n_int; r += stride) {
        const int64_t o = perm ? perm[r] : (r < n_valid ? r : -1);
        double v0 = 0.0, v1 = 0.0;
        if (o >= 0) {
            if (c2 < b) v0 = (double)src[o * b + c2];
            if (c2 + 1 < b) v1 = (double)src[o * b + c2 + 1];
        }
        const int64_t at = r * ld + c2;
        if (out_scaled != nullptr) *reinterpret_cast<f64x2*>(out_scaled + at) = f64x2{v0 * f0, v1 * f1};
        if (out_raw != nullptr) *reinterpret_cast<f64x2*>(out_raw + at) = f64x2{v0, v1};
        const double g = rowop[r].G;
        *reinterpret_cast<f64x2*>(out_xg + at) = f64x2{v0 * g, v1 * g};
    }
}

// the way out: dst[caller id] = (T)(slab value [* U of the row] * column factor): one rounding to T
template <typename T>
__global__ __launch_bounds__(WG) void k_mm64_way_out(const double* __restrict__ slab, const RowOp64* __restrict__ rowop_u, const int32_t* __restrict__ perm,
                                                      int64_t n_int, int64_t n_valid, int b, int ld, ColFactors factors, T* __restrict__ dst) {
    const int lpr = lanes_per_row64(ld), rows_per_wave = 64 / lpr;
    const int lane = threadIdx.x & 63, l = lane & (lpr - 1), c2 = 2 * l;
    if (c2 >= b) return;
    const double f0 = factors.v[c2], f1 = factors.v[c2 + 1];
    const int64_t first = (blockIdx.x * (int64_t)(WG / 64) + (threadIdx.x >> 6)) * rows_per_wave + lane / lpr;
    const int64_t stride = (int64_t)gridDim.x * (WG / 64) * rows_per_wave;
    for (int64_t r = first; r < n_int; r += stride) {
        const int64_t o = perm ? perm[r] : (r < n_valid ? r : -1);
        if (o < 0) continue;
        f64x2 v = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(slab + r * ld + c2));
        if (rowop_u != nullptr) v *= rowop_u[r].U;
        dst[o * b + c2] = (T)(v.x * f0);
        if (c2 + 1 < b) dst[o * b + c2 + 1] = (T)(v.y * f1);
    }
}

// the lane groups of a wavefront hold the same columns: fold them in group order, then the wavefronts in wavefront order, and leave
// the workgroup's value of every column in partials[blockIdx.x][64] (columns beyond the slab: 0)
__device__ __forceinline__ void mm64_block_fold(double t0, double t1, int lpr, int c2, bool in_slab, int linf, double (*s_red)[kLanes],
                                                double* __restrict__ partials) {
    const int lane = threadIdx.x & 63, wave_in_wg = threadIdx.x >> 6;
    double u0 = t0, u1 = t1;
    for (int off = lpr; off < 64; off += lpr) {
        const double o0 = __shfl_down(t0, off, 64), o1 = __shfl_down(t1, off, 64);
        u0 = linf ? fmax(u0, o0) : u0 + o0;
        u1 = linf ? fmax(u1, o1) : u1 + o1;
    }
    for (int j = threadIdx.x; j < (WG / 64) * kLanes; j += WG) (&s_red[0][0])[j] = 0.0;
    __syncthreads();
    if (lane < lpr && in_slab) {
        s_red[wave_in_wg][c2] = u0;
        s_red[wave_in_wg][c2 + 1] = u1;
    }
    __syncthreads();
    if (wave_in_wg == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < WG / 64; ++w) t = linf ? fmax(t, s_red[w][lane]) : t + s_red[w][lane];
        partials[(int64_t)blockIdx.x * kLanes + lane] = t;
    }
}

// One step of every column of a recursive filter: y = a_j * U_r * sum + V_r * p with a_j the column's quotient (the state's scale),
// the next gather row y * G_r, and the workgroup's partial sums of y per column.  A stopped column's row is copied forward.
__global__ __launch_bounds__(WG) void k_mm64_step(const double* __restrict__ sums, const RowOp64* __restrict__ rowop, const double* __restrict__ p,
                                                   const double* __restrict__ y_old, double* __restrict__ y_new, double* __restrict__ xg, int64_t n,
                                                   int ld, int b, const BatchState* __restrict__ state, double* __restrict__ partials) {
    __shared__ double s_red[WG / 64][kLanes];
    if (state->all_done) return;
    const int lane = threadIdx.x & 63;
    const int lpr = lanes_per_row64(ld), rows_per_wave = 64 / lpr;
    const int l = lane & (lpr - 1), c2 = 2 * l;
    const bool live = c2 < ld;
    double a[2];
    bool frozen[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const bool col = c2 + k < b;
        a[k] = col ? state->scale[c2 + k] : 0.0;
        frozen[k] = !col || state->done[c2 + k] != 0;
    }
    double S0 = 0.0, S1 = 0.0;
    const int64_t first = (blockIdx.x * (int64_t)(WG / 64) + (threadIdx.x >> 6)) * rows_per_wave + lane / lpr;
    const int64_t stride = (int64_t)gridDim.x * (WG / 64) * rows_per_wave;
    constexpr int U = 2;
    for (int64_t r0 = first; live && r0 < n; r0 += stride * U) {
        f64x2 sum[U], pv[U], yo[U];
        RowOp64 op[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = r0 + u * stride;
            ok[u] = r < n;
            const int64_t at = (ok[u] ? r : 0) * ld + c2;
            sum[u] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(sums + at));
            pv[u] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(p + at));
            yo[u] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(y_old + at));
            op[u] = rowop[ok[u] ? r : 0];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            const int64_t at = (r0 + u * stride) * ld + c2;
            f64x2 y;
            y.x = frozen[0] ? yo[u].x : a[0] * (sum[u].x * op[u].U) + op[u].V * pv[u].x;
            y.y = frozen[1] ? yo[u].y : a[1] * (sum[u].y * op[u].U) + op[u].V * pv[u].y;
            *reinterpret_cast<f64x2*>(y_new + at) = y;
            *reinterpret_cast<f64x2*>(xg + at) = y * op[u].G;
            S0 += y.x;
            S1 += y.y;
        }
    }
    mm64_block_fold(S0, S1, lpr, c2, live, 0, s_red, partials);
}

// the residual of a step per column: sum (or max) over the rows of |y_new * s_new - y_old * s_old|, s_new = 1 / (the folded sum of
// y_new) read from the device (1 without the quotient), s_old = the state's scale.  y_old == null: |y_new| (a closed-form run's first term).
__global__ __launch_bounds__(WG) void k_mm64_residual(const double* __restrict__ y_new, const double* __restrict__ y_old, int64_t n, int ld, int b,
                                                       int use_quotient, int linf, const BatchState* __restrict__ state,
                                                       const double* __restrict__ folded_sum, double* __restrict__ partials) {
    __shared__ double s_red[WG / 64][kLanes];
    if (state->all_done) return;
    const int lane = threadIdx.x & 63;
    const int lpr = lanes_per_row64(ld), rows_per_wave = 64 / lpr;
    const int l = lane & (lpr - 1), c2 = 2 * l;
    const bool live = c2 < ld;
    double inv[2], scale[2], acc[2] = {0.0, 0.0};
    bool want[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const bool col = c2 + k < b;
        const double S = (col && use_quotient) ? folded_sum[c2 + k] : 1.0;
        inv[k] = use_quotient ? (S != 0.0 ? 1.0 / S : 0.0) : 1.0;
        scale[k] = col ? state->scale[c2 + k] : 1.0;
        want[k] = col && !state->done[c2 + k];
    }
    const int64_t first = (blockIdx.x * (int64_t)(WG / 64) + (threadIdx.x >> 6)) * rows_per_wave + lane / lpr;
    const int64_t stride = (int64_t)gridDim.x * (WG / 64) * rows_per_wave;
    constexpr int U = 4;
    for (int64_t r0 = first; live && (want[0] || want[1]) && r0 < n; r0 += stride * U) {
        f64x2 yn[U], yo[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = r0 + u * stride;
            ok[u] = r < n;
            const int64_t at = (ok[u] ? r : 0) * ld + c2;
            yn[u] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(y_new + at));
            yo[u] = y_old != nullptr ? __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(y_old + at)) : f64x2{0.0, 0.0};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            const double d0 = fabs(yn[u].x * inv[0] - yo[u].x * scale[0]), d1 = fabs(yn[u].y * inv[1] - yo[u].y * scale[1]);
            acc[0] = linf ? fmax(acc[0], d0) : acc[0] + d0;
            acc[1] = linf ? fmax(acc[1], d1) : acc[1] + d1;
        }
    }
    mm64_block_fold(want[0] ? acc[0] : 0.0, want[1] ? acc[1] : 0.0, lpr, c2, live, linf, s_red, partials);
}

// per-column fold of [count][64] workgroup partials (sum or max): one workgroup per column, thread t takes the rows t, t + 256, ...,
// then the lanes and the four wavefronts are combined in a fixed order
__global__ __launch_bounds__(WG) void k_mm64_fold(const double* __restrict__ partials, int count, int linf, const BatchState* __restrict__ state,
                                                   double* __restrict__ out) {
    __shared__ double s_red[WG / 64];
    if (state != nullptr && state->all_done) return;
    const int col = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += WG) {
        const double v = partials[(int64_t)i * kLanes + col];
        acc = linf ? fmax(acc, v) : acc + v;
    }
    acc = linf ? wave_reduce_max(acc) : wave_reduce_sum(acc);
    if (lane == 0) s_red[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = s_red[0];
#pragma unroll
        for (int k = 1; k < WG / 64; ++k) t = linf ? fmax(t, s_red[k]) : t + s_red[k];
        out[col] = t;
    }
}

// closes a step: per live column the new quotient, the step count and ConvergenceManager's check (convergence.py:96-101)
struct Close64 {
    double    tol;
    long long n_orig;
    int       use_quotient, check, err_kind;
};
__global__ void k_mm64_close(BatchState* __restrict__ state, const double* __restrict__ folded_sum, const double* __restrict__ folded_err, Close64 cp) {
    const int lane = threadIdx.x;
    if (state->all_done) return;
    int done = 1;
    if (lane < state->b && !state->done[lane]) {
        if (cp.use_quotient) {
            const double S = folded_sum[lane];
            state->scale[lane] = S != 0.0 ? 1.0 / S : 0.0;
            state->sum[lane] = S;
        } else {
            state->scale[lane] = 1.0;                      // (the start quotient 1 / |p| is spent after the first step)
        }
        state->steps[lane] += 1;
        if (cp.check) {
            double err = folded_err[lane];
            if (cp.err_kind == PGH_ERR_MABS) err /= (double)cp.n_orig;
            state->err[lane] = err;
            if (err <= cp.tol) {
                state->done[lane] = 1;
                state->converged[lane] = 1;
            }
        }
        done = state->done[lane];
    }
    const unsigned long long all = __ballot(done != 0);
    if (lane == 0) {
        state->all_done = (all == ~0ULL) ? 1 : 0;
        state->executed += 1;
    }
}

// use_scale0: scale0 holds the start quotient of every column (1 / |p_j|; 0 marks a zero column: done from the start); otherwise 1
__global__ void k_mm64_state_init(BatchState* state, int b, ColFactors scale0, int use_scale0) {
    const int lane = threadIdx.x;
    const double s = use_scale0 ? scale0.v[lane] : 1.0;
    const int done = (lane < b && s != 0.0) ? 0 : 1;
    state->scale[lane] = s;
    state->err[lane] = 0.0;
    state->sum[lane] = 0.0;
    state->pred_inv[lane] = 1.0;
    state->pred_raw[lane] = 0.0;
    state->sum_p[lane] = 0.0;
    state->done[lane] = done;
    state->steps[lane] = 0;
    state->converged[lane] = 0;
    const unsigned long long all = __ballot(done != 0);
    if (lane == 0) {
        state->all_done = (all == ~0ULL) ? 1 : 0;
        state->paused = 0;
        state->executed = 0;
        state->b = b;
    }
}

// a closed-form run's check of iteration 2 (convergence.py:96-101 on delta_1 = |result_1|), per column
__global__ void k_mm64_poly_first(BatchState* __restrict__ state, const double* __restrict__ err1, int check, int err_kind, double tol, long long n) {
    const int lane = threadIdx.x;
    int done = 1;
    if (lane < state->b) {
        double e = err1[lane];
        if (err_kind == PGH_ERR_MABS && n > 0) e /= (double)n;
        state->err[lane] = e;
        if (check && e <= tol) {
            state->done[lane] = 1;
            state->converged[lane] = 1;
        }
        done = state->done[lane];
    }
    const unsigned long long all = __ballot(done != 0);
    if (lane == 0) state->all_done = (all == ~0ULL) ? 1 : 0;
}

// One taylor step of every column (pgh_poly_run's form 2): term_k = U_r * sum, the next gather row term_k * G_r, result += c_k * term_k
// for the columns still running, and the workgroup's change |result_new - result_old| per column (sum or max)
__global__ __launch_bounds__(WG) void k_mm64_poly_step(const double* __restrict__ sums, const RowOp64* __restrict__ rowop, double* __restrict__ result,
                                                        double* __restrict__ xg, double c, int linf, int64_t n, int ld, int b,
                                                        const BatchState* __restrict__ state, double* __restrict__ partials) {
    __shared__ double s_red[WG / 64][kLanes];
    if (state->all_done) return;
    const int lane = threadIdx.x & 63;
    const int lpr = lanes_per_row64(ld), rows_per_wave = 64 / lpr;
    const int l = lane & (lpr - 1), c2 = 2 * l;
    const bool live = c2 < ld;
    bool frozen[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) frozen[k] = !(c2 + k < b) || state->done[c2 + k] != 0;
    double acc[2] = {0.0, 0.0};
    const int64_t first = (blockIdx.x * (int64_t)(WG / 64) + (threadIdx.x >> 6)) * rows_per_wave + lane / lpr;
    const int64_t stride = (int64_t)gridDim.x * (WG / 64) * rows_per_wave;
    constexpr int U = 2;
    for (int64_t r0 = first; live && r0 < n; r0 += stride * U) {
        f64x2 sum[U], ro[U];
        RowOp64 op[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = r0 + u * stride;
            ok[u] = r < n;
            const int64_t at = (ok[u] ? r : 0) * ld + c2;
            sum[u] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(sums + at));
            ro[u] = *reinterpret_cast<const f64x2*>(result + at);
            op[u] = rowop[ok[u] ? r : 0];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            const int64_t at = (r0 + u * stride) * ld + c2;
            const f64x2 y = sum[u] * op[u].U;
            f64x2 rn;
            rn.x = frozen[0] ? ro[u].x : ro[u].x + c * y.x;
            rn.y = frozen[1] ? ro[u].y : ro[u].y + c * y.y;
            *reinterpret_cast<f64x2*>(xg + at) = y * op[u].G;
            *reinterpret_cast<f64x2*>(result + at) = rn;
            const double d0 = fabs(rn.x - ro[u].x), d1 = fabs(rn.y - ro[u].y);
            acc[0] = linf ? fmax(acc[0], d0) : acc[0] + d0;
            acc[1] = linf ? fmax(acc[1], d1) : acc[1] + d1;
        }
    }
    mm64_block_fold(acc[0], acc[1], lpr, c2, live, linf, s_red, partials);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------

// the buffers of one call: the row operands, the slabs a loop names, the carries, the partials and their folds, the loop state
struct MM64Run : MMRunAhead {
    pgh_graph_s* const g;
    const BsfFormat&   f;
    const int          b, ld;
    const int64_t      n, n_int;
    const size_t       slab;            // bytes of one [n_int, ld] slab of doubles
    const int          cgrid, row_grid;
    PoolBuf   rowop, bad, slabs[5], head, tail, partial, folded, state_mem;
    LoopTimer timer;

    MM64Run(pgh_graph_s* graph, int width)
        : g(graph), f(graph->bsf_mm), b(width), ld((width + 1) & ~1), n(graph->n_cols), n_int(f.n_out),
          slab(sizeof(double) * (size_t)n_int * ld), cgrid(rt().num_cus * 8), row_grid(blocks_for(n_int * lanes_per_row64(ld))) {}

    double*  s(int i) { return slabs[i].as<double>(); }
    RowOp64* ops() { return rowop.as<RowOp64>(); }
    double*  fold(int i) { return folded.as<double>() + (size_t)i * kLanes; }

    // num_slabs slabs beside the row sums (slabs[0]); the sums and the head carries start as zeros: a row without entries keeps its
    // zero sum, a tile without a head piece adds none
    int alloc(int num_slabs, bool with_state) {
        PGH_TRY(rowop.alloc(sizeof(RowOp64) * (size_t)n_int));
        PGH_TRY(bad.alloc(sizeof(int)));
        for (int i = 0; i <= num_slabs; ++i) PGH_TRY(slabs[i].alloc(slab));
        const size_t carries = sizeof(double) * (size_t)(f.num_tiles + 1) * ld;
        PGH_TRY(head.alloc(carries));
        PGH_TRY(tail.alloc(carries));
        PGH_TRY(partial.alloc(sizeof(double) * (size_t)cgrid * kLanes));
        PGH_TRY(folded.alloc(sizeof(double) * 2 * kLanes));
        PGH_HIP(hipMemsetAsync(slabs[0].p, 0, slab, rt().stream));
        PGH_HIP(hipMemsetAsync(head.p, 0, carries, rt().stream));
        PGH_HIP(hipMemsetAsync(folded.p, 0, sizeof(double) * 2 * kLanes, rt().stream));
        if (with_state) {
            PGH_TRY(state_mem.alloc(sizeof(BatchState)));
            PGH_TRY(poll_ring(&ring));
            state = state_mem.as<BatchState>();
        }
        return 0;
    }
    // the row operands of `mode` (k_mm64_rowops); *is_bad: a row whose weights are not finite
    int row_operands(int mode, double alpha, const float* lam, bool* is_bad) {
        Runtime& r = rt();
        PGH_HIP(hipMemsetAsync(bad.p, 0, sizeof(int), r.stream));
        k_mm64_rowops<<<blocks_for(n_int), WG, 0, r.stream>>>(mode, alpha, f.dst_scale, f.src_scale, g->degrees, lam, f.perm, n_int, g->n_rows, ops(),
                                                              bad.as<int>());
        PGH_HIP(hipGetLastError());
        int h_bad = 0;
        PGH_HIP(hipMemcpyAsync(&h_bad, bad.p, sizeof(int), hipMemcpyDeviceToHost, r.stream));
        PGH_HIP(hipStreamSynchronize(r.stream));
        *is_bad = h_bad != 0;
        return 0;
    }
    // slabs[0] <- the row sums of the stream times the gather slab xg
    int product(const double* xg) {
        Runtime& r = rt();
        MM64View v;
        v.colf = f.colf;
        v.val = f.val;
        v.seg_row = f.seg_row;
        v.close = f.mm_close;
        v.tile = f.tile;
        v.head = head.as<double>();
        v.tail = tail.as<double>();
        v.num_tiles = f.num_tiles;
        const int lpr = lanes_per_row64(ld);
        const int which = (f.val ? 4 : 0) + (lpr == 32 ? 0 : (lpr == 16 ? 1 : (lpr == 8 ? 2 : 3)));
        const void* kernels[8] = {(const void*)k_mm64_partial<false, 32>, (const void*)k_mm64_partial<false, 16>, (const void*)k_mm64_partial<false, 8>,
                                  (const void*)k_mm64_partial<false, 4>,  (const void*)k_mm64_partial<true, 32>,  (const void*)k_mm64_partial<true, 16>,
                                  (const void*)k_mm64_partial<true, 8>,   (const void*)k_mm64_partial<true, 4>};
        static int per_cu_of[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int& per_cu = per_cu_of[which];
        if (per_cu == 0) {
            PGH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernels[which], WG, 0));
            if (per_cu < 1) per_cu = 1;
        }
        const int grid = r.num_cus * per_cu;               // persistent: as many workgroups as the registers let a CU hold
        {
            ProfScope prof(PGH_K_SPMM);
            switch (which) {
                case 0: k_mm64_partial<false, 32><<<grid, WG, 0, r.stream>>>(v, xg, ld, s(0), state); break;
                case 1: k_mm64_partial<false, 16><<<grid, WG, 0, r.stream>>>(v, xg, ld, s(0), state); break;
                case 2: k_mm64_partial<false, 8><<<grid, WG, 0, r.stream>>>(v, xg, ld, s(0), state); break;
                case 3: k_mm64_partial<false, 4><<<grid, WG, 0, r.stream>>>(v, xg, ld, s(0), state); break;
                case 4: k_mm64_partial<true, 32><<<grid, WG, 0, r.stream>>>(v, xg, ld, s(0), state); break;
                case 5: k_mm64_partial<true, 16><<<grid, WG, 0, r.stream>>>(v, xg, ld, s(0), state); break;
                case 6: k_mm64_partial<true, 8><<<grid, WG, 0, r.stream>>>(v, xg, ld, s(0), state); break;
                default: k_mm64_partial<true, 4><<<grid, WG, 0, r.stream>>>(v, xg, ld, s(0), state); break;
            }
        }
        {
            ProfScope prof(PGH_K_FIXUP);
            k_mm64_fixup<<<blocks_for((int64_t)f.num_tiles * lpr, 64), WG, 0, r.stream>>>(v, ld, s(0), state);
        }
        PGH_HIP(hipGetLastError());
        return 0;
    }
    // The way out: `result` times the column's factor (the state's quotient when state_scale, times its output scale), rounded once
    // to f32.  A column reports first_iterations + its steps; a zero column (zero[j]) reports nothing.
    int finish(bool state_scale, const double* result, const pgh_loop_cfg* cfg, const double* out_scales, const double* in_norms, float* dst,
               int first_iterations, pgh_loop_result* results) {
        hipStream_t stream = rt().stream;
        BatchState hs;
        PGH_HIP(hipMemcpyAsync(&hs, state, sizeof(BatchState), hipMemcpyDeviceToHost, stream));
        PGH_HIP(hipStreamSynchronize(stream));
        ColFactors factors{};
        for (int j = 0; j < b; ++j) {
            double scale = out_scales ? out_scales[j] : cfg->out_scale;
            if (!out_scales && scale < 0.0) scale = in_norms ? in_norms[j] : 1.0;
            factors.v[j] = (state_scale ? hs.scale[j] : 1.0) * scale;
        }
        k_mm64_way_out<float><<<row_grid, WG, 0, stream>>>(result, nullptr, f.perm, n_int, n, b, ld, factors, dst);
        PGH_HIP(hipGetLastError());
        double ms = 0.0;
        PGH_TRY(timer.stop(&ms));
        for (int j = 0; j < b; ++j) {
            memset(&results[j], 0, sizeof(pgh_loop_result));
            if (in_norms != nullptr) results[j].in_norm = in_norms[j];
            if (in_norms != nullptr && in_norms[j] == 0.0) continue;
            results[j].iterations = first_iterations + hs.steps[j];
            results[j].converged = hs.converged[j];
            results[j].spmv_count = hs.steps[j];
            results[j].last_error = hs.err[j];
            results[j].loop_ms = ms;
        }
        return 0;
    }
};

// null arguments and widths outside [1, 64] are errors; what the loops do not serve is declined with nothing written
int check64(pgh_graph_t g, int b, bool nulls, const char* who) {
    PGH_CHECK(!nulls, std::string(who) + ": null argument");
    PGH_CHECK(b >= 1 && b <= kLanes, std::string(who) + ": the batch width must be in [1, 64]");
    if (g->n_rows != g->n_cols) return declined(PGH_BATCH64_DECLINED, "the f64 multi-seed loops need a square matrix");
    if (!g->bsf.enabled) return declined(PGH_BATCH64_DECLINED, "the f64 multi-seed loops need a graph with the blocked layout");
    if (g->n_cols == 0 || g->nnz == 0) return declined(PGH_BATCH64_DECLINED, "the f64 multi-seed loops need a graph with entries");
    return 0;
}
int check64_mats(pgh_graph_t g, pgh_mat_t p, pgh_mat_t out, const pgh_loop_cfg* cfg, const char* who) {
    PGH_CHECK(p->n == g->n_cols && out->n == g->n_cols && p->b == out->b, std::string(who) + ": shape mismatch");
    PGH_CHECK(cfg->end_modulo >= 1, "end_modulo must be >= 1");
    return 0;
}

// mode 0 / 1 / 2 of k_mm64_rowops (the modes of recursive_run_f64, pgh_spmv.hip)
int recursive_batch64(pgh_graph_t g, int mode, pgh_mat_t p, const float* lam, pgh_mat_t ranks, const pgh_loop_cfg* cfg, const double* out_scales,
                      pgh_loop_result* results, const double* in_norms, const char* who) {
    const int b = p->b;
    ColFactors inv{};
    for (int j = 0; j < b; ++j) {
        PGH_CHECK(std::isfinite(in_norms[j]) && in_norms[j] >= 0.0, std::string(who) + ": a norm that is negative or not finite");
        inv.v[j] = in_norms[j] != 0.0 ? 1.0 / in_norms[j] : 0.0;
    }
    PGH_CHECK(mode != 0 || std::isfinite(cfg->alpha), std::string(who) + ": a non-finite alpha");
    PGH_CHECK(mode == 0 || g->degrees != nullptr, "the absorbing walks need the graph's degrees");
    PGH_TRY(mm_ensure_layout(g));
    Runtime& r = rt();
    MM64Run run(g, b);
    // slabs: 0 the row sums, 1 p / |p|, 2 and 3 the two iterates, 4 the gather slab
    PGH_TRY(run.alloc(4, true));
    bool bad = false;
    PGH_TRY(run.row_operands(mode, cfg->alpha, lam, &bad));
    if (bad) return declined(PGH_BATCH64_DECLINED, "a row with absorption + degree == 0 (or a non-finite absorption): the single-vector loop's NaN");
    const int ld = run.ld, cgrid = run.cgrid;
    const int64_t n_int = run.n_int;
    double* y[2] = {run.s(2), run.s(3)};
    double* partial = run.partial.as<double>();
    BatchState* state = run.state;
    PGH_TRY(run.timer.start());
    k_mm64_state_init<<<1, kLanes, 0, r.stream>>>(state, b, inv, 1);
    // the iterate is kept UN-normalised with its quotient beside it (x_k = y_k * scale_k): x_0 = p / |p| is y_0 = p with scale_0 = 1 / |p|
    k_mm64_way_in<float><<<run.row_grid, WG, 0, r.stream>>>(p->data, run.f.perm, n_int, run.n, b, ld, inv, run.ops(), run.s(1), y[0], run.s(4));
    PGH_HIP(hipGetLastError());
    const int linf = cfg->err_kind == PGH_ERR_LINF;
    const int max_steps = cfg->max_iters - 1 > 0 ? cfg->max_iters - 1 : 0;
    Close64 cp{};
    cp.tol = cfg->tol;
    cp.n_orig = run.n;
    cp.use_quotient = cfg->use_quotient;
    cp.err_kind = cfg->err_kind;
    // step k produces the iterate of iteration k + 1 and is followed by that iteration's check
    auto enqueue_step = [&](int k) -> int {
        PGH_TRY(run.product(run.s(4)));
        {
            ProfScope prof(PGH_K_COMBINE);
            k_mm64_step<<<cgrid, WG, 0, r.stream>>>(run.s(0), run.ops(), run.s(1), y[(k - 1) & 1], y[k & 1], run.s(4), n_int, ld, b, state, partial);
        }
        if (cfg->use_quotient) k_mm64_fold<<<kLanes, WG, 0, r.stream>>>(partial, cgrid, 0, state, run.fold(0));
        Close64 c2 = cp;
        c2.check = loop_checks_at(cfg->err_kind, k + 1, cfg->max_iters, cfg->end_modulo) ? 1 : 0;
        if (c2.check) {
            ProfScope prof(PGH_K_RESIDUAL);
            k_mm64_residual<<<cgrid, WG, 0, r.stream>>>(y[k & 1], y[(k - 1) & 1], n_int, ld, b, cfg->use_quotient, linf, state, run.fold(0), partial);
            k_mm64_fold<<<kLanes, WG, 0, r.stream>>>(partial, cgrid, linf, state, run.fold(1));
        }
        k_mm64_close<<<1, kLanes, 0, r.stream>>>(state, run.fold(0), run.fold(1), c2);
        PGH_HIP(hipGetLastError());
        return run.publish_poll(k);
    };
    PGH_TRY(run.run_ahead(max_steps, enqueue_step));
    // the iterate of the last executed step: a stopped column was copied forward by every later one
    BatchPoll last{};
    PGH_HIP(hipMemcpyAsync(&last, &state->all_done, sizeof(BatchPoll), hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(hipStreamSynchronize(r.stream));
    return run.finish(true, y[last.executed & 1], cfg, out_scales, in_norms, ranks->data, 1, results);
}

}  // namespace

extern "C" int pgh_spmm_f64(pgh_graph_t g, const double* x_host, int32_t b, double* y_host) {
    PGH_TRY(check64(g, b, !(g && x_host && y_host), "pgh_spmm_f64"));
    PGH_CHECK(x_host != y_host, "pgh_spmm_f64: the output aliases the input");
    PGH_TRY(mm_ensure_layout(g));
    Runtime& r = rt();
    MM64Run run(g, b);
    PGH_TRY(run.alloc(1, false));                          // slabs: 0 the row sums, 1 the gather slab
    bool bad = false;
    PGH_TRY(run.row_operands(3, 0.0, nullptr, &bad));
    PoolBuf io;                                            // the caller's [n, b] doubles on the device, in and then out
    const size_t bytes = sizeof(double) * (size_t)run.n * b;
    PGH_TRY(io.alloc(bytes));
    StreamFence fence;
    PGH_HIP(hipMemcpyAsync(io.p, x_host, bytes, hipMemcpyHostToDevice, r.stream));
    ColFactors ones{};
    for (int j = 0; j < kLanes; ++j) ones.v[j] = 1.0;
    k_mm64_way_in<double><<<run.row_grid, WG, 0, r.stream>>>(io.as<double>(), run.f.perm, run.n_int, run.n, b, run.ld, ones, run.ops(), nullptr, nullptr,
                                                             run.s(1));
    PGH_HIP(hipGetLastError());
    PGH_TRY(run.product(run.s(1)));
    k_mm64_way_out<double><<<run.row_grid, WG, 0, r.stream>>>(run.s(0), run.ops(), run.f.perm, run.n_int, run.n, b, run.ld, ones, io.as<double>());
    PGH_HIP(hipGetLastError());
    PGH_HIP(hipMemcpyAsync(y_host, io.p, bytes, hipMemcpyDeviceToHost, r.stream));
    PGH_HIP(fence.wait());
    return 0;
}

extern "C" int pgh_ppr_run_batch_f64(pgh_graph_t g, pgh_mat_t p, pgh_mat_t ranks, const pgh_loop_cfg* cfg, const double* out_scales,
                                     pgh_loop_result* results, const double* in_norms) {
    const char* who = "pgh_ppr_run_batch_f64";
    PGH_TRY(check64(g, p ? p->b : 1, !(g && p && ranks && cfg && results && in_norms), who));
    PGH_TRY(check64_mats(g, p, ranks, cfg, who));
    return recursive_batch64(g, 0, p, nullptr, ranks, cfg, out_scales, results, in_norms, who);
}

extern "C" int pgh_absorb_run_batch_f64(pgh_graph_t g, pgh_mat_t p, pgh_vec_t lam, pgh_mat_t ranks, const pgh_loop_cfg* cfg,
                                        const double* out_scales, pgh_loop_result* results, const double* in_norms) {
    const char* who = "pgh_absorb_run_batch_f64";
    PGH_TRY(check64(g, p ? p->b : 1, !(g && p && lam && ranks && cfg && results && in_norms), who));
    PGH_TRY(check64_mats(g, p, ranks, cfg, who));
    PGH_CHECK(lam->n == g->n_cols, std::string(who) + ": absorption length mismatch");
    return recursive_batch64(g, 1, p, lam->data, ranks, cfg, out_scales, results, in_norms, who);
}

extern "C" int pgh_sarw_run_batch_f64(pgh_graph_t g, pgh_mat_t p, pgh_mat_t ranks, const pgh_loop_cfg* cfg, const double* out_scales,
                                      pgh_loop_result* results, const double* in_norms) {
    const char* who = "pgh_sarw_run_batch_f64";
    PGH_TRY(check64(g, p ? p->b : 1, !(g && p && ranks && cfg && results && in_norms), who));
    PGH_TRY(check64_mats(g, p, ranks, cfg, who));
    return recursive_batch64(g, 2, p, nullptr, ranks, cfg, out_scales, results, in_norms, who);
}

// The taylor form with f64 terms and accumulator for b columns: iteration 1 is result_1 = c_1 p with the check of iteration 2 on
// |result_1|, step k (iteration k + 1) adds c_{k+1} (M^T)^k p and the check of iteration k + 2 compares result_{k+1} with result_k.
// Column j: iterations = 2 + its steps, as pgh_poly_run reports them.
extern "C" int pgh_poly_run_batch_f64(pgh_graph_t g, pgh_mat_t p, const double* coeffs, int32_t num_coeffs, pgh_mat_t result,
                                      const pgh_loop_cfg* cfg, const double* out_scales, pgh_loop_result* results) {
    const char* who = "pgh_poly_run_batch_f64";
    PGH_TRY(check64(g, p ? p->b : 1, !(g && p && result && cfg && results && (coeffs || num_coeffs == 0)), who));
    PGH_TRY(check64_mats(g, p, result, cfg, who));
    PGH_CHECK(num_coeffs >= 0, std::string(who) + ": a negative schedule length");
    for (int i = 0; i < num_coeffs; ++i) PGH_CHECK(std::isfinite(coeffs[i]), std::string(who) + ": a non-finite coefficient");
    Runtime& r = rt();
    const int b = p->b;
    auto coeff = [&](int it) -> double { return (it >= 1 && it <= num_coeffs) ? coeffs[it - 1] : 0.0; };
    if (cfg->max_iters <= 1) {            // convergence.py:86-89: stops before the first step, the sum is empty
        PGH_HIP(hipMemsetAsync(result->data, 0, sizeof(float) * (size_t)g->n_cols * b, r.stream));
        PGH_HIP(hipStreamSynchronize(r.stream));
        for (int j = 0; j < b; ++j) {
            memset(&results[j], 0, sizeof(pgh_loop_result));
            results[j].iterations = 1;
        }
        return 0;
    }
    PGH_TRY(mm_ensure_layout(g));
    MM64Run run(g, b);
    PGH_TRY(run.alloc(2, true));                           // slabs: 0 the row sums, 1 the result, 2 the gather slab (the current term)
    bool bad = false;
    PGH_TRY(run.row_operands(3, 0.0, nullptr, &bad));
    const int ld = run.ld, cgrid = run.cgrid;
    const int64_t n_int = run.n_int;
    double* partial = run.partial.as<double>();
    BatchState* state = run.state;
    PGH_TRY(run.timer.start());
    ColFactors c1{};
    for (int j = 0; j < kLanes; ++j) c1.v[j] = coeff(1);
    k_mm64_state_init<<<1, kLanes, 0, r.stream>>>(state, b, c1, 0);
    // result_1 = c_1 p, term_1 = p in gather form
    k_mm64_way_in<float><<<run.row_grid, WG, 0, r.stream>>>(p->data, run.f.perm, n_int, run.n, b, ld, c1, run.ops(), run.s(1), nullptr, run.s(2));
    const int linf = cfg->err_kind == PGH_ERR_LINF;
    k_mm64_residual<<<cgrid, WG, 0, r.stream>>>(run.s(1), nullptr, n_int, ld, b, 0, linf, state, run.fold(0), partial);
    k_mm64_fold<<<kLanes, WG, 0, r.stream>>>(partial, cgrid, linf, state, run.fold(1));
    const int check2 = loop_checks_at(cfg->err_kind, 2, cfg->max_iters, cfg->end_modulo);
    k_mm64_poly_first<<<1, kLanes, 0, r.stream>>>(state, run.fold(1), check2, cfg->err_kind, cfg->tol, (long long)run.n);
    PGH_HIP(hipGetLastError());
    const int max_steps = cfg->max_iters - 2 > 0 ? cfg->max_iters - 2 : 0;
    Close64 cp{};
    cp.tol = cfg->tol;
    cp.n_orig = run.n;
    cp.use_quotient = 0;
    cp.err_kind = cfg->err_kind;
    // step k runs iteration k + 1; its check is the one of iteration k + 2
    auto enqueue_step = [&](int k) -> int {
        PGH_TRY(run.product(run.s(2)));
        {
            ProfScope prof(PGH_K_COMBINE);
            k_mm64_poly_step<<<cgrid, WG, 0, r.stream>>>(run.s(0), run.ops(), run.s(1), run.s(2), coeff(k + 1), linf, n_int, ld, b, state, partial);
        }
        Close64 c2 = cp;
        c2.check = loop_checks_at(cfg->err_kind, k + 2, cfg->max_iters, cfg->end_modulo) ? 1 : 0;
        if (c2.check) k_mm64_fold<<<kLanes, WG, 0, r.stream>>>(partial, cgrid, linf, state, run.fold(1));
        k_mm64_close<<<1, kLanes, 0, r.stream>>>(state, run.fold(0), run.fold(1), c2);
        PGH_HIP(hipGetLastError());
        return run.publish_poll(k);
    };
    PGH_TRY(run.run_ahead(max_steps, enqueue_step));
    return run.finish(false, run.s(1), cfg, out_scales, nullptr, result->data, 2, results);
}

PGH_WARM_KERNEL(k_mm64_fixup)
