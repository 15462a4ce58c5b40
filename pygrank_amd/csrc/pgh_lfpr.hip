// include/pgh_lfpr.h: the row operands of the locally fair PageRank in one pass, and what follows the product of one of its steps in one
// pass.
//
// Reference counterpart: LFPR.normalization / _start / _formula (pygrank/algorithms/filters/adhoc.py:227-293) with the quotient
// (abstract_filters.py:133-134) and the residual (convergence.py:96-101): about fifteen backend calls at set-up and ten per step, each a
// pass over n-vectors with a temporary.
//
// Three kernels on the engine's stream, all HBM-streaming:
//   k_lfpr_setup<ORIG>   lane <-> four consecutive elements (16-byte loads and stores), grid-stride; the elements behind the last whole
//                        quad -- or all of them when an operand is not 16-byte aligned -- go one per lane.  Every operand load is
//                        unconditional, the three cases are selects; the nullable `original` is the template parameter.
//   k_lfpr_close<LINF>   the same shape: seven operand quads in, two out, five sums.
//   k_fold_regions       one workgroup folds the block partials of every sum in their order (pgh_slab.h).
// Sums: f64 per lane -> wavefront shuffles -> LDS -> one partial per workgroup in rt().d_partials (one region per sum) -> the fold.  The
// grid is a function of the length alone, so two calls on the same input return the same bits.
// Every stored value, the residual term y * y_scale - x * x_scale and the case test R < phi * (R + B) are formed from individually rounded
// operations in the order the header writes them: this file is compiled with contraction into fused multiply-adds switched off (the
// pragma below; __dmul_rn and its kin are inline functions of a header the pragma does not reach, and their bodies are contracted like
// any other product and sum: measured -- a row on the edge came out as 2^-54 instead of 0 with them), so that a sign, a maximum,
// a row exactly on the edge between two cases and a difference that cancels (dR and dB next to that edge) come out as in a plain f64
// evaluation.  The kernels are bound by HBM, not by these operations.
#include "pgh_slab.h"
#include "pgh_lfpr.h"

#include <cmath>

using namespace pgh;

#pragma clang fp contract(off)

namespace {
static_assert(kPartialRegions >= 5, "one region of block partials per sum");
const char* const kSetup = "pgh_lfpr_setup";
const char* const kClose = "pgh_lfpr_close";

__device__ __forceinline__ double safe_inv(double v) { return v != 0.0 ? 1.0 / v : 0.0; }

struct SetupOut {
    float d, dr, db, xr, xb;
};

__device__ __forceinline__ SetupOut setup_one(float s_, float r_, float b_, float o_, double phi, double omp) {
    const double s = (double)s_, R = (double)r_, B = (double)b_, o = (double)o_;
    const bool case1 = R < phi * (R + B);
    const bool case2 = !case1 && R != 0.0;
    const double iR = safe_inv(R), iB = safe_inv(B);
    SetupOut out;
    out.d = (float)(case1 ? iB * omp : case2 ? iR * phi : 1.0);
    out.dr = (float)(case1 ? phi - (omp * iB) * R : case2 ? 0.0 : phi);
    out.db = (float)(case2 ? omp - (phi * iR) * B : case1 ? 0.0 : omp);
    out.xr = (float)(o * s);
    out.xb = (float)(o * (1.0 - s));
    return out;
}

template <bool ORIG>
__global__ __launch_bounds__(kSlabBlock) __attribute__((amdgpu_waves_per_eu(1, 4))) void k_lfpr_setup(const float* __restrict__ sens, const float* __restrict__ out_r,
                                                           const float* __restrict__ out_b, const float* __restrict__ orig, double phi, int64_t n,
                                                           int64_t nvec, float* __restrict__ d, float* __restrict__ dr, float* __restrict__ db,
                                                           float* __restrict__ xr, float* __restrict__ xb, double* __restrict__ partials) {
    __shared__ double s_red[4];
    const double omp = 1.0 - phi;
    const int64_t stride = (int64_t)gridDim.x * kSlabBlock;
    const int64_t gtid = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x;
    double sum_r = 0.0, sum_b = 0.0;
    for (int64_t v = gtid; v < nvec; v += stride) {
        const float4 s4 = reinterpret_cast<const float4*>(sens)[v];
        const float4 r4 = reinterpret_cast<const float4*>(out_r)[v];
        const float4 b4 = reinterpret_cast<const float4*>(out_b)[v];
        float4 o4 = make_float4(1.f, 1.f, 1.f, 1.f);
        if (ORIG) o4 = reinterpret_cast<const float4*>(orig)[v];
        loads_issued();
        const SetupOut e0 = setup_one(s4.x, r4.x, b4.x, o4.x, phi, omp);
        const SetupOut e1 = setup_one(s4.y, r4.y, b4.y, o4.y, phi, omp);
        const SetupOut e2 = setup_one(s4.z, r4.z, b4.z, o4.z, phi, omp);
        const SetupOut e3 = setup_one(s4.w, r4.w, b4.w, o4.w, phi, omp);
        reinterpret_cast<float4*>(d)[v] = make_float4(e0.d, e1.d, e2.d, e3.d);
        reinterpret_cast<float4*>(dr)[v] = make_float4(e0.dr, e1.dr, e2.dr, e3.dr);
        reinterpret_cast<float4*>(db)[v] = make_float4(e0.db, e1.db, e2.db, e3.db);
        reinterpret_cast<float4*>(xr)[v] = make_float4(e0.xr, e1.xr, e2.xr, e3.xr);
        reinterpret_cast<float4*>(xb)[v] = make_float4(e0.xb, e1.xb, e2.xb, e3.xb);
        sum_r += (((double)e0.xr + (double)e1.xr) + (double)e2.xr) + (double)e3.xr;
        sum_b += (((double)e0.xb + (double)e1.xb) + (double)e2.xb) + (double)e3.xb;
    }
    for (int64_t i = 4 * nvec + gtid; i < n; i += stride) {
        const SetupOut e = setup_one(sens[i], out_r[i], out_b[i], ORIG ? orig[i] : 1.f, phi, omp);
        d[i] = e.d;
        dr[i] = e.dr;
        db[i] = e.db;
        xr[i] = e.xr;
        xb[i] = e.xb;
        sum_r += (double)e.xr;
        sum_b += (double)e.xb;
    }
    sum_r = block_reduce_256<0>(sum_r, s_red);
    sum_b = block_reduce_256<0>(sum_b, s_red);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = sum_r;
        partials[kMaxPartials + blockIdx.x] = sum_b;
    }
}

struct CloseAcc {
    double sy = 0.0, sr = 0.0, sb = 0.0, err = 0.0, sd = 0.0;
};
struct CloseOut {
    float y, u;
};

template <bool LINF>
__device__ __forceinline__ CloseOut close_one(float y0, float x, float xr, float xb, float d, float dr, float db, double cR, double cB,
                                              double x_scale, double y_scale, CloseAcc& acc) {
    CloseOut out;
    out.y = (float)(((double)y0 + cR * (double)xr) + cB * (double)xb);
    const double y = (double)out.y;
    out.u = (float)(y * (double)d);
    acc.sy += y;
    acc.sr += y * (double)dr;
    acc.sb += y * (double)db;
    const double t = y * y_scale - (double)x * x_scale;
    const double mag = fabs(t);
    acc.err = LINF ? fmax(acc.err, mag) : acc.err + mag;
    acc.sd += t > 0.0 ? y : t < 0.0 ? -y : 0.0;
    return out;
}

// y may be y0 (every element is read, then written, by the one lane that owns it).  No operand carries __restrict__ (loads_issued(),
// pgh_slab.h); every load of an iteration precedes its stores anyway
template <bool LINF>
__global__ __launch_bounds__(kSlabBlock) __attribute__((amdgpu_waves_per_eu(1, 4))) void k_lfpr_close(const float* y0, const float* x, double x_scale, const float* xr,
                                                           const float* xb, const float* d, const float* dr, const float* db, double cR,
                                                           double cB, double y_scale, int64_t n, int64_t nvec, float* y, float* u,
                                                           double* __restrict__ partials) {
    __shared__ double s_red[4];
    const int64_t stride = (int64_t)gridDim.x * kSlabBlock;
    const int64_t gtid = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x;
    CloseAcc acc;
    for (int64_t v = gtid; v < nvec; v += stride) {
        const float4 a4 = reinterpret_cast<const float4*>(y0)[v];
        const float4 x4 = reinterpret_cast<const float4*>(x)[v];
        const float4 r4 = reinterpret_cast<const float4*>(xr)[v];
        const float4 b4 = reinterpret_cast<const float4*>(xb)[v];
        const float4 d4 = reinterpret_cast<const float4*>(d)[v];
        const float4 p4 = reinterpret_cast<const float4*>(dr)[v];
        const float4 q4 = reinterpret_cast<const float4*>(db)[v];
        loads_issued();
        const CloseOut e0 = close_one<LINF>(a4.x, x4.x, r4.x, b4.x, d4.x, p4.x, q4.x, cR, cB, x_scale, y_scale, acc);
        const CloseOut e1 = close_one<LINF>(a4.y, x4.y, r4.y, b4.y, d4.y, p4.y, q4.y, cR, cB, x_scale, y_scale, acc);
        const CloseOut e2 = close_one<LINF>(a4.z, x4.z, r4.z, b4.z, d4.z, p4.z, q4.z, cR, cB, x_scale, y_scale, acc);
        const CloseOut e3 = close_one<LINF>(a4.w, x4.w, r4.w, b4.w, d4.w, p4.w, q4.w, cR, cB, x_scale, y_scale, acc);
        reinterpret_cast<float4*>(y)[v] = make_float4(e0.y, e1.y, e2.y, e3.y);
        reinterpret_cast<float4*>(u)[v] = make_float4(e0.u, e1.u, e2.u, e3.u);
    }
    for (int64_t i = 4 * nvec + gtid; i < n; i += stride) {
        const CloseOut e = close_one<LINF>(y0[i], x[i], xr[i], xb[i], d[i], dr[i], db[i], cR, cB, x_scale, y_scale, acc);
        y[i] = e.y;
        u[i] = e.u;
    }
    const double sy = block_reduce_256<0>(acc.sy, s_red);
    const double sr = block_reduce_256<0>(acc.sr, s_red);
    const double sb = block_reduce_256<0>(acc.sb, s_red);
    const double err = LINF ? block_reduce_256<1>(acc.err, s_red) : block_reduce_256<0>(acc.err, s_red);
    const double sd = block_reduce_256<0>(acc.sd, s_red);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = sy;
        partials[kMaxPartials + blockIdx.x] = sr;
        partials[2 * kMaxPartials + blockIdx.x] = sb;
        partials[3 * kMaxPartials + blockIdx.x] = err;
        partials[4 * kMaxPartials + blockIdx.x] = sd;
    }
}

// quads the kernels take as 16-byte words, and the grid for them plus the elements that go one per lane
void shape_for(int64_t n, bool all_aligned, int64_t* nvec, int* grid) {
    *nvec = all_aligned ? n / 4 : 0;
    const int64_t lanes = *nvec + (n - 4 * *nvec);
    *grid = grid_capped(lanes, kSlabBlock);
}
}  // namespace

PGH_WARM_KERNEL(k_lfpr_setup<false>)

extern "C" int pgh_lfpr_setup(pgh_vec_t sensitive, pgh_vec_t out_r, pgh_vec_t out_b, pgh_vec_t original, double phi, pgh_vec_t d,
                              pgh_vec_t dR, pgh_vec_t dB, pgh_vec_t xR, pgh_vec_t xB, double* sums_host) {
    PGH_CHECK(sensitive && out_r && out_b && d && dR && dB && xR && xB && sums_host, "pgh_lfpr_setup: null argument");
    const int64_t n = sensitive->n;
    PGH_CHECK(out_r->n == n && out_b->n == n && (original == nullptr || original->n == n) && d->n == n && dR->n == n && dB->n == n &&
                  xR->n == n && xB->n == n,
              "pgh_lfpr_setup: the vectors differ in length");
    const float* ins[4] = {sensitive->data, out_r->data, out_b->data, original ? original->data : nullptr};
    float* outs[5] = {d->data, dR->data, dB->data, xR->data, xB->data};
    if (n > 0) {
        for (int a = 0; a < 5; ++a) {
            for (int b = a + 1; b < 5; ++b) PGH_CHECK(outs[a] != outs[b], "pgh_lfpr_setup: two outputs share their memory");
            for (int b = 0; b < 4; ++b) PGH_CHECK(outs[a] != ins[b], "pgh_lfpr_setup: an output shares its memory with an input");
        }
    }
    if (!std::isfinite(phi)) return declined(PGH_LFPR_DECLINED, kSetup, "phi is not finite");
    if (n == 0) {
        sums_host[0] = sums_host[1] = 0.0;
        return 0;
    }
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    bool ok16 = true;
    for (const float* p : ins) ok16 = ok16 && aligned16(p);
    for (const float* p : outs) ok16 = ok16 && aligned16(p);
    int64_t nvec = 0;
    int grid = 1;
    shape_for(n, ok16, &nvec, &grid);
    if (original != nullptr)
        k_lfpr_setup<true><<<grid, kSlabBlock, 0, r.stream>>>(ins[0], ins[1], ins[2], ins[3], phi, n, nvec, outs[0], outs[1], outs[2], outs[3],
                                                          outs[4], r.d_partials);
    else
        k_lfpr_setup<false><<<grid, kSlabBlock, 0, r.stream>>>(ins[0], ins[1], ins[2], ins[0], phi, n, nvec, outs[0], outs[1], outs[2], outs[3],
                                                           outs[4], r.d_partials);
    PGH_HIP(hipGetLastError());
    return fold_regions_to_host(grid, 2, -1, sums_host);
}

extern "C" int pgh_lfpr_close(pgh_vec_t y0, pgh_vec_t x, double x_scale, pgh_vec_t xR, pgh_vec_t xB, pgh_vec_t d, pgh_vec_t dR,
                              pgh_vec_t dB, double cR, double cB, double y_scale, int32_t err_kind, pgh_vec_t y, pgh_vec_t u,
                              double* sums_host) {
    PGH_CHECK(y0 && x && xR && xB && d && dR && dB && y && u && sums_host, "pgh_lfpr_close: null argument");
    const int64_t n = y0->n;
    PGH_CHECK(x->n == n && xR->n == n && xB->n == n && d->n == n && dR->n == n && dB->n == n && y->n == n && u->n == n,
              "pgh_lfpr_close: the vectors differ in length");
    const float* ins[7] = {y0->data, x->data, xR->data, xB->data, d->data, dR->data, dB->data};
    if (n > 0) {
        PGH_CHECK(u->data != y->data, "pgh_lfpr_close: u and y share their memory");
        for (int a = 0; a < 7; ++a) {
            PGH_CHECK(u->data != ins[a], "pgh_lfpr_close: u shares its memory with an input");
            PGH_CHECK(a == 0 || y->data != ins[a], "pgh_lfpr_close: y shares its memory with an input other than y0");
        }
    }
    if (!(std::isfinite(cR) && std::isfinite(cB) && std::isfinite(x_scale) && std::isfinite(y_scale)))
        return declined(PGH_LFPR_DECLINED, kClose, "a coefficient or a scale is not finite");
    if (err_kind != PGH_ERR_MABS && err_kind != PGH_ERR_L1 && err_kind != PGH_ERR_LINF)
        return declined(PGH_LFPR_DECLINED, kClose, "the residual is sum |.| (PGH_ERR_MABS, PGH_ERR_L1) or max |.| (PGH_ERR_LINF)");
    if (n == 0) {
        for (int k = 0; k < 5; ++k) sums_host[k] = 0.0;
        return 0;
    }
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    bool ok16 = aligned16(y->data) && aligned16(u->data);
    for (const float* p : ins) ok16 = ok16 && aligned16(p);
    int64_t nvec = 0;
    int grid = 1;
    shape_for(n, ok16, &nvec, &grid);
    const bool linf = err_kind == PGH_ERR_LINF;
    if (linf)
        k_lfpr_close<true><<<grid, kSlabBlock, 0, r.stream>>>(ins[0], ins[1], x_scale, ins[2], ins[3], ins[4], ins[5], ins[6], cR, cB, y_scale, n,
                                                          nvec, y->data, u->data, r.d_partials);
    else
        k_lfpr_close<false><<<grid, kSlabBlock, 0, r.stream>>>(ins[0], ins[1], x_scale, ins[2], ins[3], ins[4], ins[5], ins[6], cR, cB, y_scale, n,
                                                           nvec, y->data, u->data, r.d_partials);
    PGH_HIP(hipGetLastError());
    return fold_regions_to_host(grid, 5, linf ? 3 : -1, sums_host);
}
