// include/pgh_fair.h: the edited priors of up to 64 candidates of FairPersonalizer in one elementwise pass.
//
// Reference counterpart: FairPersonalizer.__culep (pygrank/algorithms/postprocess/fairness.py:78-93), about ten elementwise backend
// calls and as many temporaries per bucket and candidate.
//
// One kernel on the engine's stream:
//   k_prior_edit   lane <-> one element of the row-major [n, probes] slab, consecutive lanes on consecutive elements: a wavefront stores
//                  256 contiguous bytes.  The lanes that share a row load the same three operand words (one request per row, served
//                  from cache).  The parameters lie in LDS as [probes][4 buckets + 1] doubles, the two differences of every bucket
//                  already formed on the host (the same f64 subtraction the reference does on Python floats).  A lane walks the slab
//                  grid-stride; its (row, column) advance by the stride's quotient and remainder, so there is one 64-bit division
//                  per lane, not per element.
//   exp(-b d) is the reciprocal of exp(b d) while |b d| < 700 (both finite and normal there: one rounding more, far below the f32
//   store's half ulp); outside it is evaluated on its own.
#include "pgh_slab.h"
#include "pgh_fair.h"

#include <cmath>
#include <vector>

using namespace pgh;

namespace {
constexpr int kMaxParams = PGH_FAIR_MAX_PROBES * (4 * PGH_FAIR_MAX_BUCKETS + 1);

__global__ __launch_bounds__(kSlabBlock) void k_prior_edit(const float* __restrict__ pers, const float* __restrict__ sens,
                                                            const float* __restrict__ ranks, double rank_max,
                                                            const double* __restrict__ params /* [probes][np]: (a1 - a0, a0, b1 - b0, b0) x buckets, residual */,
                                                            int buckets, int probes, int skew, int64_t n, float* __restrict__ out) {
    __shared__ double s_p[kMaxParams];
    const int np = 4 * buckets + 1;
    for (int j = threadIdx.x; j < probes * np; j += kSlabBlock) s_p[j] = params[j];
    __syncthreads();
    const int64_t total = n * probes;
    const int64_t stride = (int64_t)gridDim.x * kSlabBlock;
    int64_t e = blockIdx.x * (int64_t)kSlabBlock + threadIdx.x;
    if (e >= total) return;
    int64_t row = e / probes;
    int col = (int)(e - row * probes);
    const int64_t row_step = stride / probes;
    const int col_step = (int)(stride - row_step * probes);
    for (; e < total; e += stride) {
        const double p = (double)pers[row], s = (double)sens[row];
        const double r = (double)ranks[row] / rank_max;
        const double d = skew ? r - p : fabs(r - p);
        const double* __restrict__ P = s_p + col * np;
        double res = buckets == 0 ? r : 0.0;
        for (int t = 0; t < buckets; ++t) {
            const double a = s * P[4 * t] + P[4 * t + 1];
            const double b = s * P[4 * t + 2] + P[4 * t + 3];
            const double x = b * d;
            const double up = exp(x);
            const double down = fabs(x) < 700.0 ? 1.0 / up : exp(-x);
            res = res + (1.0 - a) * up + a * down;
        }
        const double keep = P[np - 1];
        out[e] = (float)((1.0 - keep) * res + p * keep);
        row += row_step;
        col += col_step;
        if (col >= probes) {
            col -= probes;
            ++row;
        }
    }
}

const char* const kEdit = "pgh_prior_edit";
}  // namespace

PGH_WARM_KERNEL(k_prior_edit)

extern "C" int pgh_prior_edit(pgh_vec_t personalization, pgh_vec_t sensitive, pgh_vec_t ranks, double rank_max,
                              const double* params_host, int32_t buckets, int32_t probes, int32_t skew, pgh_mat_t out) {
    PGH_CHECK(personalization && sensitive && ranks && params_host && out, "pgh_prior_edit: null argument");
    PGH_CHECK(probes >= 1 && buckets >= 0, "pgh_prior_edit: probes >= 1 and buckets >= 0 expected");
    if (probes > PGH_FAIR_MAX_PROBES) return declined(PGH_FAIR_DECLINED, kEdit, "more than 64 probes");
    if (buckets > PGH_FAIR_MAX_BUCKETS) return declined(PGH_FAIR_DECLINED, kEdit, "more than 4 parameter buckets");
    const int64_t n = personalization->n;
    PGH_CHECK(sensitive->n == n && ranks->n == n && out->n == n, "pgh_prior_edit: the three vectors and out differ in length");
    PGH_CHECK(out->b == probes, "pgh_prior_edit: out must have one column per probe");
    if (rank_max == 0.0 || !std::isfinite(rank_max)) return declined(PGH_FAIR_DECLINED, kEdit, "rank_max is zero or not finite");
    const int np = 4 * buckets + 1;
    std::vector<double> staged((size_t)probes * np);
    for (int q = 0; q < probes; ++q) {
        const double* P = params_host + (size_t)q * np;
        for (int j = 0; j < np; ++j)
            if (!std::isfinite(P[j])) return declined(PGH_FAIR_DECLINED, kEdit, "non-finite parameter");
        double* S = staged.data() + (size_t)q * np;
        for (int t = 0; t < buckets; ++t) {
            S[4 * t] = P[4 * t] - P[4 * t + 1];
            S[4 * t + 1] = P[4 * t + 1];
            S[4 * t + 2] = P[4 * t + 2] - P[4 * t + 3];
            S[4 * t + 3] = P[4 * t + 3];
        }
        S[np - 1] = P[np - 1];
    }
    if (n == 0) return 0;
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const size_t bytes = sizeof(double) * staged.size();
    PoolBuf d_p;
    PGH_TRY(d_p.alloc(bytes));
    StreamFence fence;                                       // the staged parameters go away
    PGH_HIP(hipMemcpyAsync(d_p.p, staged.data(), bytes, hipMemcpyHostToDevice, r.stream));
    k_prior_edit<<<grid_capped(n * probes, kSlabBlock), kSlabBlock, 0, r.stream>>>(personalization->data, sensitive->data, ranks->data, rank_max,
                                                                          d_p.as<double>(), buckets, probes, skew != 0 ? 1 : 0, n, out->data);
    PGH_HIP(hipGetLastError());
    PGH_HIP(fence.wait());
    return 0;
}
