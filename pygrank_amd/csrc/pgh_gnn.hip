// include/pgh_gnn.h: the transposed graph with its partner's mask mirrored, the resident loop of the linear recurrences (the forward and
// the adjoint passes of pygrank_amd/gnn.py), and slab views of foreign buffers.
//
// Reference counterpart: pygrank's APPNP example (tests/test_gnn.py:22-28) differentiates ranker.propagate(..., graph_dropout=) by
// running the filter on an autograd backend.  Here the filters a GNN propagates with are linear maps of the feature slab, a step under
// graph_dropout multiplies by the masked matrix of its seed, and the adjoint of K such steps is K steps with the transposed masked
// matrices in reverse order: the same multi-seed kernel (k_mm_partial<..., DROP>, pgh_spmm.hip) on the transposed graph, whose index
// words name the partner's entries.
#include "pgh_kernels.h"
#include "pgh_gnn.h"

#include <hipcub/hipcub.hpp>

#include <cmath>

using namespace pgh;

namespace {

constexpr int kLanes = 64;

// ------------------------------------------------------------------------------------------------- transposition
__global__ void k_gnn_iota(int32_t* __restrict__ v, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] = (int32_t)i;
}

// run-length pass over the sorted columns: ptr[s] = first position whose column is >= s (s = 0 .. n)
__global__ void k_gnn_ptr(const int32_t* __restrict__ col_sorted, int64_t nnz, int64_t n, int32_t* __restrict__ ptr) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= nnz; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t prev = i > 0 ? (int64_t)col_sorted[i - 1] : -1;
        const int64_t cur = i < nnz ? (int64_t)col_sorted[i] : n;
        for (int64_t s = prev + 1; s <= cur && s <= n; ++s) ptr[s] = (int32_t)i;
    }
}

// position i of the transposed CSR holds entry e = entry_sorted[i] of the stored one: its column there is e's row here
__global__ void k_gnn_fill(const int32_t* __restrict__ entry_sorted, int64_t nnz, const int32_t* __restrict__ rowptr, int64_t n,
                           const float* __restrict__ val, const int32_t* __restrict__ mult, int32_t* __restrict__ col_t,
                           float* __restrict__ val_t, int32_t* __restrict__ mult_t) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t e = entry_sorted[i];
        int64_t lo = 0, hi = n - 1;                          // the largest row r with rowptr[r] <= e (empty rows share their successor's start)
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (rowptr[mid] <= e) lo = mid;
            else hi = mid - 1;
        }
        col_t[i] = (int32_t)lo;
        val_t[i] = val[e];
        if (mult_t != nullptr) mult_t[i] = mult[e];
    }
}

// row sums of the stored CSR, one wavefront per row, f64 sums: the transposed graph's degrees (the row sums of ITS M)
__global__ __launch_bounds__(WG) void k_gnn_row_sums(const int32_t* __restrict__ rowptr, const float* __restrict__ val, int64_t n,
                                                      float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = blockIdx.x * (int64_t)(WG / 64) + (threadIdx.x >> 6), stride = (int64_t)gridDim.x * (WG / 64);
    for (int64_t r = wave; r < n; r += stride) {
        double s = 0.0;
        for (int e = rowptr[r] + lane; e < rowptr[r + 1]; e += 64) s += (double)val[e];
        s = wave_reduce_sum(s);
        if (lane == 0) out[r] = (float)s;
    }
}

// ------------------------------------------------------------------------------------------------- the loop's close
typedef float f32x4 __attribute__((ext_vector_type(4)));

// One step's close, a float4 of one row per thread: the product P = dst scale * row sums, the next iterate s = a * P + b * v, acc += c * s
// and the iterate in gather form (s * s').  first: the way in -- s = b * v (b carries s0), acc = c * s, the row sums are not read.
// Rows without entries hold zero sums for the whole run (cleared once by the driver): they need no flag here.
__global__ __launch_bounds__(WG) void k_gnn_close(const f32x4* __restrict__ rowop, const f32x4* __restrict__ sums, const f32x4* __restrict__ v,
                                                   f32x4* __restrict__ acc, f32x4* __restrict__ xg, int64_t n_int, int quads, float a, float b,
                                                   float c, int first) {
    const int64_t total = n_int * quads;
    for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < total; i += (int64_t)gridDim.x * WG) {
        const f32x4 op = rowop[i / quads];
        const f32x4 vv = v[i];
        f32x4 s = vv * b;
        if (!first) s += (__builtin_nontemporal_load(sums + i) * op[0]) * a;
        const f32x4 cs = s * c;
        acc[i] = first ? cs : acc[i] + cs;
        xg[i] = s * op[1];
    }
}

}  // namespace

extern "C" int pgh_graph_transposed(pgh_graph_t g, pgh_graph_t* out) {
    PGH_CHECK(g && out, "pgh_graph_transposed: null argument");
    if (g->n_rows != g->n_cols) return declined(PGH_GNN_DECLINED, "pgh_graph_transposed: a square matrix only");
    if (g->part_perm != nullptr || g->row_begin != 0) return declined(PGH_GNN_DECLINED, "pgh_graph_transposed: not on a slice of a row partition");
    if (g->rowptr == nullptr || g->col == nullptr || g->val == nullptr) return declined(PGH_GNN_DECLINED, "pgh_graph_transposed: the graph keeps no CSR image");
    if (!g->bsf.enabled) return declined(PGH_GNN_DECLINED, "pgh_graph_transposed: the graph has no blocked layout");
    if (g->n_rows == 0) return declined(PGH_GNN_DECLINED, "pgh_graph_transposed: an empty graph");
    PGH_TRY(ensure_init());
    Runtime& r = rt();
    const int64_t n = g->n_rows, nnz = g->nnz;
    const bool value_free = g->keep_mult != nullptr;
    pgh_graph_s* t = new pgh_graph_s();
    t->n_rows = n;
    t->n_cols = n;
    t->nnz = nnz;
    const int rc = [&]() -> int {
        DevBuf<int32_t> col_sorted, entry, entry_sorted, mult_t;
        DevBuf<char> temp;
        const size_t count = (size_t)(nnz > 0 ? nnz : 1);
        PGH_HIP(pooled_malloc(&t->rowptr, sizeof(int32_t) * (size_t)(n + 1)));
        PGH_HIP(pooled_malloc(&t->col, sizeof(int32_t) * count));
        PGH_HIP(pooled_malloc(&t->val, sizeof(float) * count));
        PGH_HIP(pooled_malloc(&t->degrees, sizeof(float) * (size_t)n));
        PGH_TRY(col_sorted.alloc(count));
        if (nnz > 0) {
            PGH_TRY(entry.alloc(count));
            PGH_TRY(entry_sorted.alloc(count));
            if (value_free) PGH_TRY(mult_t.alloc(count));
            int end_bit = 1;
            while (((int64_t)1 << end_bit) < n) ++end_bit;
            size_t temp_bytes = 0;
            PGH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, g->col, col_sorted.p, entry.p, entry_sorted.p, (int)nnz, 0, end_bit, r.stream));
            PGH_TRY(temp.alloc(temp_bytes));
            // one stable sort of (column, entry): the entries of a column keep the order of the stored CSR -- ascending rows, the copies of a
            // repeated entry in their order -- which is the order of the transposed CSR's rows
            k_gnn_iota<<<blocks_for(nnz), WG, 0, r.stream>>>(entry.p, nnz);
            PGH_HIP(hipcub::DeviceRadixSort::SortPairs(temp.p, temp_bytes, g->col, col_sorted.p, entry.p, entry_sorted.p, (int)nnz, 0, end_bit, r.stream));
            k_gnn_fill<<<blocks_for(nnz), WG, 0, r.stream>>>(entry_sorted.p, nnz, g->rowptr, n, g->val, value_free ? g->keep_mult : nullptr, t->col, t->val,
                                                           value_free ? mult_t.p : nullptr);
        }
        k_gnn_ptr<<<blocks_for(nnz + 1), WG, 0, r.stream>>>(col_sorted.p, nnz, n, t->rowptr);
        k_gnn_row_sums<<<blocks_for(n * 64), WG, 0, r.stream>>>(g->rowptr, g->val, n, t->degrees);
        PGH_HIP(hipGetLastError());
        PGH_HIP(hipStreamSynchronize(r.stream));
        PGH_TRY(finish_graph(t));
        if (value_free) {
            // M = diag(src) * W * diag(dst) read the other way round: the two scales change places
            if (g->keep_dst != nullptr) {
                PGH_HIP(pooled_malloc(&t->keep_src, sizeof(float) * (size_t)n));
                PGH_HIP(hipMemcpyAsync(t->keep_src, g->keep_dst, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, r.stream));
            }
            if (g->keep_src != nullptr) {
                PGH_HIP(pooled_malloc(&t->keep_dst, sizeof(float) * (size_t)n));
                PGH_HIP(hipMemcpyAsync(t->keep_dst, g->keep_src, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, r.stream));
            }
            PGH_HIP(hipStreamSynchronize(r.stream));
            t->keep_mult = mult_t.release();
            PGH_TRY(bsf_build(t, nullptr, t->keep_mult, t->keep_src, t->keep_dst, g->bsf.relabelled));
        } else {
            PGH_TRY(bsf_build(t, t->val, nullptr, nullptr, nullptr, g->bsf.relabelled));
        }
        // the mirrored index words now, from the partner's CSR: the transposed graph does not refer to its partner afterwards
        return mm_mirror_edge_ids(t, g);
    }();
    if (rc != 0) {
        const std::string keep = pgh_last_error();
        pgh_graph_destroy(t);
        return fail(keep);
    }
    *out = t;
    return 0;
}

extern "C" int pgh_linear_run_batch(pgh_graph_t g, pgh_mat_t v, double s0, int32_t steps, const double* a, const double* b, const double* c,
                                    pgh_mat_t out, double rate, uint64_t seed_first, int64_t seed_stride, double* loop_ms) {
    PGH_CHECK(g && v && out && c && (steps <= 0 || (a && b)), "pgh_linear_run_batch: null argument");
    PGH_CHECK(steps >= 0, "pgh_linear_run_batch: a negative number of steps");
    PGH_CHECK(rate >= 0.0 && rate < 1.0, "pgh_linear_run_batch: the rate must lie in [0, 1)");
    if (g->n_rows != g->n_cols) return declined(PGH_GNN_DECLINED, "pgh_linear_run_batch: a square matrix only");
    if (!g->bsf.enabled) return declined(PGH_GNN_DECLINED, "pgh_linear_run_batch: the graph has no blocked layout");
    if (v->b > kLanes) return declined(PGH_GNN_DECLINED, "pgh_linear_run_batch: at most 64 columns");
    if (rate > 0.0 && g->bsf_mm.mm_edge == nullptr && (g->rowptr == nullptr || g->col == nullptr))
        return declined(PGH_GNN_DECLINED, "pgh_linear_run_batch: graph_dropout needs the CSR image of the graph");
    PGH_CHECK(v->n == g->n_cols && out->n == g->n_cols && v->b == out->b && v->b >= 1, "pgh_linear_run_batch: shape mismatch");
    PGH_CHECK(v->data != out->data, "pgh_linear_run_batch: the output aliases the input");
    PGH_CHECK(std::isfinite(s0) && std::isfinite(c[0]), "pgh_linear_run_batch: a non-finite coefficient");
    for (int k = 0; k < steps; ++k)
        PGH_CHECK(std::isfinite(a[k]) && std::isfinite(b[k]) && std::isfinite(c[k + 1]), "pgh_linear_run_batch: a non-finite coefficient");
    if (loop_ms) *loop_ms = 0.0;
    if (g->n_cols == 0) return 0;
    PGH_TRY(mm_ensure_layout(g));
    Runtime& r = rt();
    const BsfFormat& f = g->bsf_mm;
    const int width = v->b, ld = (width + 3) & ~3, quads = ld / 4;
    const int64_t n_int = f.n_out;
    const size_t bytes = sizeof(float) * (size_t)n_int * ld;
    PoolBuf v_int, xg, sums, acc;
    PGH_TRY(v_int.alloc(bytes));
    PGH_TRY(xg.alloc(bytes));
    PGH_TRY(sums.alloc(bytes));
    PGH_TRY(acc.alloc(bytes));
    const f32x4* rowop = reinterpret_cast<const f32x4*>(f.mm_rowop);
    const int grid = blocks_for(n_int * quads, 8);
    LoopTimer timer;
    PGH_TRY(timer.start());
    PGH_HIP(hipMemsetAsync(sums.p, 0, bytes, r.stream));
    PGH_TRY(mm_slab_in(g, v->data, width, ld, v_int.as<float>()));
    k_gnn_close<<<grid, WG, 0, r.stream>>>(rowop, sums.as<f32x4>(), v_int.as<f32x4>(), acc.as<f32x4>(), xg.as<f32x4>(), n_int, quads, 0.f, (float)s0,
                                           (float)c[0], 1);
    for (int k = 1; k <= steps; ++k) {
        const uint64_t seed = seed_first + (uint64_t)((int64_t)(k - 1) * seed_stride);
        PGH_TRY(mm_masked_sums(g, xg.as<float>(), ld, width, sums.as<float>(), rate, seed));
        k_gnn_close<<<grid, WG, 0, r.stream>>>(rowop, sums.as<f32x4>(), v_int.as<f32x4>(), acc.as<f32x4>(), xg.as<f32x4>(), n_int, quads, (float)a[k - 1],
                                               (float)b[k - 1], (float)c[k], 0);
    }
    PGH_HIP(hipGetLastError());
    PGH_TRY(mm_slab_out(g, acc.as<float>(), width, ld, out->data));
    double ms = 0.0;
    PGH_TRY(timer.stop(&ms));                          // (waits for the loop's last launch: the caller's slab is written)
    if (loop_ms) *loop_ms = ms;
    return 0;
}

extern "C" int pgh_mat_wrap(void* device_ptr, int64_t n, int32_t b, pgh_mat_t* out) {
    PGH_TRY(ensure_init());
    PGH_CHECK(out != nullptr && n >= 0 && b >= 1, "pgh_mat_wrap: bad shape");
    PGH_CHECK(device_ptr != nullptr || n == 0, "pgh_mat_wrap: null pointer");
    pgh_mat_s* m = new pgh_mat_s();
    m->data = (float*)device_ptr;
    m->n = n;
    m->b = b;
    m->owns = false;
    *out = m;
    return 0;
}

PGH_WARM_KERNEL(k_gnn_close)
