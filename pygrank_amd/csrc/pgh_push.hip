// The first step of a seed-set PageRank run over the seeds' out-edges ("seed push").
//
// A run that starts from its personalization starts from a vector with a handful of non-zeros, and step 1 -- a * M^T x0 + b * p -- has
// a few thousand non-zero rows: the seeds and their out-neighbours.  The dense step streams the whole image for it (k_bsf_partial +
// k_pb_gather + k_pb_finish: ~206 us at scale 23, one iteration out of ~11).  Here the graph keeps its entries listed by SOURCE (the
// out-edge index, built on the first run that can use it) and step 1 is four small launches:
//   k_push_plan    one workgroup: sorts the seeds the way in listed (k_pair_scan), prefixes their out-degrees and DECIDES -- on the
//                  device, no host round trip -- whether the run qualifies: at most max_seeds seeds, no negative (or NaN) entry, at
//                  most max_edges out-edges (4096 and 2^18).  A run that qualifies is held (LoopState::done = kPushHold): the dense
//                  launches of step 1, which the host enqueues either way, return at once as they do behind a converged step.
//   k_push_expand  clears the output vector; one item per seed (its own row, contribution 0) and per out-edge (row, value * x0[seed])
//   k_push_accum   adds the items into 64-bit fixed-point row sums (scaled from the step's largest contribution, as k_pb_finish scales
//                  its hub pieces: integer addition, so the order of arrival does not show) and elects the smallest item of every row
//   k_push_finish  the elected item of a row writes what a finish launch writes: y, the row's slot of the next gather vector, and the
//                  partial sums of sum(y), sum(deg * y), sum(p) -- per workgroup, items in index order, so every bit repeats
// The residual and the close of step 1 take the loop's path for a step whose residual is not fused (k_step_residual, then the close
// with res_mode 2 / 0); the in-kernel residual goes on from step 2.  A run that does not qualify runs exactly what it ran before.
//
// Step 2's cold tail ("seed push 2").  After a pushed step 1 the iterate still has a few thousand non-zero rows, hubs among them: the hot
// half of step 2 (k_bsf_partial) has to stream, a push of all of it would be millions of atomic items aimed at hub rows.  But the COLD
// sources among those rows -- the ones whose gathers the cold image serves -- have a few ten thousand out-edges between them, and the
// cold image (k_pb_gather + the stream half of k_pb_finish) moves 33 M products for them at scale 23, nearly all zero.  So:
//   k_push_finish     lists every row it writes that is a cold source with out-edges: caller id and value in gather form, any order
//   k_push_plan2      one workgroup, behind step 2's k_bsf_partial (which must not see the hold): prefixes the listed sources' out-degrees
//                     and decides -- step 1 was pushed, at most C2 items, no negative (or NaN) entry.  A run that qualifies is held again
//   k_push_expand2    closes the cross-tile segments of the hot half (phase A, which passes, does it otherwise); one item per out-edge
//   k_push_accum2     adds the items into the same fixed-point scratch; no owners are elected
//   k_pb_gather, k_pb_finish     enqueued either way; they pass under the hold
//   k_bsf_combine_tail (pgh_bsf.hip)   the epilogue of a graph without a cold image, plus the row's scratch word, which it re-arms
// then k_step_residual behind the tail's gate and a close (res_mode 2 / 0) that lifts the hold; the in-kernel residual goes on from
// step 3.  A run whose tail does not qualify finds the flag clear: the new launches return at once and step 2 runs as it did.
// PGH_SEED_PUSH2=0 enqueues none of this, PGH_SEED_PUSH_C2 sets the bound on the items.
#include "pgh_kernels.h"

#include <chrono>
#include <climits>
#include <hipcub/hipcub.hpp>

namespace pgh {

namespace {

constexpr int kPushMaxSeeds = 4096;          // k_push_plan sorts the seeds in LDS
constexpr int kPushMaxEdges = 1 << 20;       // capacity of the item lists (PGH_SEED_PUSH_C may raise the bound up to it)
// the bound on the seeds' out-edges: hub seeds send most of their items to the same few rows, and the step loses to the dense one from
// about half a million items on (profiles/seed_push/push_measure_hubs_scale23.log: the largest source alone -100 us, with four / eight /
// twelve of the next largest -33 / +20 / +63 us)
constexpr int kPushDefaultEdges = 1 << 18;
// the bound on the items of step 2's cold tail (PGH_SEED_PUSH_C2), from profiles/seed_push2/push2_bound_scale23.log: against the dense
// tail the pushed one measured -40 / -36 / -27 / -19 us per run at 10 / 17 / 53 / 77 thousand items and +10 / +35 / +50 / +145 us at
// 183 / 305 / 388 / 707 thousand (medians of two blocks of eight runs each way; the dense blocks' medians agree to 4 us, single dense
// runs scatter by 17 us).  2^16 is the largest power of two with a gain above that scatter; at 2^17 the interpolated gain is ~5 us.
constexpr int kPushDefaultTail = 1 << 16;
constexpr int kPushCtlBytes = 192;           // PushIndex::ctl: {PushCtl, gate} of step 1, {PushCtl, gate} of step 2's tail, the list's counter
constexpr int kPushItemBits = 21;            // kPushMaxSeeds + kPushMaxEdges < 2^21 items
constexpr int kPushFixBits = 62 - kPushItemBits;     // bits of one item in the fixed-point sums: a row of 2^21 items stays below 2^62
constexpr int kPushHold = 3;                 // LoopState::done while the dense launches of a pushed step 1 pass
constexpr int kPlanThreads = 1024;

struct PushCtl {
    int          qualified;
    int          nseeds;
    int          total_items;      // nseeds + out-edges of the seeds
    unsigned int cmax_bits;        // bit pattern of the largest |contribution| (k_push_expand)
};

template <typename T>
struct Tmp {
    T* p = nullptr;
    ~Tmp() {
        if (p) (void)pooled_free(p);
    }
    bool alloc(size_t count) { return pooled_malloc(&p, sizeof(T) * (count > 0 ? count : 1)) == hipSuccess; }
    T* release() {
        T* q = p;
        p = nullptr;
        return q;
    }
};

int blocks_of(int64_t n, int per_block = 256) {
    int64_t b = (n + per_block - 1) / per_block;
    const int64_t cap = (int64_t)rt().num_cus * 16;
    if (b > cap) b = cap;
    return (int)(b < 1 ? 1 : b);
}

// ------------------------------------------------------------------------------------------------- index build
__global__ void k_push_iota(int32_t* __restrict__ v, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] = (int32_t)i;
}

// run-length pass over the sorted sources: out_ptr[s] = first position whose source is >= s
__global__ void k_push_ptr(const int32_t* __restrict__ src_sorted, int64_t nnz, int64_t n_rows, int32_t* __restrict__ out_ptr) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= nnz; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t prev = i > 0 ? (int64_t)src_sorted[i - 1] : -1;
        const int64_t cur = i < nnz ? (int64_t)src_sorted[i] : n_rows;
        for (int64_t s = prev + 1; s <= cur && s <= n_rows; ++s) out_ptr[s] = (int32_t)i;
    }
}

// entry e of CSR(M^T) at position i of its source's list: its row in internal ids, the value the image multiplies with
__global__ void k_push_fill(const int32_t* __restrict__ entry_sorted, int64_t nnz, const int32_t* __restrict__ rowptr, int64_t n_cols,
                            const int32_t* __restrict__ iperm, const float* __restrict__ val, const int32_t* __restrict__ mult,
                            int32_t* __restrict__ out_row, float* __restrict__ out_val) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t e = entry_sorted[i];
        int64_t lo = 0, hi = n_cols - 1;                     // the largest row r with rowptr[r] <= e (empty rows share their successor's start)
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (rowptr[mid] <= e) lo = mid;
            else hi = mid - 1;
        }
        out_row[i] = iperm[lo];
        out_val[i] = mult != nullptr ? (float)mult[e] : val[e];
    }
}

__global__ void k_push_fill_i32(int32_t* __restrict__ v, int64_t n, int32_t value) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] = value;
}

// ------------------------------------------------------------------------------------------------- the step
__global__ __launch_bounds__(kPlanThreads) void k_push_plan(const int32_t* __restrict__ list, const int* __restrict__ count,
                                                            const int32_t* __restrict__ iperm, const float* __restrict__ v_int,
                                                            const int32_t* __restrict__ out_ptr, int max_seeds, int max_edges,
                                                            PushCtl* __restrict__ ctl, LoopState* __restrict__ gate, LoopState* __restrict__ state,
                                                            int32_t* __restrict__ seed_out, int32_t* __restrict__ off_out, int* __restrict__ tail_count) {
    __shared__ int s_key[kPushMaxSeeds];
    __shared__ long long s_scan[kPlanThreads];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int n = *count;
    if (tid == 0) {                                          // the list k_push_finish fills for step 2's cold tail: {count, bad, items}
        tail_count[0] = 0, tail_count[1] = 0;
        *reinterpret_cast<unsigned long long*>(tail_count + 2) = 0ULL;
    }
    if (n < 1 || n > max_seeds) {                            // (workgroup-uniform; a list that overflowed is never read)
        if (tid == 0) {
            ctl->qualified = 0, ctl->nseeds = 0, ctl->total_items = 0, ctl->cmax_bits = 0u;
            gate->done = 1;
        }
        return;
    }
    if (tid == 0) s_bad = 0;
    int m = 1;
    while (m < n) m <<= 1;
    for (int i = tid; i < m; i += kPlanThreads) s_key[i] = i < n ? list[i] : INT_MAX;
    __syncthreads();
    // the scan lists the seeds in order of arrival: ascending ids make the items -- and every sum over them -- repeat
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < m; i += kPlanThreads) {
                const int partner = i ^ j;
                if (partner > i) {
                    const int a = s_key[i], b = s_key[partner];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) s_key[i] = b, s_key[partner] = a;
                }
            }
            __syncthreads();
        }
    constexpr int PER = kPushMaxSeeds / kPlanThreads;
    int deg[PER];
    long long local = 0;
    bool bad = false;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int i = PER * tid + u;
        deg[u] = 0;
        if (i < n) {
            const int id = s_key[i];
            deg[u] = out_ptr[id + 1] - out_ptr[id];
            const float pv = v_int[iperm[id]];
            bad = bad || !(pv >= 0.f);                       // a signed personalization (or a NaN) takes the dense step
        }
        local += deg[u];
    }
    if (bad) s_bad = 1;
    s_scan[tid] = local;
    __syncthreads();
    for (int off = 1; off < kPlanThreads; off <<= 1) {
        const long long t = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += t;
        __syncthreads();
    }
    const long long total = s_scan[kPlanThreads - 1];
    const bool qualified = s_bad == 0 && total <= (long long)max_edges;
    if (qualified) {
        long long run = s_scan[tid] - local;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int i = PER * tid + u;
            if (i < n) {
                seed_out[i] = s_key[i];
                off_out[i] = (int32_t)run;
            }
            run += deg[u];
        }
        if (tid == 0) off_out[n] = (int32_t)total;
    }
    if (tid == 0) {
        ctl->qualified = qualified ? 1 : 0;
        ctl->nseeds = n;
        ctl->total_items = qualified ? n + (int)total : 0;
        ctl->cmax_bits = 0u;
        gate->scale = state->scale;
        gate->err = 0.0, gate->sum = 0.0;
        gate->steps = 0, gate->converged = 0, gate->pad = 0;
        gate->done = qualified ? 0 : 1;                      // the residual launch of the pushed step runs only behind one
        if (qualified) {
            state->done = kPushHold;                         // the dense launches of step 1 pass (k_push_close lifts it)
            state->pad = 1;                                  // what the host reads at the end of the run: step 1 was pushed
        }
    }
}

struct PushStepArgs {
    const PushCtl* ctl;
    const int32_t* seed;
    const int32_t* off;
    const int32_t* iperm;
    const float*   v_int;
    const float*   src_scale;      // or null
    const float*   dst_scale;      // or null
    const float*   deg;            // row sums of M, internal ids (the fused residual's next prediction), or null
    const int32_t* out_ptr;
    const int32_t* out_row;
    const float*   out_val;
    int32_t*       item_row;
    float*         item_val;
    long long*     acc;
    int32_t*       owner;
    float*         y;
    float*         xg_out;         // or null
    int64_t        n_int;
    int            xg_blk, xg_live;
    double         a, b;
    const LoopState* state;
    double*        part_sum;
    double*        part_t;
    double*        part_d;
    double*        part_r;
    // step 2's cold tail: the list k_push_finish fills (tail_src null: none) and k_push_expand2 reads
    const int32_t* perm;
    int32_t*       tail_src;
    float*         tail_xg;
    int32_t*       tail_off;
    int*           tail_count;
    int            tail_blk, tail_hot, tail_cap;
};

__global__ __launch_bounds__(256) void k_push_expand(PushStepArgs p, PushCtl* __restrict__ ctl_rw) {
    if (p.ctl->qualified == 0) return;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    // every row the step does not touch is zero (the dense step writes them all; the pool's vectors are not cleared)
    if ((reinterpret_cast<uintptr_t>(p.y) & 15) == 0) {
        float4* y4 = reinterpret_cast<float4*>(p.y);
        const int64_t body = p.n_int >> 2;
        for (int64_t i = tid; i < body; i += stride) y4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t i = (body << 2) + tid; i < p.n_int; i += stride) p.y[i] = 0.f;
    } else {
        for (int64_t i = tid; i < p.n_int; i += stride) p.y[i] = 0.f;
    }
    const int n = p.ctl->nseeds, total = p.ctl->total_items;
    unsigned int biggest = 0u;
    for (int64_t i = tid; i < total; i += stride) {
        int row;
        float c = 0.f;
        if (i < n) {
            row = p.iperm[p.seed[i]];
        } else {
            const int j = (int)i - n;
            int lo = 0, hi = n - 1;                          // the seed whose range holds edge j: the largest s with off[s] <= j
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (p.off[mid] <= j) lo = mid;
                else hi = mid - 1;
            }
            const int old = p.seed[lo];
            const int e = p.out_ptr[old] + (j - p.off[lo]);
            const int si = p.iperm[old];
            float xs = p.v_int[si];                          // x0 = p / |p| in the gather vector's form, as the way in wrote it
            if (p.src_scale != nullptr) xs *= p.src_scale[si];
            row = p.out_row[e];
            c = p.out_val[e] * xs;
        }
        p.item_row[i] = row;
        p.item_val[i] = c;
        const unsigned int bits = __float_as_uint(fabsf(c));
        biggest = bits > biggest ? bits : biggest;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned int other = (unsigned int)__shfl_down((int)biggest, off, 64);
        biggest = other > biggest ? other : biggest;
    }
    if ((threadIdx.x & 63) == 0 && biggest != 0u) atomicMax(&ctl_rw->cmax_bits, biggest);
}

// |contribution| <= cmax < 2^e: an item gets kPushFixBits bits
__device__ __forceinline__ int push_exponent(unsigned int cmax_bits) { return (int)(cmax_bits >> 23) - 126; }

__global__ __launch_bounds__(256) void k_push_accum(PushStepArgs p) {
    if (p.ctl->qualified == 0) return;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const int total = p.ctl->total_items;
    const unsigned int cmax = p.ctl->cmax_bits;
    const bool finite = cmax < 0x7f800000u;
    const double S = __longlong_as_double((long long)(1023 + kPushFixBits - push_exponent(cmax)) << 52);
    for (int64_t i = tid; i < total; i += stride) {
        const int row = p.item_row[i];
        if (finite) {
            const long long q = __double2ll_rn((double)p.item_val[i] * S);
            if (q != 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.acc + row), (unsigned long long)q);
        }
        atomicMin(p.owner + row, (int)i);
    }
}

// (the list of step 2's cold tail is staged per workgroup: one reservation in the global list, one addition to the total of the
// out-degrees -- thousands of atomics on one word of memory take their turns)
constexpr int kPushGrid = 1024;              // push_partials()
constexpr int kListPerGroup = 256 * ((kPushMaxSeeds + kPushMaxEdges + kPushGrid * 256 - 1) / (kPushGrid * 256));      // a workgroup's items
__global__ __launch_bounds__(256) void k_push_finish(PushStepArgs p) {
    __shared__ double s_red[4];
    __shared__ int s_src[kListPerGroup];
    __shared__ float s_xg[kListPerGroup];
    __shared__ unsigned long long s_deg;
    __shared__ int s_n, s_bad, s_base;
    if (p.ctl->qualified == 0) return;
    if (threadIdx.x == 0) s_n = 0, s_bad = 0, s_deg = 0ULL;
    __syncthreads();
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const int total = p.ctl->total_items;
    const unsigned int cmax = p.ctl->cmax_bits;
    const bool finite = cmax < 0x7f800000u;
    const double inv_S = __longlong_as_double((long long)(1023 - kPushFixBits + push_exponent(cmax)) << 52);
    const float a_eff = (float)(p.a * p.state->scale);       // the factors as the epilogue forms them (epi_apply)
    const float b_eff = (float)p.b;
    double sum_y = 0.0, sum_t = 0.0, sum_p = 0.0;
    for (int64_t i = tid; i < total; i += stride) {
        const int row = p.item_row[i];
        if (p.owner[row] != (int)i) continue;               // one item per row finishes it; the scratch goes back to its idle state
        double sum = finite ? (double)p.acc[row] * inv_S : __longlong_as_double(0x7ff8000000000000LL);
        p.acc[row] = 0;
        p.owner[row] = INT_MAX;
        if (p.dst_scale != nullptr) sum *= (double)p.dst_scale[row];
        const float pv = p.v_int[row];
        const float y = a_eff * (float)sum + b_eff * pv;
        p.y[row] = y;
        if (p.xg_out != nullptr) {
            const int slot = xg_slot(row, p.xg_blk, p.xg_live);
            if (slot >= 0) p.xg_out[slot] = y * p.src_scale[row];
        }
        if (p.tail_src != nullptr) {                         // a cold source with out-edges: step 2's cold tail may push it
            int b = 0;
#pragma unroll
            for (int k = 1; k < 8; ++k) b += (row >= k * p.tail_blk) ? 1 : 0;
            const float xg = p.src_scale != nullptr ? y * p.src_scale[row] : y;
            if (row - b * p.tail_blk >= p.tail_hot && !(xg == 0.f)) {
                const int old = p.perm[row];
                const int d = p.out_ptr[old + 1] - p.out_ptr[old];
                if (d > 0) {
                    const int at = atomicAdd(&s_n, 1);       // (at most one row per item: the stage holds them all)
                    if (at < kListPerGroup) s_src[at] = old, s_xg[at] = xg;
                    atomicAdd(&s_deg, (unsigned long long)d);
                    if (!(xg >= 0.f)) s_bad = 1;             // a negative entry (or a NaN) takes the dense tail
                }
            }
        }
        sum_y += (double)y;
        if (p.deg != nullptr) sum_t += (double)p.deg[row] * (double)y;
        sum_p += (double)pv;
    }
    const double by = block_reduce_256<0>(sum_y, s_red);
    __syncthreads();
    const double bt = block_reduce_256<0>(sum_t, s_red);
    __syncthreads();
    const double bp = block_reduce_256<0>(sum_p, s_red);
    if (threadIdx.x == 0) {
        p.part_sum[blockIdx.x] = by;
        p.part_t[blockIdx.x] = bt;
        p.part_d[blockIdx.x] = bp;
        p.part_r[blockIdx.x] = 0.0;
    }
    __syncthreads();
    const int listed = min(s_n, kListPerGroup);
    if (p.tail_src != nullptr && listed > 0) {               // (workgroup-uniform)
        if (threadIdx.x == 0) {
            s_base = atomicAdd(p.tail_count, listed);
            atomicAdd(reinterpret_cast<unsigned long long*>(p.tail_count + 2), s_deg);
            if (s_bad) atomicOr(p.tail_count + 1, 1);
        }
        __syncthreads();
        for (int k = threadIdx.x; k < listed; k += 256) {
            const int at = s_base + k;
            if (at < p.tail_cap) p.tail_src[at] = s_src[k], p.tail_xg[at] = s_xg[k];
        }
    }
}

// the close of step 1: the pushed step's (the hold is lifted first) or, for a run that did not qualify, the dense step's
__global__ __launch_bounds__(WG) void k_push_close(const PushCtl* __restrict__ ctl, PendingClose dense, PendingClose pushed) {
    __shared__ double s_red[16];
    if (ctl->qualified == 0) {
        if (dense.state->done) return;
        (void)run_pending_close(dense, s_red);
        return;
    }
    if (threadIdx.x == 0) pushed.state->done = 0;
    __syncthreads();
    (void)run_pending_close(pushed, s_red);
}

// ------------------------------------------------------------------------------------------------- step 2's cold tail
// One workgroup behind step 2's block partial sums: the prefix of the listed sources' out-degrees (thread t takes a run of the list; the
// order of the list shows in no result: the items are added as integers) and the decision.  ctl1: step 1's words.
__global__ __launch_bounds__(kPlanThreads) void k_push_plan2(const PushCtl* __restrict__ ctl1, const int* __restrict__ count,
                                                             const int32_t* __restrict__ src, const float* __restrict__ xg,
                                                             const int32_t* __restrict__ out_ptr, int max_items, int cap,
                                                             PushCtl* __restrict__ ctl, LoopState* __restrict__ gate, LoopState* __restrict__ state,
                                                             int32_t* __restrict__ off_out) {
    __shared__ long long s_scan[kPlanThreads];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int n = *count;
    // (workgroup-uniform.  A run that ended or paused in step 1, a dense step 1, a list that overflowed, more items than allowed -- the
    // list's total, so that a run far above the bound pays no prefix --, a negative entry: not read)
    const unsigned long long listed_items = *reinterpret_cast<const unsigned long long*>(count + 2);
    if (ctl1->qualified == 0 || state->done != 0 || n > cap || listed_items > (unsigned long long)max_items || count[1] != 0) {
        if (tid == 0) {
            ctl->qualified = 0, ctl->nseeds = 0, ctl->cmax_bits = 0u;
            ctl->total_items = (int)(listed_items < (unsigned long long)INT_MAX ? listed_items : (unsigned long long)INT_MAX);
            gate->done = 1;
        }
        return;
    }
    if (tid == 0) s_bad = 0;
    const int per = (n + kPlanThreads - 1) / kPlanThreads;
    const int lo = min(n, tid * per), hi = min(n, lo + per);
    long long local = 0;
    bool bad = false;
    for (int i = lo; i < hi; ++i) {
        const int id = src[i];
        local += out_ptr[id + 1] - out_ptr[id];
        bad = bad || !(xg[i] >= 0.f);                        // a negative entry (or a NaN) takes the dense step
    }
    s_scan[tid] = local;
    __syncthreads();
    if (bad) s_bad = 1;
    for (int off = 1; off < kPlanThreads; off <<= 1) {
        const long long t = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += t;
        __syncthreads();
    }
    const long long total = s_scan[kPlanThreads - 1];
    const bool qualified = s_bad == 0 && total <= (long long)max_items;
    if (qualified) {
        long long run = s_scan[tid] - local;
        for (int i = lo; i < hi; ++i) {
            const int id = src[i];
            off_out[i] = (int32_t)run;
            run += out_ptr[id + 1] - out_ptr[id];
        }
        if (tid == 0) off_out[n] = (int32_t)total;
    }
    if (tid == 0) {
        ctl->qualified = qualified ? 1 : 0;
        ctl->nseeds = n;
        ctl->total_items = (int)(total < (long long)INT_MAX ? total : (long long)INT_MAX);      // (read behind `qualified` only)
        ctl->cmax_bits = 0u;
        gate->scale = state->scale;
        gate->err = 0.0, gate->sum = 0.0;
        gate->steps = 0, gate->converged = 0, gate->pad = 0;
        gate->done = qualified ? 0 : 1;                      // the epilogue and the residual launch of the pushed tail run only behind one
        if (qualified) {
            state->done = kPushHold;                         // the cold-image launches of step 2 pass (the close lifts it)
            state->pad |= 2;                                 // what the host reads at the end of the run: step 2's cold tail was pushed
        }
    }
}

// p.ctl: the tail's words.  One item per out-edge of a listed source; y is not cleared (the epilogue writes every row) and nobody is elected.
__global__ __launch_bounds__(256) void k_push_expand2(PushStepArgs p, PushCtl* __restrict__ ctl_rw, FixView fix) {
    if (p.ctl->qualified == 0) return;
    // the cross-tile segments of the block partial sums: phase A of the cold image closes them, and it passes under the hold
    bsf_fixup_tiles(fix, blockIdx.x * 256, gridDim.x * 256);
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const int n = p.ctl->nseeds, total = p.ctl->total_items;
    unsigned int biggest = 0u;
    for (int64_t i = tid; i < total; i += stride) {
        const int j = (int)i;
        int lo = 0, hi = n - 1;                              // the source whose range holds edge j: the largest s with off[s] <= j
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (p.tail_off[mid] <= j) lo = mid;
            else hi = mid - 1;
        }
        const int e = p.out_ptr[p.tail_src[lo]] + (j - p.tail_off[lo]);
        const float c = p.out_val[e] * p.tail_xg[lo];
        p.item_row[i] = p.out_row[e];
        p.item_val[i] = c;
        const unsigned int bits = __float_as_uint(fabsf(c));
        biggest = bits > biggest ? bits : biggest;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned int other = (unsigned int)__shfl_down((int)biggest, off, 64);
        biggest = other > biggest ? other : biggest;
    }
    // (a wavefront that cannot raise the maximum stays away from it: atomics on one word take their turns, and with a quarter of a
    // million items every wavefront of the grid has one)
    if ((threadIdx.x & 63) == 0 && biggest > __hip_atomic_load(&ctl_rw->cmax_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(&ctl_rw->cmax_bits, biggest);
}

// The items of a pushed cold tail, added into the row scratch: k_push_accum without the election.  Integer sums: no order shows.  Items
// that are not finite mark their row instead (k_bsf_combine_tail).  (A workgroup summing its items by row in an LDS table first was
// measured: 16 us instead of 5 at the bench's 10-50 thousand items, and no better at a quarter of a million.)
__global__ __launch_bounds__(256) void k_push_accum2(PushStepArgs p) {
    if (p.ctl->qualified == 0) return;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const int total = p.ctl->total_items;
    const unsigned int cmax = p.ctl->cmax_bits;
    const bool finite = cmax < 0x7f800000u;
    const double S = __longlong_as_double((long long)(1023 + kPushFixBits - push_exponent(cmax)) << 52);
    for (int64_t i = tid; i < total; i += stride) {
        const int row = p.item_row[i];
        if (finite) {
            const long long q = __double2ll_rn((double)p.item_val[i] * S);
            if (q != 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.acc + row), (unsigned long long)q);
        } else {
            p.acc[row] = kPushNotFinite;
        }
    }
}

int env_or(const char* name, int fallback) {
    const char* s = getenv(name);
    return s != nullptr ? atoi(s) : fallback;
}

}  // namespace

PGH_WARM_KERNEL(k_push_plan)

bool push_switched_on() { return env_or("PGH_SEED_PUSH", 1) != 0; }     // read per run: a caller may compare both paths in one process

void push_destroy(pgh_graph_s* g) {
    PushIndex& x = g->push;
    (void)pooled_free(x.out_ptr);
    (void)pooled_free(x.out_row);
    (void)pooled_free(x.out_val);
    (void)pooled_free(x.acc);
    (void)pooled_free(x.owner);
    (void)pooled_free(x.item_row);
    (void)pooled_free(x.item_val);
    (void)pooled_free(x.seed);
    (void)pooled_free(x.seed_off);
    (void)pooled_free(x.ctl);
    (void)pooled_free(x.tail_src);
    (void)pooled_free(x.tail_xg);
    (void)pooled_free(x.tail_off);
    g->device_bytes -= x.device_bytes;
    const bool failed = x.failed;
    x = PushIndex();
    x.failed = failed;
}

// Builds the out-edge index and the step's scratch on first use.  Returns 0 with g->push.out_ptr == nullptr when the graph cannot have
// one (no memory for it: the run takes the dense step and the build is not tried again).
int push_ensure(pgh_graph_s* g) {
    PushIndex& x = g->push;
    if (x.out_ptr != nullptr || x.failed) return 0;
    const BsfFormat& f = g->bsf;
    const bool value_free = f.val == nullptr && f.pb.val == nullptr && g->keep_mult != nullptr;
    if (g->rowptr == nullptr || g->col == nullptr || f.iperm == nullptr || g->n_rows != g->n_cols || (!value_free && g->val == nullptr)) {
        x.failed = true;
        return 0;
    }
    Runtime& r = rt();
    PGH_HIP(hipStreamSynchronize(r.stream));
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t nnz = g->nnz, n = g->n_rows, n_int = f.n_out;
    const int items = kPushMaxSeeds + kPushMaxEdges;
    Tmp<int32_t> out_ptr, out_row, owner, item_row, seed, seed_off, src_sorted, entry, entry_sorted, tail_src, tail_off;
    Tmp<float> out_val, item_val, tail_xg;
    Tmp<long long> acc;
    Tmp<char> ctl, temp;
    bool ok = out_ptr.alloc(n + 1) && out_row.alloc(nnz) && out_val.alloc(nnz) && acc.alloc(n_int) && owner.alloc(n_int) && item_row.alloc(items) &&
              item_val.alloc(items) && seed.alloc(kPushMaxSeeds) && seed_off.alloc(kPushMaxSeeds + 1) && ctl.alloc(kPushCtlBytes) &&
              tail_src.alloc(kPushMaxEdges) && tail_xg.alloc(kPushMaxEdges) && tail_off.alloc(kPushMaxEdges + 1) && src_sorted.alloc(nnz) && entry.alloc(nnz) && entry_sorted.alloc(nnz);
    size_t temp_bytes = 0;
    int end_bit = 1;
    while (((int64_t)1 << end_bit) < n) ++end_bit;
    if (ok && nnz > 0) {
        PGH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, g->col, src_sorted.p, entry.p, entry_sorted.p, (int)nnz, 0, end_bit, r.stream));
        ok = temp.alloc(temp_bytes);
    }
    if (!ok) {                                               // (the pool has dropped its idle blocks before it gives up)
        (void)hipGetLastError();
        x.failed = true;
        return 0;
    }
    if (nnz > 0) {
        // one stable sort of (source, entry): a source's entries keep the order of CSR(M^T), ascending rows
        k_push_iota<<<blocks_of(nnz), 256, 0, r.stream>>>(entry.p, nnz);
        PGH_HIP(hipcub::DeviceRadixSort::SortPairs(temp.p, temp_bytes, g->col, src_sorted.p, entry.p, entry_sorted.p, (int)nnz, 0, end_bit, r.stream));
        k_push_fill<<<blocks_of(nnz), 256, 0, r.stream>>>(entry_sorted.p, nnz, g->rowptr, g->n_cols, f.iperm, value_free ? nullptr : g->val,
                                                          value_free ? g->keep_mult : nullptr, out_row.p, out_val.p);
    }
    k_push_ptr<<<blocks_of(nnz + 1), 256, 0, r.stream>>>(src_sorted.p, nnz, n, out_ptr.p);
    PGH_HIP(hipMemsetAsync(acc.p, 0, sizeof(long long) * (size_t)(n_int > 0 ? n_int : 1), r.stream));
    k_push_fill_i32<<<blocks_of(n_int), 256, 0, r.stream>>>(owner.p, n_int, INT_MAX);
    PGH_HIP(hipMemsetAsync(ctl.p, 0, kPushCtlBytes, r.stream));
    PGH_HIP(hipGetLastError());
    PGH_HIP(hipStreamSynchronize(r.stream));
    x.out_ptr = out_ptr.release(), x.out_row = out_row.release(), x.out_val = out_val.release();
    x.acc = acc.release(), x.owner = owner.release();
    x.item_row = item_row.release(), x.item_val = item_val.release();
    x.seed = seed.release(), x.seed_off = seed_off.release();
    x.ctl = ctl.release();
    x.tail_src = tail_src.release(), x.tail_xg = tail_xg.release(), x.tail_off = tail_off.release();
    x.max_seeds = kPushMaxSeeds, x.max_edges = kPushMaxEdges;
    x.device_bytes = 4 * (n + 1) + 8 * (nnz > 0 ? nnz : 1) + 12 * (n_int > 0 ? n_int : 1) + 8 * (int64_t)items + 4 * (2 * kPushMaxSeeds + 1) + kPushCtlBytes +
                     4 * (3 * (int64_t)kPushMaxEdges + 1);
    g->device_bytes += x.device_bytes;
    build_phase_add("seed push: out-edge index (first use)", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}

static_assert(sizeof(PushCtl) + sizeof(LoopState) <= 64, "PushIndex::ctl holds both");

namespace {
PushCtl* tail_ctl(const PushIndex& x) { return reinterpret_cast<PushCtl*>(reinterpret_cast<char*>(x.ctl) + 64); }
LoopState* tail_gate_of(const PushIndex& x) { return reinterpret_cast<LoopState*>(reinterpret_cast<char*>(x.ctl) + 64 + sizeof(PushCtl)); }
int* tail_counter(const PushIndex& x) { return reinterpret_cast<int*>(reinterpret_cast<char*>(x.ctl) + 128); }
}  // namespace

// Enqueues the plan and the three launches of the pushed step (all of them return at once for a run that does not qualify).
// ep: the step's epilogue operands in internal ids (v, y, the next gather vector); deg: null unless the close predicts from it;
// partials: rt().d_partials (regions 0, 2, 3, 4 receive push_partials() sums each).  list_tail: k_push_finish lists the cold sources it
// writes for step 2's cold tail (push_launch_tail).
int push_launch_step(pgh_graph_s* g, const EpiParams& ep, const int32_t* seed_list, const int* seed_count, const float* deg, LoopState* state,
                     bool list_tail) {
    PushIndex& x = g->push;
    const BsfFormat& f = g->bsf;
    Runtime& r = rt();
    PushCtl* ctl = reinterpret_cast<PushCtl*>(x.ctl);
    LoopState* gate = reinterpret_cast<LoopState*>(reinterpret_cast<char*>(x.ctl) + sizeof(PushCtl));
    int max_seeds = env_or("PGH_SEED_PUSH_K", x.max_seeds), max_edges = env_or("PGH_SEED_PUSH_C", kPushDefaultEdges);
    max_seeds = max_seeds < 0 ? 0 : (max_seeds > x.max_seeds ? x.max_seeds : max_seeds);
    max_edges = max_edges < 0 ? 0 : (max_edges > x.max_edges ? x.max_edges : max_edges);
    k_push_plan<<<1, kPlanThreads, 0, r.stream>>>(seed_list, seed_count, f.iperm, ep.v, x.out_ptr, max_seeds, max_edges, ctl, gate, state, x.seed,
                                                  x.seed_off, tail_counter(x));
    PushStepArgs p{};
    p.ctl = ctl;
    p.seed = x.seed, p.off = x.seed_off, p.iperm = f.iperm;
    p.v_int = ep.v;
    p.src_scale = ep.xg_out != nullptr ? ep.src_scale : nullptr;
    p.dst_scale = f.dst_scale;
    p.deg = deg;
    p.out_ptr = x.out_ptr, p.out_row = x.out_row, p.out_val = x.out_val;
    p.item_row = x.item_row, p.item_val = x.item_val;
    p.acc = x.acc, p.owner = x.owner;
    p.y = ep.y;
    p.xg_out = ep.xg_out;
    p.n_int = f.n_out;
    p.xg_blk = ep.xg_blk, p.xg_live = ep.xg_live;
    p.a = ep.a, p.b = ep.b;
    p.state = state;
    p.part_sum = r.d_partials;
    p.part_r = r.d_partials + 2 * kMaxPartials;
    p.part_d = r.d_partials + 3 * kMaxPartials;
    p.part_t = r.d_partials + 4 * kMaxPartials;
    if (list_tail) {
        p.perm = f.perm;
        p.tail_src = x.tail_src, p.tail_xg = x.tail_xg, p.tail_count = tail_counter(x);
        p.tail_blk = f.blk_size, p.tail_hot = f.pb.hot, p.tail_cap = x.max_edges;
    }
    const int grid = push_partials();
    k_push_expand<<<grid, 256, 0, r.stream>>>(p, ctl);
    k_push_accum<<<grid, 256, 0, r.stream>>>(p);
    k_push_finish<<<grid, 256, 0, r.stream>>>(p);
    PGH_HIP(hipGetLastError());
    return 0;
}

int push_partials() { return kPushGrid; }

const LoopState* push_gate(const pgh_graph_s* g) {
    return reinterpret_cast<const LoopState*>(reinterpret_cast<const char*>(g->push.ctl) + sizeof(PushCtl));
}

int push_launch_close(pgh_graph_s* g, const PendingClose& dense, const PendingClose& pushed) {
    k_push_close<<<1, WG, 0, rt().stream>>>(reinterpret_cast<const PushCtl*>(g->push.ctl), dense, pushed);
    PGH_HIP(hipGetLastError());
    return 0;
}

// ---- step 2's cold tail
bool push_tail_switched_on() { return env_or("PGH_SEED_PUSH2", 1) != 0; }      // read per run, like PGH_SEED_PUSH

int push_launch_tail(pgh_graph_s* g, LoopState* state) {
    PushIndex& x = g->push;
    Runtime& r = rt();
    PushCtl* ctl = tail_ctl(x);
    int max_items = env_or("PGH_SEED_PUSH_C2", kPushDefaultTail);
    max_items = max_items < 0 ? 0 : (max_items > x.max_edges ? x.max_edges : max_items);
    k_push_plan2<<<1, kPlanThreads, 0, r.stream>>>(reinterpret_cast<const PushCtl*>(x.ctl), tail_counter(x), x.tail_src, x.tail_xg, x.out_ptr,
                                                   max_items, x.max_edges, ctl, tail_gate_of(x), state, x.tail_off);
    PushStepArgs p{};
    p.ctl = ctl;
    p.out_ptr = x.out_ptr, p.out_row = x.out_row, p.out_val = x.out_val;
    p.item_row = x.item_row, p.item_val = x.item_val;
    p.acc = x.acc;
    p.tail_src = x.tail_src, p.tail_xg = x.tail_xg, p.tail_off = x.tail_off;
    const int grid = push_partials();
    k_push_expand2<<<grid, 256, 0, r.stream>>>(p, ctl, bsf_fix_view(g->bsf));
    k_push_accum2<<<grid, 256, 0, r.stream>>>(p);
    PGH_HIP(hipGetLastError());
    return 0;
}

int push_launch_tail_combine(pgh_graph_s* g, const EpiParams& ep, const float* deg, const IsoTail& iso, int* num_partials) {
    PushIndex& x = g->push;
    Runtime& r = rt();
    PushTailView t{};
    t.gate = tail_gate_of(x);
    t.acc = x.acc;
    t.cmax_bits = &tail_ctl(x)->cmax_bits;
    t.fix_bits = kPushFixBits;
    t.deg = deg;
    t.part_r = r.d_partials + 2 * kMaxPartials;
    t.part_d = r.d_partials + 3 * kMaxPartials;
    t.part_t = r.d_partials + 4 * kMaxPartials;
    return bsf_launch_combine_tail(g, ep, t, iso, num_partials);
}

const LoopState* push_tail_gate(const pgh_graph_s* g) { return tail_gate_of(g->push); }

bool push_tail_census(const pgh_graph_s* g, int* sources, int* items) {
    PushCtl h{};
    int listed = 0;
    if (hipMemcpy(&h, tail_ctl(g->push), sizeof(h), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&listed, tail_counter(g->push), sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return false;
    *sources = listed;
    *items = h.total_items;
    return h.qualified != 0;
}

int push_launch_tail_close(pgh_graph_s* g, const PendingClose& dense, const PendingClose& pushed) {
    k_push_close<<<1, WG, 0, rt().stream>>>(tail_ctl(g->push), dense, pushed);
    PGH_HIP(hipGetLastError());
    return 0;
}

}  // namespace pgh
