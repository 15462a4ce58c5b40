// The retiring protocol of the multi-seed device loops (include/pgh_retire.h, include/pgh_retire64.h), shared by the f32 loops
// (pgh_spmm.hip) and their f64 siblings (pgh_spmm64.hip): the plan of a run (its levels and its report), the ledger of which caller
// column sits in which lane, the kernel that lets the loop state follow its columns, and the exchange of a workspace's blocks with the
// pool.  Everything here but the two kernels is host arithmetic: no function of this file waits for the stream or enqueues a copy.
// What differs between the families -- the way out of the leaving columns, the repack of the slabs, where a narrowing waits -- stays
// with the loops.
#pragma once
#include "pgh_mm_run.h"
#include "pgh_retire.h"

#include <initializer_list>
#include <vector>

namespace pgh {
namespace {     // (no exported symbols)

// what a retiring entry takes behind its plain sibling's arguments (null: the plain entry)
struct RetireArgs {
    const int32_t*     levels;
    int32_t            num_levels;
    pgh_retire_report* report;
};

// The host's record of a run that retires its columns: the levels, and the report as it grows.  quantum: the columns a slab is padded
// to (4 floats, 2 doubles: a lane's 16 bytes).
struct RetirePlan {
    std::vector<int>  levels;        // strictly descending
    pgh_retire_report report{};
    int               quantum = 4;
    // null levels (num_levels != 0): default_levels
    int init(const int32_t* given, int32_t num_levels, const char* who, int pad_quantum, std::initializer_list<int> default_levels) {
        quantum = pad_quantum;
        if (given == nullptr && num_levels != 0) {
            levels = default_levels;
            return 0;
        }
        PGH_CHECK(num_levels >= 0 && num_levels < kLanes, std::string(who) + ": the number of levels must be in [0, 63]");
        for (int i = 0; i < num_levels; ++i) {
            PGH_CHECK(given[i] >= 1 && given[i] < kLanes && (i == 0 || given[i] < given[i - 1]),
                      std::string(who) + ": the levels must be strictly descending live-column counts in [1, 63]");
            levels.push_back(given[i]);
        }
        return 0;
    }
    // the live count at or below which a slab of width ld narrows (0: never): the greatest level below ld, and a narrower slab results
    int trigger(int ld, int stages) const {
        if (stages >= PGH_RETIRE_MAX_STAGES) return 0;
        for (int level : levels)
            if (level < ld) return level < ld - quantum ? level : ld - quantum;
        return 0;
    }
    void stage(int ld, int live, int first_step) {
        const int s = report.num_stages;
        if (s > 0) report.column_steps += (int64_t)report.ld[s - 1] * (first_step - report.first_step[s - 1]);
        report.ld[s] = ld;
        report.live[s] = live;
        report.first_step[s] = first_step;
        report.num_stages = s + 1;
    }
    void close(int executed) {
        const int s = report.num_stages - 1;
        report.column_steps += (int64_t)report.ld[s] * (executed + 1 - report.first_step[s]);
    }
};
// the way out of a retiring entry (ra null: a plain one): the report once the run has ended well
int retire_report_out(int status, const RetirePlan& plan, const RetireArgs* ra) {
    if (status == 0 && ra != nullptr && ra->report != nullptr) *ra->report = plan.report;
    return status;
}
// the steps a run executed, from the records MMRun::finish / MM64Run::finish wrote: the column that ran longest took part in every one
int executed_steps(const pgh_loop_result* results, int b) {
    int executed = 0;
    for (int j = 0; j < b; ++j) executed = results[j].spmv_count > executed ? results[j].spmv_count : executed;
    return executed;
}

// the lanes of the loop state follow their columns: lane i <- lane src.v[i] for i < b_new, the lanes beyond are done from the start (as
// the state's init kernels leave them); the word that voided the enqueued steps is cleared
struct ColMap {
    int v[kLanes];
};
__global__ void k_mm_state_narrow(BatchState* state, ColMap src, int b_new) {
    const int lane = threadIdx.x;
    const int s = lane < b_new ? src.v[lane] : -1;
    const double scale = s >= 0 ? state->scale[s] : 1.0, err = s >= 0 ? state->err[s] : 0.0, sum = s >= 0 ? state->sum[s] : 0.0;
    const double pred_inv = s >= 0 ? state->pred_inv[s] : 1.0, pred_raw = s >= 0 ? state->pred_raw[s] : 0.0, sum_p = s >= 0 ? state->sum_p[s] : 0.0;
    const int done = s >= 0 ? state->done[s] : 1, steps = s >= 0 ? state->steps[s] : 0, converged = s >= 0 ? state->converged[s] : 0;
    __syncthreads();                                       // every lane has read before any lane writes
    state->scale[lane] = scale;
    state->err[lane] = err;
    state->sum[lane] = sum;
    state->pred_inv[lane] = pred_inv;
    state->pred_raw[lane] = pred_raw;
    state->sum_p[lane] = sum_p;
    state->done[lane] = done;
    state->steps[lane] = steps;
    state->converged[lane] = converged;
    if (lane == 0) {
        state->paused = 0;
        state->b = b_new;
    }
}

// a closed-form run's check of iteration 2 (convergence.py:96-101 on delta_1 = |result_1|, the single-vector loop's host-side check), per column
__global__ void k_mm_poly_first(BatchState* __restrict__ state, const double* __restrict__ err1, int check, int err_kind, double tol, long long n) {
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

// The column ledger of a run that retires its columns.  A column leaves once, at the narrowing that follows its stop or at the end, and
// its part of the loop state is kept for results[].
struct RetireLedger {
    const int  width;                // the caller's row length
    const int  quantum;              // RetirePlan::quantum
    int        col_of[kLanes];       // the caller's column in lane (column) i of the current slabs
    BatchState kept{};               // lanes indexed by the caller's column

    RetireLedger(int b, int pad_quantum) : width(b), quantum(pad_quantum) {
        for (int j = 0; j < kLanes; ++j) col_of[j] = j < b ? j : -1;
    }
    int padded(int b) const { return (b + quantum - 1) / quantum * quantum; }
    // The lanes of the b current ones that have stopped (all: every lane) leave: each(lane, the caller's column, the state's quotient)
    // forms the caller's factor of the way out.
    template <typename Each>
    void leave(const BatchState& hs, int b, bool all, Each&& each) {
        for (int j = 0; j < b; ++j) {
            if (!(all || hs.done[j])) continue;
            const int c = col_of[j];
            kept.steps[c] = hs.steps[j];
            kept.converged[c] = hs.converged[j];
            kept.err[c] = hs.err[j];
            each(j, c, hs.scale[j]);
        }
    }
    // the live lanes of the b current ones, in lane order (-1 beyond them), and their count; an error unless the state behind step k asks
    // for a slab narrower than ld
    int live_map(const BatchState& hs, int b, int ld, int k, const char* who, ColMap* map, int* live) const {
        int nb = 0;
        for (int j = 0; j < kLanes; ++j) map->v[j] = -1;
        for (int j = 0; j < b; ++j)
            if (!hs.done[j]) map->v[nb++] = j;
        PGH_CHECK(nb >= 1 && padded(nb) < ld && hs.executed == k, std::string(who) + ": the loop state does not ask for a narrowing");
        *live = nb;
        return 0;
    }
    void follow(const ColMap& map, int nb) {
        int cols_now[kLanes];
        memcpy(cols_now, col_of, sizeof(cols_now));
        for (int j = 0; j < kLanes; ++j) col_of[j] = j < nb ? cols_now[map.v[j]] : -1;
    }
    // results[] of a run that narrowed, from what the columns left behind
    void fill(pgh_loop_result* results, double ms) const {
        for (int j = 0; j < width; ++j) {
            memset(&results[j], 0, sizeof(pgh_loop_result));
            results[j].iterations = 1 + kept.steps[j];
            results[j].converged = kept.converged[j];
            results[j].spmv_count = kept.steps[j];
            results[j].last_error = kept.err[j];
            results[j].loop_ms = ms;
            results[j].flags = PGH_RETIRE_NARROWED;
        }
    }
};

// `count` buffers of a workspace are taken again from the pool at new sizes, one after the other in the order given: the block a buffer
// held is parked in wide[i] (the stream may still be reading it) and what wide[i] held goes back to the pool (the caller has waited
// behind its last reader).  wide null: a first allocation.  The order is part of the speed (MMRun's members, pgh_spmm.hip).
int pool_renew(PoolBuf* const* mine, const size_t* bytes, int count, PoolBuf* wide) {
    for (int i = 0; i < count; ++i) {
        if (wide != nullptr) {
            if (wide[i].p != nullptr) pool_free(wide[i].p);
            wide[i].p = mine[i]->p;
            mine[i]->p = nullptr;
        }
        PGH_TRY(mine[i]->alloc(bytes[i]));
    }
    return 0;
}

}  // namespace
}  // namespace pgh
