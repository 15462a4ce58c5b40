// The run-ahead protocol of the multi-seed device loops, shared by the f32 loops (pgh_spmm.hip) and their f64 siblings
// (pgh_spmm64.hip): the per-column loop state the close kernels keep, the pinned ring its last four words are copied to after every
// step, and the host driver that keeps a few steps enqueued beyond the last one whose outcome it has seen.
#pragma once
#include "pgh_common.h"

#include <functional>

namespace pgh {
namespace {     // (no exported symbols)

constexpr int kLanes = 64;

struct BatchState {
    double scale[kLanes];        // quotient of the current iterate (1 / sum(y_k); 1 without the quotient)
    double err[kLanes];
    double sum[kLanes];
    double pred_inv[kLanes];     // PREDICTED quotient of the step being written (in-kernel residual, see k_mm_step)
    double pred_raw[kLanes];     // the uncorrected prediction it came from
    double sum_p[kLanes];        // sum of the column's personalization (measured by the first step)
    int    done[kLanes];
    int    steps[kLanes];
    int    converged[kLanes];
    // the four words the host polls after every step (copied to a pinned ring): every column has stopped / the in-kernel residual
    // of step `steps` could not vouch for its verdict on some column and the step waits for the separate kernel / executed steps
    // (paused == 2: the step is committed and the run waits to be narrowed, CloseParams::narrow_at)
    int    all_done;
    int    paused;
    int    executed;
    int    b;
};

// what the host polls after every step: the tail of BatchState, copied to a pinned ring by the stream (no queue drain per look)
struct BatchPoll {
    int all_done, paused, executed, b;
};
constexpr int kPollRing = 8;
struct PollRing {
    BatchPoll* host = nullptr;       // pinned [kPollRing]
    hipEvent_t ev[kPollRing] = {nullptr};
};
int poll_ring(PollRing** out) {
    static PollRing ring;
    if (ring.host == nullptr) {
        PGH_HIP(hipHostMalloc(reinterpret_cast<void**>(&ring.host), sizeof(BatchPoll) * kPollRing, hipHostMallocDefault));
        for (int i = 0; i < kPollRing; ++i) PGH_HIP(hipEventCreateWithFlags(&ring.ev[i], hipEventDisableTiming));
    }
    *out = &ring;
    return 0;
}

// The poll ring's protocol for one run: `ring` from poll_ring(), `state` the run's BatchState on the device.
struct MMRunAhead {
    PollRing*   ring = nullptr;
    BatchState* state = nullptr;

    // behind the close of step k: its outcome into slot k of the ring
    int publish_poll(int k) {
        PGH_HIP(hipMemcpyAsync(&ring->host[k % kPollRing], &state->all_done, sizeof(BatchPoll), hipMemcpyDeviceToHost, rt().stream));
        PGH_HIP(hipEventRecord(ring->ev[k % kPollRing], rt().stream));
        return 0;
    }
    // The host keeps up to three steps enqueued beyond the last one whose outcome it has seen; launches behind a stop or a pause are
    // no-ops.  enqueue_step(k) ends in publish_poll(k).  A step that reports a pause ran but for its close, and the steps enqueued behind
    // it did nothing: on_pause(k) closes it, its outcome comes through slot 0 and the run goes on behind it.  Slot 0 is also the slot
    // of every step that is a multiple of 8: the wait for the stream, before anything new is enqueued, is what makes that safe.
    // (on_pause empty: a loop whose kernels never pause.)
    // A step that reports the narrowing word (paused == 2, CloseParams::narrow_at) is committed and the steps enqueued behind it did
    // nothing either: on_narrow(k) moves the run into its narrower workspace, waits for the stream and clears the word, and the run goes
    // on behind step k.  The close that answers a pause may raise the word as well: a narrowing follows a committed close only.
    int run_ahead(int max_steps, const std::function<int(int)>& enqueue_step, const std::function<int(int)>& on_pause = nullptr,
                  const std::function<int(int)>& on_narrow = nullptr) {
        int enq = 0, seen = 0;
        bool stop = false;
        while (!stop) {
            while (enq < max_steps && enq - seen < 3) {
                PGH_TRY(enqueue_step(enq + 1));
                ++enq;
            }
            if (seen == enq) break;
            const int k = seen + 1;
            PGH_HIP(hipEventSynchronize(ring->ev[k % kPollRing]));
            const BatchPoll poll = ring->host[k % kPollRing];
            ++seen;
            if (poll.paused == 2 && on_narrow) {
                PGH_TRY(on_narrow(k));
                enq = seen;
            } else if (poll.paused && on_pause) {
                PGH_TRY(on_pause(k));
                PGH_HIP(hipMemcpyAsync(&ring->host[0], &state->all_done, sizeof(BatchPoll), hipMemcpyDeviceToHost, rt().stream));
                PGH_HIP(hipStreamSynchronize(rt().stream));
                enq = seen;
                stop = ring->host[0].all_done != 0;
                if (!stop && ring->host[0].paused == 2 && on_narrow) PGH_TRY(on_narrow(k));
            } else if (poll.all_done) {
                stop = true;
            }
        }
        return 0;
    }
};

}  // namespace
}  // namespace pgh
