// tuning.h -- the kernels' tuning constants.
//
// Shipped build: every knob below is a COMPILE-TIME constant (the value its sweep settled on; the measurements sit next to
// the code that reads it) and dqq_set_option() knows none of them: a call's route is a function of its arguments.
// Developer build (-DDQQ_TUNING: `DQQ_EXTRA_FLAGS=-DDQQ_TUNING python -m diffqcqp_amd.build`): the same names are
// process-wide atomics behind dqq_set_option / dqq_get_option, for A/B sweeps (tools/) and for the tests that drive the
// alternative kernels (tests/: `needs_tuning`).  Nothing here changes a result: the knobs that DO change numerics --
// reference-order kernels instead of the matrix-core ones for 16 < N <= 64 -- are a per-call flag of the C ABI
// (DQQ_F_REFERENCE_ORDER, include/diffqcqp_hip.h), not process state.
#pragma once

#include <atomic>

namespace dqq {

// name, shipped value                 what it selects (0 / -1 = the built-in choice where noted).  The ONE list of the knobs:
// knob_<name>() below, and in capi.hip the atomics and the option names of the developer build, are generated from it.
#define DQQ_KNOBS(X)                                                                                                          \
    X(fwd_lpp, 0)             /* lanes per problem of the diagonal forward (0 = from (N, B): route.cpp default_lpp) */       \
    X(wpb, 0)                 /* waves per workgroup of the diagonal kernels (0 = 4) */                                      \
    X(fuse_fallback, -1)      /* non-diagonal tiles inside the fast kernel (1), queued (0), by (N, B) (-1) */                \
    X(fwd_respread, 16)       /* N = 8 forward on two lanes: tail of <= this many problems moves to four lanes */            \
    X(fwd_respread2, 8)       /* ... and of <= this many to eight lanes */                                                   \
    X(fwd_respread2_from, 48) /* ... but not before this iteration (below) */                                                \
    X(lane_dense, 1)          /* general forward N <= 8: lane-per-problem kernel */                                          \
    X(lane_defer, 0)          /* general forward N <= 16: refactorisation every k trips (0 = 4 QCQP / 6 others) */           \
    X(dense_teams, 1)         /* general backward: 64/T problems per wave for small N */                                     \
    X(small_fwd, 1)           /* general forward N = 10..16: team-per-problem kernel */                                      \
    X(small_bwd, 1)           /* general backward even N <= 16: statically sized team kernel */                              \
    X(lane_bwd, 1)            /* general backward N <= 8, B >= 16384: lane-per-problem kernel */                             \
    X(fwd_feedback, 1)        /* 0: the forward ignores DQQ_F_EXPECT_DENSE */                                                \
    X(bwd_skip_classify, 1)   /* 0: the backward ignores DQQ_F_EXPECT_DENSE (always classifies first) */
// fwd_respread2_from: a tile whose problems are done by then (the well-conditioned bench shape: tile maxima 24-38) skips the
// second move, which costs it more than its last few iterations on four lanes (QP forward 26.0 -> 25.4 us, round 6)

#if defined(DQQ_TUNING)
constexpr bool kTuning = true;
#define DQQ_KNOB(name, dflt)              \
    extern std::atomic<int> g_##name;     \
    inline int knob_##name() { return g_##name.load(std::memory_order_relaxed); }
#else
constexpr bool kTuning = false;
#define DQQ_KNOB(name, dflt) \
    constexpr int knob_##name() { return (dflt); }
#endif
DQQ_KNOBS(DQQ_KNOB)
#undef DQQ_KNOB

// Route counters (diagnostics, both builds): how often the feedback hint changed a route.  Read with dqq_get_option, reset by
// dqq_set_option(name, 0) -- the only names the shipped dqq_set_option accepts.
extern std::atomic<int> g_lane_list_drains;    // drain launches sent to the lane-per-problem backward
extern std::atomic<int> g_bwd_whole_batches;   // DQQ_P_AUTO backwards solved whole by the lane-per-problem kernel
extern std::atomic<int> g_fwd_feedback_routes; // N = 8 forwards moved to one lane per problem

} // namespace dqq
