// report.h -- the report word a drain launch leaves for the caller and the arithmetic that reads it (plain C++; route.cpp
// turns it into hint flags), and the device code that writes it.
#pragma once

#include "worklist.h"

namespace dqq {

// ---- the report word and the route hints (round 4; stateless since round 5).  Which kernel drains a work-list best depends
// on how long the list is: the team kernel (bwd_small.hip) for a few thousand problems, the lane-per-problem kernel
// (bwd_lane_dense.hip) when the list fills the chip -- and the host, which picks the kernel, never sees the length (it sits in
// device memory and nothing on this path may wait for the device).  So the CALLER may hand a backward call one 8-byte word
// of host memory the device can write (`report`): the drain launch stores (B, entries it found) there -- when that differs from
// what the same workspace stored there last --, and the caller turns the word into hint flags for its NEXT calls of that kind,
// N and B with dqq_hint_flags(), a pure function: DQQ_F_EXPECT_LONG_LIST (drain with the lane kernel), DQQ_F_EXPECT_DENSE
// (backward: the lane kernel takes the whole batch, no classifying launch; forward of N = 8: one lane per problem).
// A hint, never a dependency: the routes give the same bits on ANY input (tests/test_gpu_parity.py), so a stale, racy or
// wrong hint costs time only.  The library keeps no state: where the word lives, for how long, per which device or stream,
// and whether to hint at all (not under stream capture: a graph is replayed on batches the word knows nothing about) is the
// caller's business -- diffqcqp_amd/_capi.py keeps one word per (device, kind, N).
// The word: bits 0..30 entries found, bit 31 "the entries are single problems" (with the forward's hand-off the fast path
// queues only the non-diagonal problems of a classified tile; otherwise whole tiles of 128 / N), 32..61 B (mod 2^30),
// 62..63 how many times IN A ROW before this one the same workspace reported "three quarters of the batch or more"
// (saturating at 3).
constexpr unsigned long long kFbBMask = 0x3fffffffULL, kFbCountMask = 0x7fffffffULL, kFbPerProblem = 0x80000000ULL;
inline bool hint_applies(int kind, int N) { return (kind == 0 || kind == 1) && N >= 2 && N <= 8 && N % 2 == 0; }
// entries the drain launch that wrote `w` found, if it ran on a batch of B problems; -1: not known.
// *streak (optional): consecutive earlier reports of count >= 3/4 B.
inline long report_count(unsigned long long w, long B, int* streak = nullptr, bool* per_problem = nullptr)
{
    if (streak != nullptr) *streak = 0;
    if (per_problem != nullptr) *per_problem = false;
    if (w == 0 || ((w >> 32) & kFbBMask) != ((unsigned long long)B & kFbBMask)) return -1;
    if (streak != nullptr) *streak = (int)(w >> 62);
    if (per_problem != nullptr) *per_problem = (w & kFbPerProblem) != 0;
    return (long)(w & kFbCountMask);
}
// problems that sit in a 16-problem block with a non-diagonal one (what the fused forward of N = 8 pays for: one pass of its
// general solve per such block), from the word: the count itself when whole tiles were queued, an estimate for scattered
// problems when single problems were
inline long report_count_in_blocks(unsigned long long w, long B)
{
    bool per_problem = false;
    const long c = report_count(w, B, nullptr, &per_problem);
    if (c <= 0 || !per_problem) return c;
    double stay = 1.0 - (double)c / (double)B, p = stay;
    for (int k = 0; k < 4; ++k) p *= p;   // (1 - c/B)^16
    return (long)((double)B * (1.0 - p));
}
#if defined(__HIPCC__)
// Call from ONE lane of the launch.  The store goes to host memory, and a launch that has one in flight ends later
// (headline step +0.5 us, A/B): the workspace header remembers the last word this workspace sent and where, and an unchanged
// word -- every step of a training loop on one kind of batch -- is not sent again.  The streak (above) is what lets the host
// skip the fast path's launch only for a caller whose batches have been all non-diagonal at least twice running: a caller
// that alternates between kinds of batches under one (kind, N, B) never gets there.
static DQQ_D void worklist_feedback(unsigned long long* fb, int* ws, long B, long count)
{
    const bool per_problem = ws[kWsPerProblem] != 0;   // (set by the fast path that filled this list; this launch drains it)
    if (per_problem) ws[kWsPerProblem] = 0;
    if (fb == nullptr) return;
    unsigned long long* shadow = reinterpret_cast<unsigned long long*>(ws + kWsFbShadow);   // (ws: 16-byte aligned)
    const unsigned long long prev = shadow[0], bb = (unsigned long long)B & kFbBMask;
    const bool same_place = shadow[1] == reinterpret_cast<unsigned long long>(fb);
    unsigned long long streak = 0;
    if (same_place && ((prev >> 32) & kFbBMask) == bb && 4 * (long)(prev & kFbCountMask) >= 3 * B && 4 * count >= 3 * B)
        streak = (prev >> 62) < 3 ? (prev >> 62) + 1 : 3;
    const unsigned long long v = (streak << 62) | (bb << 32) | (per_problem ? kFbPerProblem : 0ULL) | (unsigned long long)count;
    // (the shadow is per WORKSPACE, the word may be shared by several -- diffqcqp_amd/_capi.py keeps one per (device, kind,
    // N) --: another workspace's launch may have overwritten a word this one believes unchanged.  Every 64th unchanged
    // report is therefore sent anyway, so that a word can be stale for a bounded number of calls only: ADVICE r5)
    if (prev == v && same_place && ws[kWsFbSkips] < 63) { ws[kWsFbSkips] += 1; return; }
    ws[kWsFbSkips] = 0;
    shadow[0] = v;
    shadow[1] = reinterpret_cast<unsigned long long>(fb);
    __hip_atomic_store(fb, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
#endif

} // namespace dqq
