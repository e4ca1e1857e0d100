// worklist.h -- the fallback work-list in the caller's workspace: its memory layout (plain C++) and the device-side protocol
// of the kernels that fill it (hygiene, push) and drain it (release, strided readers, WorkClaim).  DESIGN.md section 2.
#pragma once

#include "common.h"

namespace dqq {

// Fallback work-list in the caller's workspace (ints).  [0] number of queued
// problem indices, [1] exit ticket of the dense kernel (its last participant
// re-zeroes the header), [2] next unclaimed entry (dynamic pick-up), then 32 sub-tickets one cache line apart,
// entries from [kWsEntries].
constexpr int kWsCount = 0;
constexpr int kWsTicket = 1;
constexpr int kWsNext = 2; // work-list mode with dynamic pick-up: next unclaimed entry
constexpr int kWsRepTop = 8;    // [8..9] bwd_lane_dense.hip, REPORT mode: 64-bit (groups arrived, problems counted); zero between launches
constexpr int kWsFbShadow = 4;  // [4..7]: what this workspace's drain launches last wrote to the feedback buffer, and where (below)
constexpr int kWsFbSkips = 10;    // unchanged reports not sent since the last one that was (worklist_feedback)
constexpr int kWsPerProblem = 11; // bwd_diag.hip: 1 = this list holds single problems of classified mixed tiles (not whole tiles); cleared by the drain
constexpr int kWsDirty = 12;      // sticky: 1 = a kernel found this header inconsistent (see "work-list hygiene" below); dqq_workspace_status reads it, dqq_workspace_reset clears it
constexpr int kWsSubTickets = 32;   // first of 32 sub-tickets, kWsSubStride ints apart
constexpr int kWsSubStride = 32;    // 128 bytes: one sub-ticket per cache line
// N >= 32 (one to sixteen problems per workgroup of the fast kernel: a dense batch through DQQ_P_AUTO queues from
// thousands of workgroups within microseconds): the list is SEGMENTED -- workgroup i appends to segment i mod 32, each
// with its own counter on its own cache line and kWsSegCap(B) slots in the entry area; ws[kWsCount] is a flag there
// (1 = something is queued: an empty list is recognised with one load).  The
// 8192 same-address atomics of a 65536 x 64 batch took 0.12 ms of its forward and 0.10 ms of its backward (round 3).
constexpr int kWsSegCounts = kWsSubTickets + 32 * kWsSubStride; // entries queued on segment g: [kWsSegCounts + g * kWsSubStride]
constexpr int kWsSegNext = kWsSegCounts + 32 * kWsSubStride;   // next unclaimed entry of segment g (dynamic pick-up)
constexpr int kWsEntries = kWsSegNext + 32 * kWsSubStride;
constexpr bool worklist_segmented(int N) { return N >= 32; }
// slots per segment: the workgroups of one residue class hold at most B/32 + 2 * (problems per workgroup <= 256) problems.
// The invariant behind it -- one tile per wave, a grid of exactly ceil(tiles / waves per workgroup) workgroups, at most
// 256 problems per workgroup -- is static_assert'ed where the fast kernels push (fwd_diag.hip, bwd_diag.hip); a
// persistent or grid-stride fast kernel would need another capacity.
DQQ_HD constexpr long kWsSegCap(long B) { return B / 32 + 512; }
// ints behind the header that hold entries: B for the plain list, 32 segments otherwise
DQQ_HD constexpr long kWsEntryInts(long B) { return 32 * kWsSegCap(B); }

// what the outside world depends on (tests/test_gpu_worklist_guard.py)
static_assert(kWsSubTickets == 32 && kWsSegCounts == 1056 && kWsSegNext == 2080 && kWsEntries == 3104 && kWsDirty == 12,
              "work-list header layout");


// ---- work-list hygiene (round 5).  The protocol rests on an invariant -- "zero-filled once, every call leaves the header
// zeroed" -- that a caller can break: a workspace that was never zeroed, memory scribbled over, a launch chain cut short by an
// error.  The kernels therefore do not TRUST the header:
//   * the fast kernel that fills the list re-zeroes every word only the drain kernel writes that is not zero (exit tickets,
//     pick-up counters: worklist_prepare_begin / _end -- they are idle while it runs, so this is not a race) -- whatever they
//     held is repaired;
//   * a push whose slot would fall outside the entry area is not performed: the caller poisons that tile's outputs with NaN
//     and the header is marked dirty (worklist_push_entries returns false);
//   * a drain kernel clamps the count it reads to the entry area and replaces an entry that is not a problem of this batch
//     by problem 0 (solved once more, to the same values): nothing is read or written out of bounds, no problem that does
//     not exist is "solved", and the header is marked dirty;
//   * stale entries that ARE problems of this batch (a list left behind by an aborted chain) are solved again by the general
//     kernel behind the fast path: the same problem, the right answer -- and the drain re-zeroes the header as always.
// "Dirty" is sticky and host-visible (dqq_workspace_status); dqq_workspace_reset clears everything.
#if defined(__HIPCC__)
// plain list: slots behind the header; segmented list: slots per segment
DQQ_HD constexpr long worklist_capacity(int N, long B) { return worklist_segmented(N) ? kWsSegCap(B) : kWsEntryInts(B); }
// the count in *word (a word of the header ws), clamped to [0, cap]; a negative one is also repaired on the spot (nobody
// would draw the exit tickets of an "empty" list)
static DQQ_D long worklist_checked_count(const int* ws, const int* word, long cap)
{
    const long c = *word;
    if (c < 0 || c > cap) {
        const_cast<int*>(ws)[kWsDirty] = 1;
        if (c < 0) *const_cast<int*>(word) = 0;
        return c < 0 ? 0 : cap;
    }
    return c;
}
static DQQ_D long worklist_checked_entry(const int* ws, long e, long B)
{
    if ((unsigned long)e >= (unsigned long)B) {
        const_cast<int*>(ws)[kWsDirty] = 1;
        return 0;
    }
    return e;
}
// ONE wave of the fast kernel (the first of workgroup 0) LOADS those words when it starts (worklist_prepare_begin: the loads
// are in flight while the wave does its own tile) and looks at them when it is done (worklist_prepare_end): only a word that
// is not zero is written.  On the path every call takes this costs a handful of instructions and no wait; unconditional
// stores to the ~100 cache lines these words sit on delayed that wave -- and with it the end of an 8 us backward -- by
// 0.2 us (A/B of the builds, tools/ab_libs.py).  The drain is launched behind the fast kernel: the end of it is early enough.
struct WorklistIdle {
    int sub, sub_hi, segnext, head;   // lane < 32: its sub-ticket (two words) and segment pick-up; lane 0: ticket | next | report words
};
static DQQ_D WorklistIdle worklist_prepare_begin(const int* __restrict__ ws, int lane)
{
    WorklistIdle w{0, 0, 0, 0};
    if (lane < 32) {
        w.sub = ws[kWsSubTickets + lane * kWsSubStride];
        w.sub_hi = ws[kWsSubTickets + lane * kWsSubStride + 1];   // (the high word of the 64-bit report counters, bwd_lane_dense.hip)
        w.segnext = ws[kWsSegNext + lane * kWsSubStride];
    }
    if (lane == 0) w.head = ws[kWsTicket] | ws[kWsNext] | ws[kWsRepTop] | ws[kWsRepTop + 1];
    return w;
}
static DQQ_D void worklist_prepare_end(int* __restrict__ ws, int lane, const WorklistIdle& w)
{
    if ((w.sub | w.sub_hi | w.segnext | w.head) == 0) return;
    if (lane < 32) {
        ws[kWsSubTickets + lane * kWsSubStride] = 0;
        ws[kWsSubTickets + lane * kWsSubStride + 1] = 0;
        ws[kWsSegNext + lane * kWsSubStride] = 0;
    }
    if (lane == 0) {
        ws[kWsTicket] = 0;
        ws[kWsNext] = 0;
        ws[kWsRepTop] = 0;
        ws[kWsRepTop + 1] = 0;
    }
}

// Work-list mode of the general kernels: the last participant (wave or workgroup) out re-zeroes the
// work-list header for the next call.  Call from ONE lane per participant; `participants` = how many call
// (gridDim.x, or gridDim.x * waves per workgroup).
// With an empty list nothing is touched: hundreds of same-address atomics would otherwise serialise into
// ~13 us of an otherwise empty launch.  With entries, the tickets are drawn in two levels -- participant i on
// sub-ticket i mod 32, the last of each on the top ticket -- so that no address sees more than
// participants / 32 atomics: 4096 tickets on ONE address took ~30 us of the 67 us backward of a dense 65536 x 8
// batch through DQQ_P_AUTO (round 3).
static DQQ_D void worklist_release(int* ws, long count, int participants)
{
    if (count > 0) {
        const int id = (participants == (int)gridDim.x) ? (int)blockIdx.x
                                                        : (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
        const int g = id & 31;
        const int members = (participants - g + 31) >> 5;      // ids congruent to g below `participants`
        int* sub = ws + kWsSubTickets + g * kWsSubStride;
        if (atomicAdd(sub, 1) == members - 1) {
            *sub = 0;
            const int groups = participants < 32 ? participants : 32;
            if (atomicAdd(&ws[kWsTicket], 1) == groups - 1) {
                ws[kWsCount] = 0;
                ws[kWsTicket] = 0;
                ws[kWsNext] = 0;
                ws[kWsPerProblem] = 0;
                for (int h = 0; h < 32; ++h) {  // (segmented list, N >= 32)
                    ws[kWsSegCounts + h * kWsSubStride] = 0;
                    ws[kWsSegNext + h * kWsSubStride] = 0;
                }
            }
        }
    }
}

// Queue the n problems [first, first + n) of the calling wave (n = 0: none) for the general kernel.
// AGG: ONE global atomic per workgroup instead of one per wave -- with N >= 32 a wave tile is 2 to 16 problems, and
// a dense batch through DQQ_P_AUTO otherwise serialises tens of thousands of same-address atomics (0.38 ms at
// B=65536, N=64).  Every wave of the workgroup that has not returned yet must make the call (three workgroup
// barriers; waves that already ended are not waited for).  s_cnt: two ints of LDS.
// SEG: the segmented list (see kWsSegCounts): the counter and the slots of segment blockIdx.x mod 32.
template <bool AGG, bool SEG = false>
static DQQ_D bool worklist_push_entries(int* __restrict__ ws, long B, int n, bool writes, int rank, int entry, int lane,
                                        int* s_cnt)
{
    // n (wave-uniform) entries from this wave; the lanes with `writes` hold them: `entry` goes to slot base + rank.
    // Returns false (wave-uniform) when the slots would fall outside the entry area -- a header that did not start at
    // zero --: nothing is written then, the header is marked dirty and the caller poisons these problems' outputs.
    int* counter = SEG ? ws + kWsSegCounts + (int)(blockIdx.x & 31u) * kWsSubStride : ws + kWsCount;
    int* slots = SEG ? ws + kWsEntries + (long)(blockIdx.x & 31u) * kWsSegCap(B) : ws + kWsEntries;
    const long cap = SEG ? kWsSegCap(B) : kWsEntryInts(B);
    bool ok = true;
    if constexpr (!AGG) {
        if (n > 0) {
            int base = 0;
            if (lane == 0) {
                base = atomicAdd(counter, n);
                if (SEG) ws[kWsCount] = 1;
            }
            base = __shfl(base, 0, 64);
            ok = base >= 0 && (long)base + n <= cap;
            if (ok) { if (writes) slots[base + rank] = entry; }
            else if (lane == 0) ws[kWsDirty] = 1;
        }
    } else {
        if (threadIdx.x == 0) s_cnt[0] = 0;
        __syncthreads();
        int local = 0;
        if (lane == 0 && n > 0) local = atomicAdd(&s_cnt[0], n);
        __syncthreads();
        if (threadIdx.x == 0 && s_cnt[0] > 0) {
            s_cnt[1] = atomicAdd(counter, s_cnt[0]);
            if (SEG) ws[kWsCount] = 1;
        }
        __syncthreads();
        if (n > 0) {
            const int base = s_cnt[1] + __shfl(local, 0, 64);
            ok = s_cnt[1] >= 0 && (long)base + n <= cap;
            if (ok) { if (writes) slots[base + rank] = entry; }
            else if (lane == 0) ws[kWsDirty] = 1;
        }
    }
    return ok;
}
template <bool AGG, bool SEG = false>
static DQQ_D bool worklist_push(int* __restrict__ ws, long B, long first, int n, int lane, int* s_cnt)
{
    return worklist_push_entries<AGG, SEG>(ws, B, n, lane < n, lane, (int)(first + lane), lane, s_cnt);
}

// Readers of the work-list for the kernels that drain it with a fixed stride (the kernels behind tuning options and
// the global-memory kernels).  Plain list: the count word and entry w.  Segmented list (N >= 32): the 32 segment
// counters are summed / scanned on every call (~6 us: these kernels spend 50 us to milliseconds per problem).  The
// counters do not change while a drain kernel runs (the last participant out re-zeroes them, worklist_release).
static DQQ_D long worklist_count(const int* __restrict__ ws, int N, long B)
{
    if (ws[kWsCount] == 0) return 0;   // (an empty list, either kind: one load)
    if (!worklist_segmented(N)) return worklist_checked_count(ws, ws + kWsCount, kWsEntryInts(B));
    long c = 0;
#pragma unroll
    for (int h = 0; h < 32; ++h) c += worklist_checked_count(ws, ws + kWsSegCounts + h * kWsSubStride, kWsSegCap(B));
    return c;
}
// 0 <= w < worklist_count
static DQQ_D long worklist_entry(const int* __restrict__ ws, int N, long B, long w)
{
    if (!worklist_segmented(N)) return worklist_checked_entry(ws, ws[kWsEntries + w], B);
    long base = 0, at = 0;     // entries before segment g; slot of entry w
    int g = 0;
#pragma unroll
    for (int h = 0; h < 32; ++h) {
        const long c = worklist_checked_count(ws, ws + kWsSegCounts + h * kWsSubStride, kWsSegCap(B));
        if (w >= base && w < base + c) { g = h; at = w - base; }
        base += c;
    }
    return worklist_checked_entry(ws, ws[kWsEntries + g * kWsSegCap(B) + at], B);
}

// Dynamic pick-up for the wave-per-problem kernels (one wave per workgroup; iteration counts differ by 2x between
// problems, a fixed stride would leave the grid waiting for its unluckiest wave).  Every value is wave-uniform.
// Plain list: tickets on ws[kWsNext].  Segmented list: a wave starts on segment blockIdx.x mod 32, draws tickets on
// THAT segment's pick-up word and moves on when it is exhausted; after 32 exhausted segments it is done -- no
// prefix sums, and the tickets are spread over 32 addresses as the pushes were.
// The segmented pick-up can be pipelined (the backward kernels do; without the three ahead_* calls next() claims on
// the spot): while a wave works on a problem its ticket for the next one is in flight
// (ahead_issue right after next(), ahead_entry once the problem's own loads have landed, ahead_done at its end).  A
// ticket and the entry behind it are two dependent round trips to memory, ~3 us that the wave otherwise spends idle
// before every problem -- 7 % of a 42 us backward at N = 64.
struct WorkClaim {
    long count;        // direct mode: B; plain list: entries; segmented list: non-zero iff anything is queued
    int seg, left, c;  // segmented: current segment, segments not yet found exhausted, entries of the current one
    bool listed, segd;
    bool primed;       // segmented: `ahead` holds the wave's next problem (-1: none left)
    bool pipelined;    // ahead_done ran after the last next()
    long ahead;
    int flight;        // per lane: the ticket (stage 1) / the entry (stage 2) in flight
    int stage;         // 0 nothing in flight, 1 ticket, 2 entry
    DQQ_D void open(const int* __restrict__ ws, int use_worklist, int N, long B)
    {
        listed = use_worklist != 0;
        segd = listed && worklist_segmented(N);
        count = listed ? (segd ? (long)(ws[kWsCount] != 0) : worklist_checked_count(ws, ws + kWsCount, kWsEntryInts(B))) : B;
        seg = (int)(blockIdx.x & 31u);
        left = 32;
        c = -1;
        primed = false;
        pipelined = false;
        ahead = -1;
        flight = 0;
        stage = 0;
    }
    DQQ_D long claim_segmented(int* __restrict__ ws, long B)
    {
        while (left > 0) {
            if (c < 0) c = __builtin_amdgcn_readfirstlane((int)worklist_checked_count(ws, ws + kWsSegCounts + seg * kWsSubStride, kWsSegCap(B)));
            if (c > 0) {
                const int t = __builtin_amdgcn_readfirstlane(
                    threadIdx.x == 0 ? atomicAdd(&ws[kWsSegNext + seg * kWsSubStride], 1) : 0);
                if (t >= 0 && t < c)
                    return worklist_checked_entry(ws, (long)__builtin_amdgcn_readfirstlane(ws[kWsEntries + seg * kWsSegCap(B) + t]), B);
            }
            seg = (seg + 1) & 31;
            --left;
            c = -1;
        }
        return -1;
    }
    // the next problem of this wave, -1 = none left.  w: the caller's strided counter (direct mode only).
    // (An empty list is left untouched: nobody would reset its words.)
    DQQ_D long next(int* __restrict__ ws, long B, long w)
    {
        if (!listed) return w < count ? w : -1;
        if (count == 0) return -1;
        if (!segd) {
            const long t = __builtin_amdgcn_readfirstlane(threadIdx.x == 0 ? atomicAdd(&ws[kWsNext], 1) : 0);
            return (t >= 0 && t < count) ? worklist_checked_entry(ws, (long)__builtin_amdgcn_readfirstlane(ws[kWsEntries + t]), B) : -1;
        }
        if (!primed || !pipelined) { // the first problem, or a kernel that does not claim ahead
            ahead = claim_segmented(ws, B);
            primed = true;
        }
        return ahead;
    }
    // the three stages of the claim ahead; no-ops outside the segmented mode.  Call each once per problem, in order.
    DQQ_D void ahead_issue(int* __restrict__ ws)
    {
        stage = 0;
        if (segd && left > 0 && c > 0) {
            flight = threadIdx.x == 0 ? atomicAdd(&ws[kWsSegNext + seg * kWsSubStride], 1) : 0;
            stage = 1;
        }
    }
    DQQ_D void ahead_entry(const int* __restrict__ ws, long B)
    {
        if (stage == 1) {
            const int t = __builtin_amdgcn_readfirstlane(flight);
            if (t >= 0 && t < c) {
                flight = ws[kWsEntries + seg * kWsSegCap(B) + t];
                stage = 2;
            } else { // this segment is exhausted: ahead_done walks on
                seg = (seg + 1) & 31;
                --left;
                c = -1;
                stage = 0;
            }
        }
    }
    DQQ_D void ahead_done(int* __restrict__ ws, long B)
    {
        if (!segd) return;
        ahead = (stage == 2) ? worklist_checked_entry(ws, (long)__builtin_amdgcn_readfirstlane(flight), B) : claim_segmented(ws, B);
        stage = 0;
        pipelined = true;
    }
};
#endif

} // namespace dqq
