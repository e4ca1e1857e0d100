// active_dense.hip -- dqq_newton_active_f64 on a general P (B,N,N): active_core.h by a team of T threads per problem, one
// template with an LDS / global switch.
//   ActiveTeam (LDS = true, N <= 64): newton_dense.hip's teams and launch geometry -- T = 8 .. 64 lanes, 64/T problems per wave,
//     a persistent grid.  The team stages P and x in its LDS slice with coalesced loads (consecutive lanes, consecutive
//     addresses) on PolishTeam's odd row stride; then lane i owns row i.
//   ActiveAny (LDS = false, N > 64): a 256-thread workgroup per problem on any_grid workgroups walks the rows in chunks of 256
//     (256 is even: a contact never straddles a chunk), a thread reading its row from global memory.  state and mult are
//     written per chunk, the minimum is carried per thread and combined at the end.  No scratch: the entry takes no workspace.
// A thread sums its row sequentially in index order with polish_acc -- no reduction tree inside a row, so the bits are the
// host core's, and a diagonal P given as (B,N,N) gives DQQ_P_DIAG's bits (adding the exact-zero products leaves the sum as it
// is).  The contact partner's z comes from the neighbouring lane (DPP), the per-problem minimum is active_tile.h's butterfly
// on (value, index) pairs (ActiveAny: per wave, then four pairs through LDS).
#include "active_tile.h"
#include "team_dense.h"

namespace dqq {

// A team's slice in doubles: the matrix, then x, padded so that the slices of a wave's teams start T rows apart modulo the 32
// eight-byte bank pairs -- lane i of team t then reads bank pair ((t T + i) ld + j) mod 32 with ld odd: the 32 lanes a
// ds_read_b64 serves at a time hit 32 different ones, as if the wave were one team.
static DQQ_HD int active_slice_doubles(int n, int T)
{
    const int need = n * (n | 1) + n, want = (T * (n | 1)) % 32;
    return need + ((want - need) % 32 + 32) % 32;
}

// the element of row i from its z (and, for a contact, the z of row i + 1): what this thread writes and its entry to the scan
template <int KIND>
static DQQ_D ActiveMin active_row(const ActiveArgs& a, long prob, int i, bool live, double z, double znext, int& st, double& m)
{
#pragma clang fp contract(off)
    const int n = a.N;
    ActiveMin mine{__builtin_inf(), 0x7fffffff};
    st = 0;
    m = 0.0;
    if constexpr (KIND == 1) {
        if (live && (i & 1) == 0) {
            const long k = prob * (long)(n / 2) + i / 2;
            double e;
            active_contact(z, znext, a.a[k] * a.b[k], st, m, e);
            mine = ActiveMin{e, i / 2};
        }
    } else {
        if (live) {
            const long k = prob * (long)n + i;
            double e;
            active_box<KIND>(z, KIND >= 2 ? a.a[k] : 0.0, KIND >= 2 ? a.b[k] : 0.0, KIND == 3 ? a.c[k] : 0.0, st, m, e);
            mine = ActiveMin{e, i};
        }
    }
    return mine;
}

// whether this thread's share of q, x and the extras of row i holds something that is not finite
template <int KIND>
static DQQ_D bool active_row_bad(const ActiveArgs& a, long prob, int i)
{
    const int n = a.N;
    const long v = prob * (long)n + i;
    bool bad = !__builtin_isfinite(a.q[v]) || !__builtin_isfinite(a.x[v]);
    if constexpr (KIND == 1) {
        if ((i & 1) == 0) {
            const long k = prob * (long)(n / 2) + i / 2;
            bad = bad || !__builtin_isfinite(a.a[k]) || !__builtin_isfinite(a.b[k]);
        }
    }
    if constexpr (KIND >= 2) bad = bad || polish_lo_bad(a.a[v], a.inf_bounds != 0) || polish_hi_bad(a.b[v], a.inf_bounds != 0);
    if constexpr (KIND == 3) bad = bad || !__builtin_isfinite(a.c[v]);
    return bad;
}

template <int KIND>
static DQQ_D void active_row_store(const ActiveArgs& a, long prob, int i, bool bad, int st, double m)
{
    const int n = a.N;
    if constexpr (KIND == 1) {
        if ((i & 1) != 0) return;
        const long k = prob * (long)(n / 2) + i / 2;
        if (a.state != nullptr) a.state[k] = bad ? -1 : st;
        if (a.mult != nullptr) a.mult[k] = bad ? newton_nan() : m;
    } else {
        const long k = prob * (long)n + i;
        if (a.state != nullptr) a.state[k] = bad ? -1 : st;
        if (a.mult != nullptr) a.mult[k] = bad ? newton_nan() : m;
    }
}

static DQQ_D void active_problem_store(const ActiveArgs& a, long prob, bool bad, ActiveMin best)
{
    if (a.margin != nullptr) a.margin[prob] = bad ? newton_nan() : best.v;
    if (a.where != nullptr) a.where[prob] = bad ? -1 : best.i;
    if (a.status != nullptr) a.status[prob] = bad ? 2 : 0;
}

// One problem by one team of T <= 64 lanes (T >= n).  M: n x (n|1) in LDS, xs: n.
template <int KIND, int T>
static DQQ_D void team_active_problem(const ActiveArgs& a, long prob, double* M, double* xs, int lane)
{
#pragma clang fp contract(off)
    const int n = a.N, ld = n | 1;
    const double* Pg = a.P + prob * (long)n * n;
    const bool live = lane < n;
    bool bad = false;
    for (int idx = lane; idx < n * n; idx += T) {
        const double v = Pg[idx];
        bad = bad || !__builtin_isfinite(v);
        M[(idx / n) * ld + idx % n] = v;
    }
    if (live) {
        xs[lane] = a.x[prob * (long)n + lane];
        bad = bad || active_row_bad<KIND>(a, prob, lane);
    }
    wave_lds_fence();
    double z = 0.0;
    if (live) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s = polish_acc(s, M[lane * ld + j], xs[j]);
        z = polish_z(xs[lane], s, a.q[prob * (long)n + lane]);
        bad = bad || !__builtin_isfinite(z);
    }
    bad = team_any<T>(bad);
    const double znext = partner<1>(z);   // (an even lane's neighbour: the contact's second row)
    int st;
    double m;
    const ActiveMin best = active_min_over<T>(active_row<KIND>(a, prob, lane, live, z, znext, st, m));
    if (live) active_row_store<KIND>(a, prob, lane, bad, st, m);
    if (lane == 0) active_problem_store(a, prob, bad, best);
    wave_lds_fence();   // the slice is the next problem's
}

// One problem by a workgroup of 256 threads, the rows in chunks of 256.  red: 4 pairs of LDS.
template <int KIND>
static DQQ_D void any_active_problem(const ActiveArgs& a, long prob, ActiveMin* red)
{
#pragma clang fp contract(off)
    const int n = a.N, tid = (int)threadIdx.x;
    const double* Pg = a.P + prob * (long)n * n;
    const double* xg = a.x + prob * (long)n;
    ActiveMin best{__builtin_inf(), 0x7fffffff};
    bool bad = false;
    for (int base = 0; base < n; base += kTeamAnyT) {   // (a uniform trip count: every lane takes part in the exchanges)
        const int i = base + tid;
        const bool live = i < n;
        double z = 0.0;
        if (live) {
            const double* row = Pg + (long)i * n;
            double s = 0.0;
            for (int j = 0; j < n; ++j) {
                const double p = row[j];
                bad = bad || !__builtin_isfinite(p);
                s = polish_acc(s, p, xg[j]);
            }
            z = polish_z(xg[i], s, a.q[prob * (long)n + i]);
            bad = bad || !__builtin_isfinite(z) || active_row_bad<KIND>(a, prob, i);
        }
        const double znext = partner<1>(z);
        int st;
        double m;
        best = active_min(best, active_row<KIND>(a, prob, i, live, z, znext, st, m));
        if (live) active_row_store<KIND>(a, prob, i, false, st, m);
    }
    bad = team_any<kTeamAnyT>(bad);   // (a workgroup barrier; also: red is free again)
    best = active_min_over<64>(best);
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (bad)   // rare: the rows this thread wrote above, again
        for (int i = tid; i < n; i += kTeamAnyT) active_row_store<KIND>(a, prob, i, true, 0, 0.0);
    if (tid == 0) active_problem_store(a, prob, bad, active_min(active_min(red[0], red[1]), active_min(red[2], red[3])));
}

template <int KIND, int T, bool LDS>
__global__ __launch_bounds__(256) void active_dense_kernel(const ActiveArgs a, int lds_per_team)
{
    if constexpr (LDS) {
        extern __shared__ __attribute__((aligned(16))) double smem[];
        constexpr int TP = 64 / T; // teams per wave
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
        const int team = lane / T, tl = lane % T;
        double* sw = smem + (wave * TP + team) * lds_per_team;
        const long nteams = (long)gridDim.x * wpb * TP;
        // (a team past the end of the batch idles: fences, ballots and DPP exchanges are wave-wide, a team only reads its own lanes)
        for (long w = ((long)blockIdx.x * wpb + wave) * TP + team; w < a.B; w += nteams)
            team_active_problem<KIND, T>(a, w, sw, sw + a.N * (a.N | 1), tl);
    } else {
        __shared__ ActiveMin red[kTeamAnyT / 64];
        for (long w = blockIdx.x; w < a.B; w += gridDim.x) any_active_problem<KIND>(a, w, red);
    }
}

hipError_t launch_active_dense(int kind, const ActiveArgs& a, bool any, hipStream_t s)
{
    // team_dense.h's launch on this kernel's slice; the any-N form keeps its rows in registers and four pairs in LDS: no scratch
    const long slice = any ? 0 : active_slice_doubles(a.N, team_width(a.N));
    return dispatch_kind(kind, [&](auto k) {
        return launch_team(a.N, a.B, any, slice, nullptr, false, s, [&](auto t, auto lds, auto go, int lds_per_team, long) {
            return go(active_dense_kernel<decltype(k)::value, decltype(t)::value, decltype(lds)::value>, a, lds_per_team);
        });
    });
}

} // namespace dqq
