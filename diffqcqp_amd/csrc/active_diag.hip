// active_diag.hip -- dqq_newton_active_f64 with DQQ_P_DIAG: P the compact diagonal (B,N).  newton_diag.hip's tile: a wave64
// owns 128/N consecutive problems, lane = (problem, coordinate pair / contact); every (B,N) vector is one 16-byte access per
// lane at an even element offset (state (B,N): one 8-byte store of two ints), so a batch slice is a valid argument.
//
// Everything stays in registers: a lane forms its two z with active_core.h's element functions, the state, multiplier and
// margin of its two coordinates (or of its contact), and the problem's (margin, where) is a butterfly over the problem's lanes
// on (value, index) pairs -- active_min is the scan's "first smallest in index order" whatever the shape of the reduction.
// There is no loop and no LDS; what the lanes of a problem share besides the minimum is whether an input or a z was not
// finite (one ballot).
#include "active_tile.h"
#include "diag_tile.h"

namespace dqq {

template <int KIND, int N, int WPB>
__global__ __launch_bounds__(64 * WPB) void active_diag_kernel(const ActiveArgs a)
{
#pragma clang fp contract(off)
    constexpr int HL = N / 2;          // lanes per problem
    constexpr int T = 64 / HL;         // problems per wave tile (T*N == 128)
    static_assert(N >= 2 && (N & (N - 1)) == 0 && N <= 64, "N must be a power of two up to 64");

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long first = ((long)blockIdx.x * WPB + wave) * T;
    if (first >= a.B) return;
    const int nvalid = (a.B - first) < T ? (int)(a.B - first) : T;
    const int pl = lane / HL, j = lane % HL;
    const bool valid = pl < nvalid;
    const unsigned long long mine = diag_lane_mask<HL>(pl);

    const long co = first * N + 2 * lane;   // (B,N): a coordinate pair
    const long cc = first * HL + lane;      // (B,N/2): a contact
    const double2 zero2 = make_double2(0.0, 0.0);
    auto load2 = [&](const double* p) { return valid ? *reinterpret_cast<const double2*>(p + co) : zero2; };

    const double2 pv = load2(a.P), qv = load2(a.q), xv = load2(a.x);
    bool bad = !fin2(pv) || !fin2(qv) || !fin2(xv);
    double ln = 1.0, mc = 1.0;
    double2 av = zero2, bv = zero2, cv = zero2;
    if constexpr (KIND == 1) {
        if (valid) { ln = a.a[cc]; mc = a.b[cc]; }
        bad = bad || !__builtin_isfinite(ln) || !__builtin_isfinite(mc);
    }
    if constexpr (KIND >= 2) {
        av = load2(a.a);
        bv = load2(a.b);
        const bool io = a.inf_bounds != 0;   // kernel-uniform: one-sided boxes admitted (polish_core.h)
        bad = bad || polish_lo_bad(av.x, io) || polish_lo_bad(av.y, io) || polish_hi_bad(bv.x, io) || polish_hi_bad(bv.y, io);
    }
    if constexpr (KIND == 3) {
        cv = load2(a.c);
        bad = bad || !fin2(cv);
    }
    const double z0 = polish_z(xv.x, polish_acc(0.0, pv.x, xv.x), qv.x);
    const double z1 = polish_z(xv.y, polish_acc(0.0, pv.y, xv.y), qv.y);
    bad = bad || !__builtin_isfinite(z0) || !__builtin_isfinite(z1);
    bad = (__ballot(bad) & mine) != 0ull;

    int st0 = 0, st1 = 0;
    double m0 = 0.0, m1 = 0.0, e0, e1;
    ActiveMin best;
    if constexpr (KIND == 1) {
        active_contact(z0, z1, ln * mc, st0, m0, e0);
        best = ActiveMin{e0, j};
    } else {
        active_box<KIND>(z0, av.x, bv.x, cv.x, st0, m0, e0);
        active_box<KIND>(z1, av.y, bv.y, cv.y, st1, m1, e1);
        best = active_min(ActiveMin{e0, 2 * j}, ActiveMin{e1, 2 * j + 1});
    }
    best = active_min_over<HL>(best);
    if (!valid) return;
    const double nan = newton_nan();
    if constexpr (KIND == 1) {
        if (a.state != nullptr) a.state[cc] = bad ? -1 : st0;
        if (a.mult != nullptr) a.mult[cc] = bad ? nan : m0;
    } else {
        if (a.state != nullptr) *reinterpret_cast<int2*>(a.state + co) = bad ? make_int2(-1, -1) : make_int2(st0, st1);
        if (a.mult != nullptr) *reinterpret_cast<double2*>(a.mult + co) = bad ? make_double2(nan, nan) : make_double2(m0, m1);
    }
    if (j == 0) {
        if (a.margin != nullptr) a.margin[first + pl] = bad ? nan : best.v;
        if (a.where != nullptr) a.where[first + pl] = bad ? -1 : best.i;
        if (a.status != nullptr) a.status[first + pl] = bad ? 2 : 0;
    }
}

hipError_t launch_active_diag(int kind, const ActiveArgs& a, hipStream_t s)
{
    return launch_diag(kind, a.N, a.B, s,
                       [](auto k, auto n) { return active_diag_kernel<decltype(k)::value, decltype(n)::value, kDiagWPB>; }, a);
}

} // namespace dqq
