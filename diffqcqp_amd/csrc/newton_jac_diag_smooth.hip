// newton_jac_diag_smooth.hip -- dqq_newton_jac_smooth_f64 (kappa > 0) with DQQ_P_DIAG: smooth_core.h's newton_jac_problem_smooth
// on the compact diagonal (B,N), the Jacobians block-diagonal and compact.  newton_jac_diag.hip's tile, loads, stores and launch
// geometry: a wave64 owns 128/N consecutive problems, lane = (problem, coordinate pair / contact), no loop and no LDS, two ballots
// per problem (an input that is not finite, a failed pivot).  Smoothing keeps D diagonal in 1 x 1 or 2 x 2 blocks, so the compact
// layout is still exact: a lane solves its blocks for the unit tangents of its own inputs in registers with polish_solve1 /
// polish_solve2, on right-hand sides from smooth_core.h's smooth_jac_* element functions.  D and E are those of PI_k, so no
// column is a signed zero any more.  kappa and the proximal weight are read at run time from the second kernel argument
// (polish_reg).  kappa == 0 never gets here: capi.hip sends it to newton_jac_diag*.hip.
#include "diag_tile.h"
#include "smooth_core.h"

namespace dqq {

typedef double jac_smooth_v2d __attribute__((ext_vector_type(2)));   // one 16-byte non-temporal store

static DQQ_D void jsstore2(double* p, bool failed, double v0, double v1)
{
    const double nan = newton_nan();
    jac_smooth_v2d v;
    v.x = failed ? nan : v0;
    v.y = failed ? nan : v1;
    __builtin_nontemporal_store(v, reinterpret_cast<jac_smooth_v2d*>(p));
}

template <int KIND, int N, int WPB>
__global__ __launch_bounds__(64 * WPB) void newton_jac_diag_smooth_kernel(const NewtonJacArgs a, const NewtonJacSmoothOpts o)
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
    const double kappa = o.kappa;

    const long co = first * N + 2 * lane;   // (B,N): a coordinate pair
    const long cc = first * HL + lane;      // (B,N/2): a contact
    const double2 zero2 = make_double2(0.0, 0.0);
    auto load2 = [&](const double* p) { return valid ? *reinterpret_cast<const double2*>(p + co) : zero2; };

    const double2 pv = valid ? *reinterpret_cast<const double2*>(a.P + co) : make_double2(1.0, 1.0);
    const double2 qv = load2(a.q), xv = load2(a.x);
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
        bad = bad || !fin2(av) || !fin2(bv);   // one-sided boxes are not admitted under smoothing
    }
    if constexpr (KIND == 3) {
        cv = load2(a.c);
        bad = bad || !fin2(cv);
    }
    bad = (__ballot(bad) & mine) != 0ull;

    const double x0 = xv.x, x1 = xv.y;
    const double z0 = polish_z(x0, polish_acc(0.0, pv.x, x0), qv.x);
    const double z1 = polish_z(x1, polish_acc(0.0, pv.y, x1), qv.y);
    // the diagonal of P' for the blocks of M; z above read pv
    const double pm0 = polish_reg(pv.x, o.reg), pm1 = polish_reg(pv.y, o.reg);

    bool ok = true;
    double r[8];   // QCQP: (d0, d1) of q_2k, q_2k+1, l_n, mu; box-like: (coordinate 0, coordinate 1) of q, a, b
    if constexpr (KIND == 1) {
        const SmoothDisc sd = smooth_disc(z0, z1, ln * mc, kappa);
        double m[4];
        newton_contact_block(sd.D, pm0, pm1, m);
#pragma unroll
        for (int col = 0; col < 4; ++col) {
            const int which = col < 2 ? 0 : col - 1;
            const bool ha = col != 1, hb = col == 1;
            r[2 * col] = smooth_jac_contact_rhs(sd, 0, ln, mc, which, ha, hb);
            r[2 * col + 1] = smooth_jac_contact_rhs(sd, 1, ln, mc, which, ha, hb);
            ok = polish_solve2(m[0], m[1], m[2], m[3], r[2 * col], r[2 * col + 1]) && ok;
        }
    } else {
        const SmoothBox b0 = smooth_box_at<KIND>(z0, av.x, bv.x, cv.x, kappa), b1 = smooth_box_at<KIND>(z1, av.y, bv.y, cv.y, kappa);
        const double m0 = smooth_box_entry(true, b0.D, pm0), m1 = smooth_box_entry(true, b1.D, pm1);
#pragma unroll
        for (int which = 0; which < (KIND == 0 ? 1 : 3); ++which) {
            r[2 * which] = smooth_jac_box_rhs(b0, which, true);
            r[2 * which + 1] = smooth_jac_box_rhs(b1, which, true);
            ok = polish_solve1(m0, r[2 * which]) && ok;
            ok = polish_solve1(m1, r[2 * which + 1]) && ok;
        }
    }
    const bool failed = bad || (__ballot(valid && !ok) & mine) != 0ull;   // a failed block fails its problem
    if (!valid) return;
    if (j == 0 && a.status != nullptr) a.status[first + pl] = bad ? 2 : (failed ? 1 : 0);
    if constexpr (KIND == 1) {
        if (a.Jq != nullptr) {   // rows 2k and 2k+1 of (B,N,2): (d0 of q_2k, d0 of q_2k+1), (d1 of q_2k, d1 of q_2k+1)
            jsstore2(a.Jq + 2 * co, failed, r[0], r[2]);
            jsstore2(a.Jq + 2 * co + 2, failed, r[1], r[3]);
        }
        if (a.Ja != nullptr) jsstore2(a.Ja + co, failed, r[4], r[5]);
        if (a.Jb != nullptr) jsstore2(a.Jb + co, failed, r[6], r[7]);
    } else {
        if (a.Jq != nullptr) jsstore2(a.Jq + co, failed, r[0], r[1]);
        if constexpr (KIND >= 2) {
            if (a.Ja != nullptr) jsstore2(a.Ja + co, failed, r[2], r[3]);
            if (a.Jb != nullptr) jsstore2(a.Jb + co, failed, r[4], r[5]);
        }
    }
}

hipError_t launch_newton_jac_diag_smooth(int kind, const NewtonJacArgs& a, const NewtonJacSmoothOpts& o, hipStream_t s)
{
    return launch_diag(kind, a.N, a.B, s,
                       [](auto k, auto n) { return newton_jac_diag_smooth_kernel<decltype(k)::value, decltype(n)::value, kDiagWPB>; }, a, o);
}

} // namespace dqq
