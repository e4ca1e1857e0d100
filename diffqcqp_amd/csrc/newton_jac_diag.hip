// newton_jac_diag.hip -- dqq_newton_jac_f64 with DQQ_P_DIAG: P the compact diagonal (B,N), the Jacobians block-diagonal and
// compact.  newton_diag.hip's tile: a wave64 owns 128/N consecutive problems, lane = (problem, coordinate pair / contact); every
// (B,N) array is one 16-byte access per lane at an even element offset, the QCQP's Jq (B,N,2) two of them, so a batch slice is a
// valid argument.
//
// A lane solves its 1 x 1 blocks (QP, box kinds) or its 2 x 2 block (QCQP) for the unit tangents of its own inputs -- q_2k and
// q_2k+1, then a and b -- in registers with polish_solve1 / polish_solve2 on right-hand sides from newton_core.h's newton_jac_*
// element functions: newton_jac_problem's block form, bit for bit.  No LDS, no loop; what the lanes of a problem share is whether
// an input was not finite and whether a pivot failed (two ballots).  Nothing reads the outputs again here: the stores are
// non-temporal.
#include "diag_tile.h"
#include "newton_core.h"

// The proximal weight (polish_core.h): REG is a template parameter of every kernel here.  This file compiles the REG = false
// instantiations, which never read `reg`; newton_jac_diag_reg.hip defines DQQ_REG_UNIT and includes this file for the REG = true ones,
// which add reg to the diagonal entries of P where the thread that owns the entry forms M.
#ifndef DQQ_REG_UNIT
#define DQQ_REG_UNIT 0
#endif

namespace dqq {

constexpr bool kRegUnit = DQQ_REG_UNIT != 0;

typedef double jac_v2d __attribute__((ext_vector_type(2)));   // one 16-byte non-temporal store

static DQQ_D void jstore2(double* p, bool failed, double v0, double v1)
{
    const double nan = newton_nan();
    jac_v2d v;
    v.x = failed ? nan : v0;
    v.y = failed ? nan : v1;
    __builtin_nontemporal_store(v, reinterpret_cast<jac_v2d*>(p));
}

template <int KIND, int N, int WPB, bool REG>
__global__ __launch_bounds__(64 * WPB) void newton_jac_diag_kernel(const NewtonJacArgs a, const double reg)
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
        const bool io = a.inf_bounds != 0;   // kernel-uniform: one-sided boxes admitted (polish_core.h)
        bad = bad || polish_lo_bad(av.x, io) || polish_lo_bad(av.y, io) || polish_hi_bad(bv.x, io) || polish_hi_bad(bv.y, io);
    }
    if constexpr (KIND == 3) {
        cv = load2(a.c);
        bad = bad || !fin2(cv);
    }
    bad = (__ballot(bad) & mine) != 0ull;

    const double x0 = xv.x, x1 = xv.y;
    const double z0 = polish_z(x0, polish_acc(0.0, pv.x, x0), qv.x);
    const double z1 = polish_z(x1, polish_acc(0.0, pv.y, x1), qv.y);
    // the diagonal of P' (REG) for the blocks of M; z above read pv
    double pm0 = pv.x, pm1 = pv.y;
    if constexpr (REG) { pm0 = polish_reg_add(pv.x, reg); pm1 = polish_reg_add(pv.y, reg); }

    bool ok = true;
    double r[8];   // QCQP: (d0, d1) of q_2k, q_2k+1, l_n, mu; box-like: (coordinate 0, coordinate 1) of q, a, b
    if constexpr (KIND == 1) {
        const double rad = ln * mc;
        double D[3], m[4], ua, ub;
        polish_disc_jacobian(z0, z1, rad, D);
        const bool on = newton_disc_u(z0, z1, rad, ua, ub);
        newton_contact_block(D, pm0, pm1, m);
#pragma unroll
        for (int col = 0; col < 4; ++col) {
            const int which = col < 2 ? 0 : col - 1;
            const bool ha = col != 1, hb = col == 1;
            r[2 * col] = newton_jac_contact_rhs(D[0], D[1], on, ua, ln, mc, which, ha, hb);
            r[2 * col + 1] = newton_jac_contact_rhs(D[1], D[2], on, ub, ln, mc, which, ha, hb);
            ok = polish_solve2(m[0], m[1], m[2], m[3], r[2 * col], r[2 * col + 1]) && ok;
        }
    } else {
        const int st0 = newton_box_state<KIND>(z0, av.x, bv.x, cv.x), st1 = newton_box_state<KIND>(z1, av.y, bv.y, cv.y);
        const double m0 = st0 == kNewtonFree ? pm0 : 1.0, m1 = st1 == kNewtonFree ? pm1 : 1.0;
#pragma unroll
        for (int which = 0; which < (KIND == 0 ? 1 : 3); ++which) {
            r[2 * which] = newton_jac_box_rhs(st0, which, true);
            r[2 * which + 1] = newton_jac_box_rhs(st1, which, true);
            ok = polish_solve1(m0, r[2 * which]) && ok;
            ok = polish_solve1(m1, r[2 * which + 1]) && ok;
        }
    }
    const bool failed = bad || (__ballot(valid && !ok) & mine) != 0ull;   // a failed block fails its problem
    if (!valid) return;
    if (j == 0 && a.status != nullptr) a.status[first + pl] = bad ? 2 : (failed ? 1 : 0);
    if constexpr (KIND == 1) {
        if (a.Jq != nullptr) {   // rows 2k and 2k+1 of (B,N,2): (d0 of q_2k, d0 of q_2k+1), (d1 of q_2k, d1 of q_2k+1)
            jstore2(a.Jq + 2 * co, failed, r[0], r[2]);
            jstore2(a.Jq + 2 * co + 2, failed, r[1], r[3]);
        }
        if (a.Ja != nullptr) jstore2(a.Ja + co, failed, r[4], r[5]);
        if (a.Jb != nullptr) jstore2(a.Jb + co, failed, r[6], r[7]);
    } else {
        if (a.Jq != nullptr) jstore2(a.Jq + co, failed, r[0], r[1]);
        if constexpr (KIND >= 2) {
            if (a.Ja != nullptr) jstore2(a.Ja + co, failed, r[2], r[3]);
            if (a.Jb != nullptr) jstore2(a.Jb + co, failed, r[4], r[5]);
        }
    }
}

#if DQQ_REG_UNIT
hipError_t launch_newton_jac_diag_reg(int kind, const NewtonJacArgs& a, double reg, hipStream_t s)
{
#else
hipError_t launch_newton_jac_diag(int kind, const NewtonJacArgs& a, hipStream_t s)
{
    const double reg = 0.0;
#endif
    return launch_diag(kind, a.N, a.B, s,
                       [](auto k, auto n) { return newton_jac_diag_kernel<decltype(k)::value, decltype(n)::value, kDiagWPB, kRegUnit>; }, a, reg);
}

} // namespace dqq
