// newton_diag.hip -- dqq_newton_bwd_f64 / dqq_newton_jvp_f64 with DQQ_P_DIAG: P (and dP, grad_P) the compact diagonal (B,N).
// polish_diag.hip's tile: a wave64 owns 128/N consecutive problems, lane = (problem, coordinate pair / contact); every (B,N)
// vector is one 16-byte access per lane at an even element offset, so a batch slice is a valid argument.
//
// With P diagonal the matrix M of newton_core.h is diagonal (QP, box kinds) or 2 x 2 per contact (QCQP): a lane solves its own
// block, or the block's transpose, once in registers with polish_solve1 / polish_solve2 -- the general elimination's operations
// on that block, so a diagonal P handed to newton_dense.hip as (B,N,N) gives the same bits.  There is no loop and no LDS: what
// the lanes of a problem share is whether an input was not finite and whether a pivot failed (two ballots).  The mode is a
// template parameter: the JVP reads four tangents and writes dx, the backward reads grad_x and writes up to four gradients, the
// compact grad_P with non-temporal stores (nothing reads it again here).
#include "diag_tile.h"
#include "newton_core.h"

// The proximal weight (polish_core.h): REG is a template parameter of every kernel here.  This file compiles the REG = false
// instantiations, which never read `reg`; newton_diag_reg.hip defines DQQ_REG_UNIT and includes this file for the REG = true ones,
// which add reg to the diagonal entries of P where the thread that owns the entry forms M.
#ifndef DQQ_REG_UNIT
#define DQQ_REG_UNIT 0
#endif

namespace dqq {

constexpr bool kRegUnit = DQQ_REG_UNIT != 0;

typedef double newton_v2d __attribute__((ext_vector_type(2)));   // one 16-byte non-temporal store

template <int KIND, bool JVP, int N, int WPB, bool REG>
__global__ __launch_bounds__(64 * WPB) void newton_diag_kernel(const NewtonArgs a, const double reg)
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
    auto load2 = [&](const double* p) { return valid && p != nullptr ? *reinterpret_cast<const double2*>(p + co) : zero2; };
    auto load1 = [&](const double* p) { return valid && p != nullptr ? p[cc] : 0.0; };

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
    // the mode's inputs: tangents (NULL reads as zeros) or the cotangent
    const double2 i0 = load2(a.in0);
    double2 i1 = zero2, i2 = zero2, i3 = zero2;
    double s2 = 0.0, s3 = 0.0;
    bad = bad || !fin2(i0);
    if constexpr (JVP) {
        i1 = load2(a.in1);
        bad = bad || !fin2(i1);
        if constexpr (KIND == 1) {
            s2 = load1(a.in2);
            s3 = load1(a.in3);
            bad = bad || !__builtin_isfinite(s2) || !__builtin_isfinite(s3);
        }
        if constexpr (KIND >= 2) {
            i2 = load2(a.in2);
            i3 = load2(a.in3);
            bad = bad || !fin2(i2) || !fin2(i3);
        }
    }
    bad = (__ballot(bad) & mine) != 0ull;

    const double x0 = xv.x, x1 = xv.y;
    const double z0 = polish_z(x0, polish_acc(0.0, pv.x, x0), qv.x);
    const double z1 = polish_z(x1, polish_acc(0.0, pv.y, x1), qv.y);
    // the diagonal of P' (REG) for the blocks of M; z above read pv
    double pm0 = pv.x, pm1 = pv.y;
    if constexpr (REG) { pm0 = polish_reg_add(pv.x, reg); pm1 = polish_reg_add(pv.y, reg); }
    double D[3] = {0.0, 0.0, 0.0}, m[4] = {1.0, 0.0, 0.0, 1.0}, ua = 0.0, ub = 0.0;
    bool on = false;
    int st0 = kNewtonFree, st1 = kNewtonFree;
    if constexpr (KIND == 1) {
        const double rad = ln * mc;
        polish_disc_jacobian(z0, z1, rad, D);
        on = newton_disc_u(z0, z1, rad, ua, ub);
        newton_contact_block(D, pm0, pm1, m);
    } else {
        st0 = newton_box_state<KIND>(z0, av.x, bv.x, cv.x);
        st1 = newton_box_state<KIND>(z1, av.y, bv.y, cv.y);
        m[0] = st0 == kNewtonFree ? pm0 : 1.0;
        m[3] = st1 == kNewtonFree ? pm1 : 1.0;
    }

    double d0, d1;
    bool ok;
    if constexpr (JVP) {
        const double t0 = newton_t(polish_acc(0.0, i0.x, x0), i1.x), t1 = newton_t(polish_acc(0.0, i0.y, x1), i1.y);
        if constexpr (KIND == 1) {
            const double drad = newton_drad(ln, mc, s2, s3);
            d0 = newton_contact_rhs(D[0], D[1], t0, t1, on, ua, drad);
            d1 = newton_contact_rhs(D[1], D[2], t0, t1, on, ub, drad);
            ok = polish_solve2(m[0], m[1], m[2], m[3], d0, d1);
        } else {
            d0 = newton_box_rhs(st0, t0, i2.x, i3.x);
            d1 = newton_box_rhs(st1, t1, i2.y, i3.y);
            ok = polish_solve1(m[0], d0);
            ok = polish_solve1(m[3], d1) && ok;
        }
    } else {
        d0 = i0.x;
        d1 = i0.y;
        if constexpr (KIND == 1) {
            ok = polish_solve2(m[0], m[2], m[1], m[3], d0, d1);   // the transposed block
        } else {
            ok = polish_solve1(m[0], d0);
            ok = polish_solve1(m[3], d1) && ok;
        }
    }
    const bool failed = bad || (__ballot(valid && !ok) & mine) != 0ull;   // a failed block fails its problem
    if (!valid) return;
    const double nan = newton_nan();
    if (j == 0 && a.status != nullptr) a.status[first + pl] = bad ? 2 : (failed ? 1 : 0);
    if constexpr (JVP) {
        *reinterpret_cast<double2*>(a.out0 + co) = failed ? make_double2(nan, nan) : make_double2(d0, d1);
    } else {
        double v0, v1, ga0 = 0.0, ga1 = 0.0, gb0 = 0.0, gb1 = 0.0;
        if constexpr (KIND == 1) {
            v0 = newton_contact_v(D[0], D[1], d0, d1);
            v1 = newton_contact_v(D[1], D[2], d0, d1);
            const double t = newton_contact_t(ua, ub, d0, d1);
            ga0 = on ? newton_mul(mc, t) : 0.0;
            gb0 = on ? newton_mul(ln, t) : 0.0;
        } else {
            v0 = st0 == kNewtonFree ? d0 : 0.0;
            v1 = st1 == kNewtonFree ? d1 : 0.0;
            ga0 = st0 == kNewtonLo ? d0 : 0.0;
            ga1 = st1 == kNewtonLo ? d1 : 0.0;
            gb0 = st0 == kNewtonHi ? d0 : 0.0;
            gb1 = st1 == kNewtonHi ? d1 : 0.0;
        }
        if (a.out0 != nullptr) {
            newton_v2d gp;
            gp.x = failed ? nan : newton_gP(v0, x0);
            gp.y = failed ? nan : newton_gP(v1, x1);
            __builtin_nontemporal_store(gp, reinterpret_cast<newton_v2d*>(a.out0 + co));
        }
        if (a.out1 != nullptr) *reinterpret_cast<double2*>(a.out1 + co) = failed ? make_double2(nan, nan) : make_double2(-v0, -v1);
        if constexpr (KIND == 1) {
            if (a.out2 != nullptr) a.out2[cc] = failed ? nan : ga0;
            if (a.out3 != nullptr) a.out3[cc] = failed ? nan : gb0;
        }
        if constexpr (KIND >= 2) {
            if (a.out2 != nullptr) *reinterpret_cast<double2*>(a.out2 + co) = failed ? make_double2(nan, nan) : make_double2(ga0, ga1);
            if (a.out3 != nullptr) *reinterpret_cast<double2*>(a.out3 + co) = failed ? make_double2(nan, nan) : make_double2(gb0, gb1);
        }
    }
}

template <bool JVP>
static hipError_t launch_mode(int kind, const NewtonArgs& a, double reg, hipStream_t s)
{
    return launch_diag(kind, a.N, a.B, s,
                       [](auto k, auto n) { return newton_diag_kernel<decltype(k)::value, JVP, decltype(n)::value, kDiagWPB, kRegUnit>; },
                       a, reg);
}

#if DQQ_REG_UNIT
hipError_t launch_newton_diag_reg(int kind, bool jvp, const NewtonArgs& a, double reg, hipStream_t s)
{
#else
hipError_t launch_newton_diag(int kind, bool jvp, const NewtonArgs& a, hipStream_t s)
{
    const double reg = 0.0;
#endif
    return jvp ? launch_mode<true>(kind, a, reg, s) : launch_mode<false>(kind, a, reg, s);
}

} // namespace dqq
