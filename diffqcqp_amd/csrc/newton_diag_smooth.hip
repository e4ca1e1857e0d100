// newton_diag_smooth.hip -- dqq_newton_bwd_smooth_f64 / dqq_newton_jvp_smooth_f64 (kappa > 0) with DQQ_P_DIAG: smooth_core.h's
// newton_bwd_problem_smooth / newton_jvp_problem_smooth on the compact diagonal (B,N).  newton_diag.hip's tile, loads, stores and
// launch geometry: a wave64 owns 128/N consecutive problems, lane = (problem, coordinate pair / contact), no loop and no LDS, two
// ballots per problem (an input that is not finite, a failed pivot).  The lane's block of M is still 1 x 1 or 2 x 2; D and E are
// those of PI_k (smooth_box_at / smooth_disc), so no coordinate is "free" or "on a bound": every gradient entry is a product.
// The proximal weight is looked at at run time (polish_reg).  kappa == 0 never gets here: capi.hip sends it to newton_diag*.hip.
#include "diag_tile.h"
#include "smooth_core.h"

namespace dqq {

typedef double newton_v2d __attribute__((ext_vector_type(2)));   // one 16-byte non-temporal store

template <int KIND, bool JVP, int N, int WPB>
__global__ __launch_bounds__(64 * WPB) void newton_diag_smooth_kernel(const NewtonArgs a, const NewtonSmoothOpts o)
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
        bad = bad || !fin2(av) || !fin2(bv);   // one-sided boxes are not admitted under smoothing
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
    // the diagonal of P' for the blocks of M; z above read pv
    const double pm0 = polish_reg(pv.x, o.reg), pm1 = polish_reg(pv.y, o.reg);
    double m[4] = {1.0, 0.0, 0.0, 1.0};
    SmoothDisc sd = {};
    SmoothBox b0 = {}, b1 = {};
    if constexpr (KIND == 1) {
        sd = smooth_disc(z0, z1, ln * mc, kappa);
        newton_contact_block(sd.D, pm0, pm1, m);
    } else {
        b0 = smooth_box_at<KIND>(z0, av.x, bv.x, cv.x, kappa);
        b1 = smooth_box_at<KIND>(z1, av.y, bv.y, cv.y, kappa);
        m[0] = smooth_box_entry(true, b0.D, pm0);
        m[3] = smooth_box_entry(true, b1.D, pm1);
    }

    double d0, d1;
    bool ok;
    if constexpr (JVP) {
        const double t0 = newton_t(polish_acc(0.0, i0.x, x0), i1.x), t1 = newton_t(polish_acc(0.0, i0.y, x1), i1.y);
        if constexpr (KIND == 1) {
            const double drad = newton_drad(ln, mc, s2, s3);
            d0 = newton_contact_rhs(sd.D[0], sd.D[1], t0, t1, sd.on, sd.ea, drad);
            d1 = newton_contact_rhs(sd.D[1], sd.D[2], t0, t1, sd.on, sd.eb, drad);
            ok = polish_solve2(m[0], m[1], m[2], m[3], d0, d1);
        } else {
            d0 = smooth_box_rhs(b0.D, t0, b0.elo, i2.x, b0.ehi, i3.x);
            d1 = smooth_box_rhs(b1.D, t1, b1.elo, i2.y, b1.ehi, i3.y);
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
            v0 = newton_contact_v(sd.D[0], sd.D[1], d0, d1);
            v1 = newton_contact_v(sd.D[1], sd.D[2], d0, d1);
            const double t = newton_contact_t(sd.ea, sd.eb, d0, d1);
            ga0 = sd.on ? newton_mul(mc, t) : 0.0;
            gb0 = sd.on ? newton_mul(ln, t) : 0.0;
        } else {
            v0 = newton_mul(b0.D, d0);
            v1 = newton_mul(b1.D, d1);
            ga0 = newton_mul(b0.elo, d0);
            ga1 = newton_mul(b1.elo, d1);
            gb0 = newton_mul(b0.ehi, d0);
            gb1 = newton_mul(b1.ehi, d1);
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
static hipError_t launch_mode(int kind, const NewtonArgs& a, const NewtonSmoothOpts& o, hipStream_t s)
{
    return launch_diag(kind, a.N, a.B, s,
                       [](auto k, auto n) { return newton_diag_smooth_kernel<decltype(k)::value, JVP, decltype(n)::value, kDiagWPB>; },
                       a, o);
}

hipError_t launch_newton_diag_smooth(int kind, bool jvp, const NewtonArgs& a, const NewtonSmoothOpts& o, hipStream_t s)
{
    return jvp ? launch_mode<true>(kind, a, o, s) : launch_mode<false>(kind, a, o, s);
}

} // namespace dqq
