// polish_diag.hip -- dqq_polish_f64 with DQQ_P_DIAG: P is the compact diagonal (B,N).  jvp_diag.hip's tile: a wave64 owns
// 128/N consecutive problems, lane = (problem, coordinate pair / contact); every vector is one 16-byte access per lane at an
// even element offset, so a batch slice is a valid argument.
//
// With P diagonal the Newton matrix M of polish_core.h is diagonal (QP, box kinds) or 2 x 2 per contact (QCQP): a lane solves
// its own block in registers with polish_solve1 / polish_solve2 -- the general elimination's pivot rule and operations on that
// block, so a diagonal P handed to polish_dense.hip as (B,N,N) gives the same bits.  What the lanes of a problem share is the
// residual r (the |F| of a problem go through the wave's LDS slice and every lane takes their maximum in index order) and
// whether a block's pivot failed (a ballot).  The Newton loop runs per problem: a problem that has stopped is masked, the wave
// goes on until its last problem has stopped; nothing here waits for another wave.
#include "diag_tile.h"
#include "polish_core.h"

// The proximal weight (polish_core.h): REG is a template parameter of every kernel here.  This file compiles the REG = false
// instantiations, which never read `reg`; polish_diag_reg.hip defines DQQ_REG_UNIT and includes this file for the REG = true ones,
// which add reg to the diagonal entries of P where the thread that owns the entry forms M.
#ifndef DQQ_REG_UNIT
#define DQQ_REG_UNIT 0
#endif

namespace dqq {

constexpr bool kRegUnit = DQQ_REG_UNIT != 0;

template <int KIND, int N, int WPB, bool REG>
__global__ __launch_bounds__(64 * WPB) void polish_diag_kernel(const PolishArgs a, const double reg)
{
#pragma clang fp contract(off)
    constexpr int HL = N / 2;          // lanes per problem
    constexpr int T = 64 / HL;         // problems per wave tile (T*N == 128)
    static_assert(N >= 2 && (N & (N - 1)) == 0 && N <= 64, "N must be a power of two up to 64");
    __shared__ __attribute__((aligned(16))) double s_rs[WPB][T * N];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long first = ((long)blockIdx.x * WPB + wave) * T;
    if (first >= a.B) return; // whole wave leaves; no workgroup barrier is used below
    const int nvalid = (a.B - first) < T ? (int)(a.B - first) : T;
    const int pl = lane / HL, j = lane % HL;
    const bool valid = pl < nvalid;
    double* rs = s_rs[wave] + pl * N;
    const unsigned long long mine = (HL == 64 ? ~0ull : ((1ull << HL) - 1ull)) << (pl * HL);   // the lanes of this problem

    const long co = first * N + 2 * lane;
    const double2 zero2 = make_double2(0.0, 0.0);
    const double2 pv = valid ? *reinterpret_cast<const double2*>(a.P + co) : make_double2(1.0, 1.0);
    const double2 qv = valid ? *reinterpret_cast<const double2*>(a.q + co) : zero2;
    const double2 xv = valid ? *reinterpret_cast<const double2*>(a.x + co) : zero2;
    bool bad = !__builtin_isfinite(pv.x) || !__builtin_isfinite(pv.y) || !__builtin_isfinite(qv.x) || !__builtin_isfinite(qv.y) ||
               !__builtin_isfinite(xv.x) || !__builtin_isfinite(xv.y);
    double lo0 = 0.0, hi0 = 0.0, lo1 = 0.0, hi1 = 0.0, rad = 0.0;
    if constexpr (KIND == 1) {
        const long cc = first * HL + lane;   // (B,N/2): element by element
        const double ln = valid ? a.a[cc] : 1.0, mc = valid ? a.b[cc] : 1.0;
        bad = bad || !__builtin_isfinite(ln) || !__builtin_isfinite(mc);
        rad = ln * mc;
    } else {
        double2 av = zero2, bv = zero2, cv = zero2;
        if constexpr (KIND >= 2) {
            av = valid ? *reinterpret_cast<const double2*>(a.a + co) : zero2;
            bv = valid ? *reinterpret_cast<const double2*>(a.b + co) : zero2;
            const bool io = a.inf_bounds != 0;   // kernel-uniform: one-sided boxes admitted (polish_core.h)
            bad = bad || polish_lo_bad(av.x, io) || polish_lo_bad(av.y, io) || polish_hi_bad(bv.x, io) || polish_hi_bad(bv.y, io);
        }
        if constexpr (KIND == 3) {
            cv = valid ? *reinterpret_cast<const double2*>(a.c + co) : zero2;
            bad = bad || !__builtin_isfinite(cv.x) || !__builtin_isfinite(cv.y);
        }
        polish_bounds<KIND>(av.x, bv.x, cv.x, lo0, hi0);
        polish_bounds<KIND>(av.y, bv.y, cv.y, lo1, hi1);
    }
    bad = (__ballot(bad) & mine) != 0ull;
    // the diagonal of P' (REG) for the blocks of M; z and F below read pv
    double pm0 = pv.x, pm1 = pv.y;
    if constexpr (REG) { pm0 = polish_reg_add(pv.x, reg); pm1 = polish_reg_add(pv.y, reg); }

    // z and F of the lane's two coordinates at (x0, x1)
    auto eval = [&](double x0, double x1, double& z0, double& z1, double& F0, double& F1) {
        z0 = polish_z(x0, polish_acc(0.0, pv.x, x0), qv.x);
        z1 = polish_z(x1, polish_acc(0.0, pv.y, x1), qv.y);
        if constexpr (KIND == 1) {
            polish_F_contact(x0, x1, z0, z1, rad, F0, F1);
        } else {
            F0 = polish_F<KIND>(x0, z0, lo0, hi0);
            F1 = polish_F<KIND>(x1, z1, lo1, hi1);
        }
    };
    // the problem's r: every lane of the problem, from the problem's LDS slice in index order
    auto residual = [&](double F0, double F1, bool on) {
        if (on) { rs[2 * j] = F0; rs[2 * j + 1] = F1; }
        wave_lds_fence();
        double r = 0.0;
        if (on)
            for (int i = 0; i < N; ++i) r = nmax(r, rs[i]);
        wave_lds_fence();
        return r;
    };

    double x0 = xv.x, x1 = xv.y, z0, z1, F0, F1;
    eval(x0, x1, z0, z1, F0, F1);
    const double r0 = residual(F0, F1, valid);
    double r = r0;
    int steps = 0;
    bool live = valid && !bad && __builtin_isfinite(r0);
    for (int it = 0; it < a.max_steps; ++it) {
        live = live && r != 0.0;
        if (__all(!live)) break;
        double d0 = -F0, d1 = -F1, xn0 = 0.0, xn1 = 0.0, zn0 = 0.0, zn1 = 0.0, Fn0 = 0.0, Fn1 = 0.0;
        bool ok = true;
        if (live) {
            if constexpr (KIND == 1) {
                double D[3];
                polish_disc_jacobian(z0, z1, rad, D);
                ok = polish_solve2(polish_contact_entry(true, D[0], D[0], D[1], pm0, 0.0),
                                   polish_contact_entry(false, D[1], D[0], D[1], 0.0, pm1),
                                   polish_contact_entry(false, D[1], D[1], D[2], pm0, 0.0),
                                   polish_contact_entry(true, D[2], D[1], D[2], 0.0, pm1), d0, d1);
                xn0 = x0 + d0;
                xn1 = x1 + d1;
                check_proj_circle(xn0, xn1, rad);
            } else {
                ok = polish_solve1(polish_free(z0, lo0, hi0) ? pm0 : 1.0, d0);
                ok = polish_solve1(polish_free(z1, lo1, hi1) ? pm1 : 1.0, d1) && ok;
                xn0 = polish_proj<KIND>(x0 + d0, lo0, hi0);
                xn1 = polish_proj<KIND>(x1 + d1, lo1, hi1);
            }
            eval(xn0, xn1, zn0, zn1, Fn0, Fn1);
        }
        const bool failed = (__ballot(live && !ok) & mine) != 0ull;   // a failed block fails the problem's step
        const double rn = residual(Fn0, Fn1, live);
        if (live) {
            if (failed || !(rn < r)) {
                live = false;
            } else {
                x0 = xn0; x1 = xn1; z0 = zn0; z1 = zn1; F0 = Fn0; F1 = Fn1;
                r = rn;
                ++steps;
            }
        }
    }
    if (valid) {
        *reinterpret_cast<double2*>(a.x_out + co) = make_double2(x0, x1);
        if (j == 0) {
            const long b = first + pl;
            if (a.resid != nullptr) { a.resid[2 * b] = r0; a.resid[2 * b + 1] = r; }
            if (a.steps != nullptr) a.steps[b] = steps;
            if (a.status != nullptr) a.status[b] = polish_status(bad, r0, steps);
        }
    }
}

#if DQQ_REG_UNIT
hipError_t launch_polish_diag_reg(int kind, const PolishArgs& a, double reg, hipStream_t s)
{
#else
hipError_t launch_polish_diag(int kind, const PolishArgs& a, hipStream_t s)
{
    const double reg = 0.0;
#endif
    return launch_diag(kind, a.N, a.B, s,
                       [](auto k, auto n) { return polish_diag_kernel<decltype(k)::value, decltype(n)::value, kDiagWPB, kRegUnit>; }, a, reg);
}

} // namespace dqq
