// jvp_diag.hip -- dqq_jvp_f64 with DQQ_P_DIAG, the forward-mode form of bwd_diag.hip's fast path: P and dP are the compact
// diagonals (B,N), a wave64 owns a tile of 128/N consecutive problems, lane = (problem, coordinate pair / contact).
//
// A streaming kernel: per problem it reads P, dP (N each), q, dq, x (and the kind's extras and their tangents) and writes dx
// (N doubles); there is no grad_P stream.  Every vector is one coalesced 16-byte access per lane at an even element offset
// (DESIGN.md section 2), so a batch slice is a valid argument.  With P diagonal the system is block diagonal (kkt_core.h): one
// block per coordinate (QP, box kinds) or contact (QCQP) in a lane's registers, the refinement given the TRANSPOSED block
// (bwd_systems.h: forward mode), and the problem-wide residual norm summed from LDS in the reference's entry order, so that
// the loop exits where the general kernels' (jvp_dense.hip) do.
//
// Compile with -ffp-contract=off (see kkt_core.h).
#include "diag_tile.h"
#include "kkt_core.h"
#include "sbox_bounds.h"

namespace dqq {

// (dP x)_i of a diagonal dP, as the index-order sum of the full product leaves it: +0.0 plus the one term that is not an exact zero
static DQQ_D double diag_dpx(double dp, double x)
{
#pragma clang fp contract(off)
    return 0.0 + dp * x;
}

template <int KIND, int N, int WPB>
__global__ __launch_bounds__(64 * WPB) void jvp_diag_kernel(
    const double* __restrict__ P, const double* __restrict__ q, const double* __restrict__ a, const double* __restrict__ b,
    const double* __restrict__ v_sign, const double* __restrict__ x, const double* __restrict__ dP,
    const double* __restrict__ dq, const double* __restrict__ da, const double* __restrict__ db, double* __restrict__ dx,
    long B, double dual_eps, int* __restrict__ ir_steps)
{
    constexpr int HL = N / 2;          // lanes per problem
    constexpr int T = 64 / HL;         // problems per wave tile (T*N == 128)
    constexpr int NC = N / 2;          // contacts per problem
    constexpr int RS = (KIND == 0) ? N : (KIND >= 2 ? 3 * N : N + NC); // residual entries per problem
    static_assert(N >= 2 && (N & (N - 1)) == 0 && N <= 128, "N must be a power of two");
    __shared__ __attribute__((aligned(16))) double s_rs[WPB][T * RS];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long first = ((long)blockIdx.x * WPB + wave) * T;
    if (first >= B) return; // whole wave leaves; no workgroup barrier is used below
    const int nvalid = (B - first) < T ? (int)(B - first) : T;
    const int pl = lane / HL, j = lane % HL;
    const bool valid = pl < nvalid;
    double* rs = s_rs[wave];

    const long co = first * N + 2 * lane;
    const double2 zero2 = make_double2(0.0, 0.0);
    const double2 pv = valid ? *reinterpret_cast<const double2*>(P + co) : make_double2(1.0, 1.0);
    const double2 qv = valid ? *reinterpret_cast<const double2*>(q + co) : zero2;
    const double2 xv = valid ? *reinterpret_cast<const double2*>(x + co) : zero2;
    const double2 dpv = (valid && dP != nullptr) ? *reinterpret_cast<const double2*>(dP + co) : zero2;
    const double2 dqv = (valid && dq != nullptr) ? *reinterpret_cast<const double2*>(dq + co) : zero2;
    const double t0 = jvp_coord(diag_dpx(dpv.x, xv.x), dqv.x), t1 = jvp_coord(diag_dpx(dpv.y, xv.y), dqv.y);
    double dx0, dx1;
    int steps = 0;
    IrControl ctl;
    ctl.init();
    bool done = !valid;

    if (KIND == 0) {
        // the QP's blocks are 1 x 1 (P_ii, or x_i with a zero right-hand side): their own transposes
        QpCoord c0, c1;
        c0.setup(pv.x, qv.x, xv.x, t0, dual_eps);
        c1.setup(pv.y, qv.y, xv.y, t1, dual_eps);
        for (int it = 0; it < kIrMaxIter; ++it) {
            if (!done) {
                rs[pl * RS + 2 * j] = c0.step();
                rs[pl * RS + 2 * j + 1] = c1.step();
            }
            wave_lds_fence();
            if (!done) {
                double s = 0.0;
                for (int i = 0; i < RS; ++i) s += rs[pl * RS + i]; // reference entry order
                steps = it + 1;
                if (ctl.update(sqrt(s))) done = true;
            }
            wave_lds_fence();
            if (__all(done)) break;
        }
        dx0 = c0.dl();
        dx1 = c1.dl();
    } else if (KIND >= 2) {
        double2 lov = valid ? *reinterpret_cast<const double2*>(a + co) : zero2;
        double2 hiv = valid ? *reinterpret_cast<const double2*>(b + co) : zero2;
        double2 dlo = (valid && da != nullptr) ? *reinterpret_cast<const double2*>(da + co) : zero2;
        double2 dhi = (valid && db != nullptr) ? *reinterpret_cast<const double2*>(db + co) : zero2;
        if constexpr (KIND == 3) {
            const double2 vv = valid ? *reinterpret_cast<const double2*>(v_sign + co) : zero2;
            const SBoxBounds b0 = sbox_bounds(lov.x, hiv.x, vv.x), b1 = sbox_bounds(lov.y, hiv.y, vv.y);
            lov = make_double2(b0.lo, b1.lo);
            hiv = make_double2(b0.hi, b1.hi);
            dlo = make_double2(b0.keep_lo ? dlo.x : 0.0, b1.keep_lo ? dlo.y : 0.0);
            dhi = make_double2(b0.keep_hi ? dhi.x : 0.0, b1.keep_hi ? dhi.y : 0.0);
        }
        // the dual recovery is not part of the linear map: bwd_diag.hip's, unchanged
        BoxCoord c0, c1;
        c0.setup_dual(pv.x, qv.x, xv.x, lov.x, hiv.x, dual_eps);
        c1.setup_dual(pv.y, qv.y, xv.y, lov.y, hiv.y, dual_eps);
        int steps_dual = 0;
        for (int it = 0; it < kIrMaxIter; ++it) {
            if (!done) {
                double d0[3], d1[3];
                c0.step_dual(d0);
                c1.step_dual(d1);
                rs[pl * RS + 4 * j] = d0[0]; rs[pl * RS + 4 * j + 1] = d0[1];
                rs[pl * RS + 4 * j + 2] = d1[0]; rs[pl * RS + 4 * j + 3] = d1[1];
            }
            wave_lds_fence();
            if (!done) {
                double s = 0.0;
                for (int i = 0; i < 2 * N; ++i) s += rs[pl * RS + i]; // multipliers, coordinate by coordinate
                steps_dual = it + 1;
                if (ctl.update(sqrt(s))) done = true;
            }
            wave_lds_fence();
            if (__all(done)) break;
        }
        c0.finish_dual();
        c1.finish_dual();
        // A = [[0, B],[Id2, P]] restricted to (lower, upper, l), as it stands: the transpose of what the backward hands over
        {
            const double sL = c0.aL ? -1.0 : 0.0, sU = c0.aU ? 1.0 : 0.0;
            const double gam[2] = {c0.gamma_lo, c0.gamma_hi};
            const double A[3][3] = {{0.0, 0.0, c0.gamma_lo * sL}, {0.0, 0.0, c0.gamma_hi * sU}, {sL, sU, pv.x}};
            const double s[3] = {c0.aL ? box_jvp_mult(0, 1, gam, dlo.x, dhi.x) : 0.0,
                                 c0.aU ? box_jvp_mult(1, 1, gam, dlo.x, dhi.x) : 0.0, t0};
            c0.ir.setup(A, s);
        }
        {
            const double sL = c1.aL ? -1.0 : 0.0, sU = c1.aU ? 1.0 : 0.0;
            const double gam[2] = {c1.gamma_lo, c1.gamma_hi};
            const double A[3][3] = {{0.0, 0.0, c1.gamma_lo * sL}, {0.0, 0.0, c1.gamma_hi * sU}, {sL, sU, pv.y}};
            const double s[3] = {c1.aL ? box_jvp_mult(0, 1, gam, dlo.y, dhi.y) : 0.0,
                                 c1.aU ? box_jvp_mult(1, 1, gam, dlo.y, dhi.y) : 0.0, t1};
            c1.ir.setup(A, s);
        }
        ctl.init();
        done = !valid;
        for (int it = 0; it < kIrMaxIter; ++it) {
            if (!done) {
                double d0[3], d1[3];
                c0.step_derivative(d0);
                c1.step_derivative(d1);
                rs[pl * RS + 4 * j] = d0[0]; rs[pl * RS + 4 * j + 1] = d0[1];
                rs[pl * RS + 4 * j + 2] = d1[0]; rs[pl * RS + 4 * j + 3] = d1[1];
                rs[pl * RS + 2 * N + 2 * j] = d0[2];
                rs[pl * RS + 2 * N + 2 * j + 1] = d1[2];
            }
            wave_lds_fence();
            if (!done) {
                double s = 0.0;
                for (int i = 0; i < RS; ++i) s += rs[pl * RS + i]; // multipliers, then the l entries
                steps = it + 1;
                if (ctl.update(sqrt(s))) done = true;
            }
            wave_lds_fence();
            if (__all(done)) break;
        }
        dx0 = c0.dl();
        dx1 = c1.dl();
        if (valid && ir_steps != nullptr && j == 0) ir_steps[2 * (first + pl)] = steps_dual;
    } else {
        const long cc = first * NC + lane;
        const double ln = valid ? a[cc] : 1.0, mc = valid ? b[cc] : 1.0;
        const double dln = (valid && da != nullptr) ? da[cc] : 0.0, dmu = (valid && db != nullptr) ? db[cc] : 0.0;
        const QcqpDual ct = qcqp_contact(xv.x, xv.y, pv.x * xv.x + qv.x, pv.y * xv.y + qv.y, ln, mc, dual_eps);
        const double ca = 2 * xv.x, cb = 2 * xv.y;                       // C
        const double Da = 2 * ct.gamma + pv.x, Db = 2 * ct.gamma + pv.y; // D_tild + P
        SmallIr ir;
        if (ct.act) {
            // A = [[S, (gamma C^T)],[C, D_tild + P]] of the contact, as it stands
            const double A[3][3] = {{ct.S, ct.gamma * ca, ct.gamma * cb}, {ca, Da, 0.0}, {cb, 0.0, Db}};
            const double s[3] = {qcqp_jvp_mult(QcqpContact::e2(ct.gamma, ln, mc), dln, QcqpContact::e1(ct.gamma, ln, mc), dmu), t0, t1};
            ir.setup(A, s);
        } else {
            const double A[3][3] = {{0.0, 0.0, 0.0}, {0.0, Da, 0.0}, {0.0, 0.0, Db}};
            const double s[3] = {0.0, t0, t1};
            ir.setup(A, s);
        }
        for (int it = 0; it < kIrMaxIter; ++it) {
            if (!done) {
                double dsq[3];
                ir.step(dsq);
                rs[pl * RS + j] = dsq[0];
                rs[pl * RS + NC + 2 * j] = dsq[1];
                rs[pl * RS + NC + 2 * j + 1] = dsq[2];
            }
            wave_lds_fence();
            if (!done) {
                double s = 0.0;
                for (int i = 0; i < RS; ++i) s += rs[pl * RS + i]; // gamma entries, then l entries
                steps = it + 1;
                if (ctl.update(sqrt(s))) done = true;
            }
            wave_lds_fence();
            if (__all(done)) break;
        }
        dx0 = ir.xs[1];
        dx1 = ir.xs[2];
    }
    if (valid) {
        *reinterpret_cast<double2*>(dx + co) = make_double2(dx0, dx1);
        if (ir_steps != nullptr && j == 0) ir_steps[KIND >= 2 ? 2 * (first + pl) + 1 : first + pl] = steps;
    }
}

hipError_t launch_jvp_diag(int kind, const JvpArgs& a, hipStream_t s)
{
    // (this kernel takes its pointers and scalars one by one, not an argument struct)
    return launch_diag(kind, a.N, a.B, s,
                       [](auto k, auto n) { return jvp_diag_kernel<decltype(k)::value, decltype(n)::value, kDiagWPB>; }, a.P, a.q, a.a,
                       a.b, a.v, a.x, a.dP, a.dq, a.da, a.db, a.dx, a.B, a.epsilon, a.ir_steps);
}

} // namespace dqq
