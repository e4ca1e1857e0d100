// jvp_any.hip -- dqq_jvp_f64 on a general P of any size, the forward-mode form of general_any.hip's backward: one 256-thread
// workgroup per problem on a slice of the caller's scratch (any_core.h), the reference's operation order.  The slice, the LDS
// staging and the grid are the backward's (any_bwd_stride, any_grid): the system has the backward's size.  The duals, active
// sets and the matrix are the backward's (bwd_systems.h); the refinement receives the matrix transposed, the right-hand side
// s = R^T(tangents), and dx is read off the solution where the backward placed grad_x.
#include "any_core.h"
#include "launch.h"

namespace dqq {

// The doubles of `vec` any_jvp_problem touches: s, A^T b, K^-1 A^T b, x, a buffer (5 m); gamma, the multiplier rows of s (2 m each);
// S (m); vt, va (n each); 2n + 3 ints.  The slice is the BACKWARD's (any_bwd_stride: any_bwd_vec_doubles): the launcher refuses
// to run if a change of either layout ever breaks "the JVP fits the backward's slice".
static long any_jvp_vec_doubles(int kind, int n)
{
    const long m = bwd_system_rows(kind, n);
    return 10 * m + 2L * n + (2L * n + 3 + 1) / 2;
}

// One problem by one workgroup.  vec: any_bwd_vec_doubles, laid out as any_bwd_problem lays it out (vsm, the multiplier rows
// of s, where dgamma was; vt, the coordinate rows, where dl was).
template <int KIND>
static DQQ_D void any_jvp_problem(const double* __restrict__ P, const double* __restrict__ q, const double* __restrict__ a,
                                  const double* __restrict__ b, const double* __restrict__ v_sign,
                                  const double* __restrict__ x, const double* __restrict__ dP,
                                  const double* __restrict__ dq, const double* __restrict__ da,
                                  const double* __restrict__ db, double* __restrict__ dx, int* __restrict__ ir_steps,
                                  long prob, int n, double dual_eps, double* At, double* K, double* Kinv, double* vec, int t)
{
#pragma clang fp contract(off)
    const int nc = n / 2;
    const int mmax = bwd_system_rows(KIND, n);
    const int ld = mmax | 1;
    double* vdd = vec;                     // mmax: s
    double* vAb = vdd + mmax;
    double* vKAb = vAb + mmax;
    double* xs = vKAb + mmax;
    double* vb = xs + mmax;
    double* vgam = vb + mmax;              // QP / QCQP: n ; box: 2n (lower | upper)
    double* vsm = vgam + 2 * mmax;         // multiplier rows of s, by slot
    double* vS = vsm + 2 * mmax;           // QCQP: nc
    double* vt = vS + mmax;                // n: jvp_coord of every coordinate
    double* va = vt + n;                   // n
    int* perm = reinterpret_cast<int*>(va + n);  // up to 2n + 2 ints
    int* counts = perm + 2 * n + 2;
    const double* Pg = P + prob * (long)n * n;
    const double* xg = x + prob * (long)n;
    const double* qg = q + prob * (long)n;
    double* Pl = K;
    any_load_matrix(Pl, ld, Pg, n, t);
    for (int i = t; i < n; i += kAnyT) {
        const double dpx = dP != nullptr ? any_row_dot(dP + prob * (long)n * n, n, i, xg, n) : 0.0;
        vt[i] = jvp_coord(dpx, dq != nullptr ? dq[prob * (long)n + i] : 0.0);
    }
    DQQ_WG_SYNC();
    int steps = 0, steps_dual = 1;

    if (KIND == 0) {
        for (int i = t; i < n; i += kAnyT) vgam[i] = qp_dual(any_row_dot(Pl, ld, i, xg, n) + qg[i], xg[i], dual_eps);
        DQQ_WG_SYNC();
        if (t == 0) { // the order (active..., inactive...)
            int na = 0;
            for (int i = 0; i < n; ++i) if (qp_active(vgam[i])) perm[na++] = i;
            int p = na;
            for (int i = 0; i < n; ++i) if (!qp_active(vgam[i])) perm[p++] = i;
            counts[0] = na;
        }
        DQQ_WG_SYNC();
        const int na = counts[0], m = n;
        for (long idx = t; idx < (long)m * m; idx += kAnyT) {
            const int rr = (int)(idx / m), cc = (int)(idx % m);
            At[rr * ld + cc] = qp_system_A(rr, cc, na, perm, xg, Pl, ld);
        }
        for (int p = t; p < m; p += kAnyT) vdd[p] = qp_jvp_s(p, na, perm, vt);
        DQQ_WG_SYNC();
        any_ir(At, K, Kinv, vdd, vAb, vKAb, xs, vb, m, ld, t, steps, m);
        for (int p = t; p < m; p += kAnyT) dx[prob * (long)n + perm[p]] = jvp_dx_qp(p, na, xs[p]);
    } else if (KIND == 1) {
        for (int i = t; i < n; i += kAnyT) va[i] = any_row_dot(Pl, ld, i, xg, n) + qg[i];
        DQQ_WG_SYNC();
        for (int c = t; c < nc; c += kAnyT) {
            const double ln = a[prob * (long)nc + c], mc = b[prob * (long)nc + c];
            const QcqpDual ct = qcqp_contact(xg[2 * c], xg[2 * c + 1], va[2 * c], va[2 * c + 1], ln, mc, dual_eps);
            vgam[c] = ct.gamma;
            vS[c] = ct.S;
        }
        DQQ_WG_SYNC();
        if (t == 0) { // the active contacts, in contact order
            int na = 0;
            for (int c = 0; c < nc; ++c)
                if (qcqp_active(vS[c], a[prob * (long)nc + c] * b[prob * (long)nc + c])) perm[na++] = c;
            counts[0] = na;
        }
        DQQ_WG_SYNC();
        const int na = counts[0], m = n + na;
        for (int p = t; p < na; p += kAnyT) {
            const long c = prob * (long)nc + perm[p];
            const double ln = a[c], mc = b[c], gamma = vgam[perm[p]];
            vsm[p] = qcqp_jvp_mult(QcqpContact::e2(gamma, ln, mc), da != nullptr ? da[c] : 0.0, QcqpContact::e1(gamma, ln, mc),
                                   db != nullptr ? db[c] : 0.0);
        }
        for (long idx = t; idx < (long)m * m; idx += kAnyT) {
            const int rr = (int)(idx / m), cc = (int)(idx % m);
            At[rr * ld + cc] = qcqp_system_A(rr, cc, na, perm, vS, vgam, xg, Pl, ld);
        }
        DQQ_WG_SYNC();
        for (int p = t; p < m; p += kAnyT) vdd[p] = system_jvp_s(p, na, vsm, vt);
        DQQ_WG_SYNC();
        any_ir(At, K, Kinv, vdd, vAb, vKAb, xs, vb, m, ld, t, steps, m);
        for (int i = t; i < n; i += kAnyT) dx[prob * (long)n + i] = xs[na + i];
    } else {
        const double* lo = a + prob * (long)n;
        const double* hi = b + prob * (long)n;
        [[maybe_unused]] const double* vs = (KIND == 3) ? v_sign + prob * (long)n : nullptr;
        for (int i = t; i < 2 * n; i += kAnyT) vgam[i] = 0.0;
        if (t == 0) { // not_null bookkeeping: per coordinate, lower before upper
            int nn = 0;
            for (int i = 0; i < n; ++i) {
                double lo_i = lo[i], hi_i = hi[i];
                if constexpr (KIND == 3) { const SBoxBounds eb = sbox_bounds(lo_i, hi_i, vs[i]); lo_i = eb.lo; hi_i = eb.hi; }
                const BoxNotNull bn = box_not_null(xg[i], lo_i, hi_i, dual_eps);
                if (bn.aL) perm[nn++] = i;
                if (bn.aU) perm[nn++] = n + i;
            }
            counts[0] = nn;
        }
        DQQ_WG_SYNC();
        const int nn = counts[0];
        // the dual recovery is not part of the linear map: the backward's, unchanged
        for (int i = t; i < n; i += kAnyT) vdd[i] = box_dual_rhs(Pl + i * ld, xg, n, qg[i]);
        for (long idx = t; idx < (long)n * nn; idx += kAnyT) {
            const int i = (int)(idx / nn), p = (int)(idx % nn);
            At[i * ld + p] = box_dual_At(i, p, perm, n);
        }
        DQQ_WG_SYNC();
        if (nn > 0) {
            any_ir(At, K, Kinv, vdd, vAb, vKAb, xs, vb, nn, ld, t, steps_dual, n);
            for (int p = t; p < nn; p += kAnyT) vgam[perm[p]] = xs[p];
        }
        DQQ_WG_SYNC();
        const int m = nn + n;
        any_load_matrix(Pl, ld, Pg, n, t); // the refinement above used K as workspace
        for (int p = t; p < nn; p += kAnyT) {
            const int id = perm[p], i = id < n ? id : id - n;
            double dlo = da != nullptr ? da[prob * (long)n + i] : 0.0, dhi = db != nullptr ? db[prob * (long)n + i] : 0.0;
            if constexpr (KIND == 3) {
                const SBoxBounds eb = sbox_bounds(lo[i], hi[i], vs[i]);
                dlo = eb.keep_lo ? dlo : 0.0;
                dhi = eb.keep_hi ? dhi : 0.0;
            }
            vsm[p] = box_jvp_mult(id, n, vgam, dlo, dhi);
        }
        DQQ_WG_SYNC();
        for (long idx = t; idx < (long)m * m; idx += kAnyT) {
            const int rr = (int)(idx / m), cc = (int)(idx % m);
            At[rr * ld + cc] = box_system_A(rr, cc, nn, perm, vgam, Pl, ld, n);
        }
        for (int p = t; p < m; p += kAnyT) vdd[p] = system_jvp_s(p, nn, vsm, vt);
        DQQ_WG_SYNC();
        any_ir(At, K, Kinv, vdd, vAb, vKAb, xs, vb, m, ld, t, steps, m);
        for (int i = t; i < n; i += kAnyT) dx[prob * (long)n + i] = xs[nn + i];
    }
    if (ir_steps != nullptr && t == 0) {
        if (KIND >= 2) { ir_steps[2 * prob] = steps_dual; ir_steps[2 * prob + 1] = steps; }
        else ir_steps[prob] = steps;
    }
    DQQ_WG_SYNC();
}

template <int KIND, bool LDS>
__global__ __launch_bounds__(kAnyT) void jvp_any_kernel(
    const double* __restrict__ P, const double* __restrict__ q, const double* __restrict__ a, const double* __restrict__ b,
    const double* __restrict__ v_sign, const double* __restrict__ x, const double* __restrict__ dP,
    const double* __restrict__ dq, const double* __restrict__ da, const double* __restrict__ db, double* __restrict__ dx,
    long B, int n, double dual_eps, int* __restrict__ ir_steps, double* __restrict__ scratch, long scratch_stride)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int t = threadIdx.x;
    double* scr = scratch + (long)blockIdx.x * scratch_stride;
    const long mat = any_mat_doubles(bwd_system_rows(KIND, n));
    double* K = scr;
    double* At = LDS ? smem : scr + mat;
    double* Kinv = LDS ? smem + mat : scr + 2 * mat;
    double* vec = LDS ? scr + mat : scr + 3 * mat;
    for (long w = blockIdx.x; w < B; w += gridDim.x)
        any_jvp_problem<KIND>(P, q, a, b, v_sign, x, dP, dq, da, db, dx, ir_steps, w, n, dual_eps, At, K, Kinv, vec, t);
}

template <int KIND>
static hipError_t launch_jvp_any_kind(const JvpArgs& a, hipStream_t s)
{
    if (a.scratch == nullptr) return hipErrorInvalidValue; // capi.hip checks the workspace before it gets here
    if (any_jvp_vec_doubles(KIND, a.N) > any_bwd_vec_doubles(KIND > 2 ? 2 : KIND, a.N)) return hipErrorInvalidValue;
    const long mat = any_mat_doubles(bwd_system_rows(KIND, a.N));
    const size_t lds = sizeof(double) * 2 * (size_t)mat;
    const long stride = any_bwd_stride(KIND == 0 ? kKindQP : (KIND == 1 ? kKindQCQP : kKindBox), a.N);
    const unsigned grid = any_grid(a.B, stride);
    if (lds <= kAnyLdsBytes)
        return launch_lds(jvp_any_kernel<KIND, true>, dim3(grid), dim3(kAnyT), lds, s, a.P, a.q, a.a, a.b, a.v, a.x, a.dP, a.dq,
                          a.da, a.db, a.dx, a.B, a.N, a.epsilon, a.ir_steps, a.scratch, stride);
    return launch_lds(jvp_any_kernel<KIND, false>, dim3(grid), dim3(kAnyT), 0, s, a.P, a.q, a.a, a.b, a.v, a.x, a.dP, a.dq, a.da,
                      a.db, a.dx, a.B, a.N, a.epsilon, a.ir_steps, a.scratch, stride);
}

hipError_t launch_jvp_any(int kind, const JvpArgs& a, hipStream_t s)
{
    switch (kind) {
    case kKindQP: return launch_jvp_any_kind<0>(a, s);
    case kKindQCQP: return launch_jvp_any_kind<1>(a, s);
    case kKindBox: return launch_jvp_any_kind<2>(a, s);
    case kKindSignedBox: return launch_jvp_any_kind<3>(a, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace dqq
