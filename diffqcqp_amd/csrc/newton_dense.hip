// newton_dense.hip -- dqq_newton_bwd_f64 / dqq_newton_jvp_f64 on a general P (B,N,N): newton_core.h's one elimination by
// team_dense.h's teams, one template with a mode and an LDS / global switch.
//   NewtonTeam (LDS = true, N <= 64): the slice in LDS (the polish's size: one matrix and polish_vec_doubles).
//   NewtonAny (LDS = false, N > 64): a slice of the caller's scratch (dqq_newton_scratch_bytes); the persistent grid of any_grid.
// The slice: the matrix (N x (N|1): P while z is evaluated, then M in place, transposed in place for the backward), then x, z,
// the Jacobian (2N), the right-hand side, the solution, and t = dP x + dq (JVP) or v (backward).
// dP is never resident: a thread reads its row from global memory.  grad_P = -v x' goes straight out, consecutive threads to
// consecutive addresses.
#include "newton_core.h"
#include "team_dense.h"

// The proximal weight (polish_core.h): REG is a template parameter of every kernel here.  This file compiles the REG = false
// instantiations, which never read `reg`; newton_dense_reg.hip defines DQQ_REG_UNIT and includes this file for the REG = true ones,
// which add reg to the diagonal entries of P where the thread that owns the entry forms M.
#ifndef DQQ_REG_UNIT
#define DQQ_REG_UNIT 0
#endif

namespace dqq {

constexpr bool kRegUnit = DQQ_REG_UNIT != 0;

static DQQ_HD long newton_slice_doubles(int n) { return ((long)n * (n | 1) + newton_vec_doubles(n) + 1) & ~1L; }

static DQQ_D bool nfinite_or_null(const double* p, long i) { return p == nullptr || __builtin_isfinite(p[i]); }
static DQQ_D double nread(const double* p, long i) { return p != nullptr ? p[i] : 0.0; }

// One problem by one team.  M: n x ld; vec: newton_vec_doubles(n).
template <int KIND, bool JVP, int T, bool REG>
static DQQ_D void team_newton_problem(const NewtonArgs& a, double reg, long prob, double* M, double* vec, int lane)
{
#pragma clang fp contract(off)
    const int n = a.N, nc = n / 2;
    const idx_t<T> ld = n | 1;
    const int ne = KIND == 1 ? nc : n;   // entries of an extra
    double* xc = vec;
    double* z = xc + n;
    double* dj = z + n;
    double* d = dj + 2 * n;
    double* sol = d + n;
    double* tv = sol + n;
    const double* Pg = a.P + prob * (long)n * n;
    const long vo = prob * n, eo = prob * (long)ne;
    bool bad = false;
    for (idx_t<T> idx = lane; idx < (idx_t<T>)n * n; idx += T) {
        const double v = Pg[idx];
        bad = bad || !__builtin_isfinite(v);
        M[(idx / n) * ld + idx % n] = v;
        if constexpr (JVP) bad = bad || !nfinite_or_null(a.in0, prob * (long)n * n + idx);
    }
    for (int i = lane; i < n; i += T) {
        const double xi = a.x[vo + i];
        xc[i] = xi;
        bad = bad || !__builtin_isfinite(xi) || !__builtin_isfinite(a.q[vo + i]);
        if constexpr (KIND == 3) bad = bad || !__builtin_isfinite(a.c[vo + i]);
        if constexpr (JVP) bad = bad || !nfinite_or_null(a.in1, vo + i);
        else bad = bad || !__builtin_isfinite(a.in0[vo + i]);
    }
    if constexpr (KIND >= 1)
        for (int k = lane; k < ne; k += T) {
            if constexpr (KIND >= 2) bad = bad || polish_lo_bad(a.a[eo + k], a.inf_bounds != 0) || polish_hi_bad(a.b[eo + k], a.inf_bounds != 0);
            else bad = bad || !__builtin_isfinite(a.a[eo + k]) || !__builtin_isfinite(a.b[eo + k]);
            if constexpr (JVP) bad = bad || !nfinite_or_null(a.in2, eo + k) || !nfinite_or_null(a.in3, eo + k);
        }
    bad = team_any<T>(bad);
    team_sync<T>();
    // z, and the JVP's t = dP x + dq: a row per thread
    for (int i = lane; i < n; i += T) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s = polish_acc(s, M[i * ld + j], xc[j]);
        z[i] = polish_z(xc[i], s, a.q[vo + i]);
        if constexpr (JVP) {
            double sd = 0.0;
            if (a.in0 != nullptr) {
                const double* row = a.in0 + (prob * (long)n + i) * n;
                for (int j = 0; j < n; ++j) sd = polish_acc(sd, row[j], xc[j]);
            }
            tv[i] = newton_t(sd, nread(a.in1, vo + i));
        }
    }
    team_sync<T>();
    // the Jacobian and the right-hand side
    if constexpr (KIND == 1) {
        for (int k = lane; k < nc; k += T) {
            const double ln = a.a[eo + k], mc = a.b[eo + k], rad = ln * mc;
            double D[3];
            polish_disc_jacobian(z[2 * k], z[2 * k + 1], rad, D);
            dj[3 * k] = D[0]; dj[3 * k + 1] = D[1]; dj[3 * k + 2] = D[2];
            if constexpr (JVP) {
                double ua, ub;
                const bool on = newton_disc_u(z[2 * k], z[2 * k + 1], rad, ua, ub);
                const double drad = newton_drad(ln, mc, nread(a.in2, eo + k), nread(a.in3, eo + k));
                d[2 * k] = newton_contact_rhs(D[0], D[1], tv[2 * k], tv[2 * k + 1], on, ua, drad);
                d[2 * k + 1] = newton_contact_rhs(D[1], D[2], tv[2 * k], tv[2 * k + 1], on, ub, drad);
            }
        }
    } else {
        for (int i = lane; i < n; i += T) {
            const int st = newton_box_state<KIND>(z[i], KIND >= 2 ? a.a[vo + i] : 0.0, KIND >= 2 ? a.b[vo + i] : 0.0,
                                                  KIND == 3 ? a.c[vo + i] : 0.0);
            dj[i] = (double)st;
            if constexpr (JVP) d[i] = newton_box_rhs(st, tv[i], KIND >= 2 ? nread(a.in2, vo + i) : 0.0, KIND >= 2 ? nread(a.in3, vo + i) : 0.0);
        }
    }
    if constexpr (!JVP)
        for (int i = lane; i < n; i += T) d[i] = a.in0[vo + i];
    team_sync<T>();
    // M in place of P
    if constexpr (KIND == 1) {
        for (idx_t<T> idx = lane; idx < (idx_t<T>)nc * n; idx += T) {
            const int k = (int)(idx / n), j = (int)(idx % n);
            const double* D = dj + 3 * k;
            double pa = M[(2 * k) * ld + j], pb = M[(2 * k + 1) * ld + j];
            if constexpr (REG) {   // the contact's own two diagonal entries of P
                if (j == 2 * k) pa = polish_reg_add(pa, reg);
                if (j == 2 * k + 1) pb = polish_reg_add(pb, reg);
            }
            const double c0 = j == 2 * k ? D[0] : (j == 2 * k + 1 ? D[1] : 0.0);
            const double c1 = j == 2 * k ? D[1] : (j == 2 * k + 1 ? D[2] : 0.0);
            M[(2 * k) * ld + j] = polish_contact_entry(j == 2 * k, c0, D[0], D[1], pa, pb);
            M[(2 * k + 1) * ld + j] = polish_contact_entry(j == 2 * k + 1, c1, D[1], D[2], pa, pb);
        }
    } else {
        for (idx_t<T> idx = lane; idx < (idx_t<T>)n * n; idx += T) {
            const int i = (int)(idx / n), j = (int)(idx % n);
            if (dj[i] != (double)kNewtonFree) M[i * ld + j] = i == j ? 1.0 : 0.0;
            else if constexpr (REG) { if (i == j) M[i * ld + j] = polish_reg_add(M[i * ld + j], reg); }
        }
    }
    team_sync<T>();
    if constexpr (!JVP) {   // M' in place: a pair (i < j) per thread
        for (idx_t<T> idx = lane; idx < (idx_t<T>)n * n; idx += T) {
            const int i = (int)(idx / n), j = (int)(idx % n);
            if (i < j) { const double t = M[i * ld + j]; M[i * ld + j] = M[j * ld + i]; M[j * ld + i] = t; }
        }
        team_sync<T>();
    }
    const bool ok = !bad && team_solve<T>(M, ld, d, sol, n, lane);   // (bad is team-uniform: the team skips the solve together)
    team_sync<T>();
    const double nan = newton_nan();
    if (lane == 0 && a.status != nullptr) a.status[prob] = bad ? 2 : (ok ? 0 : 1);
    if constexpr (JVP) {
        for (int i = lane; i < n; i += T) a.out0[vo + i] = ok ? sol[i] : nan;
    } else {
        // v = D w into tv, the extras' gradients
        if constexpr (KIND == 1) {
            for (int k = lane; k < nc; k += T) {
                const double* D = dj + 3 * k;
                const double wa = sol[2 * k], wb = sol[2 * k + 1];
                tv[2 * k] = newton_contact_v(D[0], D[1], wa, wb);
                tv[2 * k + 1] = newton_contact_v(D[1], D[2], wa, wb);
                const double ln = a.a[eo + k], mc = a.b[eo + k];
                double ua, ub;
                const bool on = newton_disc_u(z[2 * k], z[2 * k + 1], ln * mc, ua, ub);
                const double t = newton_contact_t(ua, ub, wa, wb);
                if (a.out2 != nullptr) a.out2[eo + k] = !ok ? nan : (on ? newton_mul(mc, t) : 0.0);
                if (a.out3 != nullptr) a.out3[eo + k] = !ok ? nan : (on ? newton_mul(ln, t) : 0.0);
            }
        } else {
            for (int i = lane; i < n; i += T) {
                const int st = (int)dj[i];
                tv[i] = st == kNewtonFree ? sol[i] : 0.0;
                if constexpr (KIND >= 2) {
                    if (a.out2 != nullptr) a.out2[vo + i] = !ok ? nan : (st == kNewtonLo ? sol[i] : 0.0);
                    if (a.out3 != nullptr) a.out3[vo + i] = !ok ? nan : (st == kNewtonHi ? sol[i] : 0.0);
                }
            }
        }
        team_sync<T>();
        if (a.out1 != nullptr)
            for (int i = lane; i < n; i += T) a.out1[vo + i] = ok ? -tv[i] : nan;
        if (a.out0 != nullptr) {
            double* G = a.out0 + prob * (long)n * n;
            for (idx_t<T> idx = lane; idx < (idx_t<T>)n * n; idx += T)
                __builtin_nontemporal_store(ok ? newton_gP(tv[idx / n], xc[idx % n]) : nan, G + idx);
        }
    }
    team_sync<T>();   // the slice is the next problem's
}

template <int KIND, bool JVP, int T, bool LDS, bool REG>
__global__ __launch_bounds__(256) void newton_dense_kernel(const NewtonArgs a, int lds_per_team, long scratch_stride, const double reg)
{
    const int n = a.N;
    const long mat = (long)n * (n | 1);
    if constexpr (LDS) {
        extern __shared__ __attribute__((aligned(16))) double smem[];
        constexpr int TP = 64 / T; // teams per wave
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
        const int team = lane / T, tl = lane % T;
        double* sw = smem + (wave * TP + team) * lds_per_team;
        const long nteams = (long)gridDim.x * wpb * TP;
        // (a team past the end of the batch idles through the wave's fences: they are wave-wide, never team-wide)
        for (long w = ((long)blockIdx.x * wpb + wave) * TP + team; w < a.B; w += nteams)
            team_newton_problem<KIND, JVP, T, REG>(a, reg, w, sw, sw + mat, tl);
    } else {
        double* scr = a.scratch + (long)blockIdx.x * scratch_stride;
        for (long w = blockIdx.x; w < a.B; w += gridDim.x)
            team_newton_problem<KIND, JVP, T, REG>(a, reg, w, scr, scr + mat, (int)threadIdx.x);
    }
}

#if !DQQ_REG_UNIT
size_t newton_scratch_bytes(int N, long B) { return team_any_scratch_bytes(newton_slice_doubles(N), B); }
#endif

template <bool JVP>
static hipError_t launch_newton_mode(int kind, const NewtonArgs& a, double reg, bool any, hipStream_t s)
{
    // team_dense.h's launch on the polish's slice size, LDS teams and the any-N form's scratch alike
    return dispatch_kind(kind, [&](auto k) {
        return launch_team(a.N, a.B, any, newton_slice_doubles(a.N), a.scratch, true, s, [&](auto t, auto lds, auto go, int lds_per_team, long stride) {
            return go(newton_dense_kernel<decltype(k)::value, JVP, decltype(t)::value, decltype(lds)::value, kRegUnit>, a, lds_per_team, stride, reg);
        });
    });
}

#if DQQ_REG_UNIT
hipError_t launch_newton_dense_reg(int kind, bool jvp, const NewtonArgs& a, double reg, bool any, hipStream_t s)
{
#else
hipError_t launch_newton_dense(int kind, bool jvp, const NewtonArgs& a, bool any, hipStream_t s)
{
    const double reg = 0.0;
#endif
    return jvp ? launch_newton_mode<true>(kind, a, reg, any, s) : launch_newton_mode<false>(kind, a, reg, any, s);
}

} // namespace dqq
