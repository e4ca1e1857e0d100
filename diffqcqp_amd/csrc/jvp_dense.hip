// jvp_dense.hip -- dqq_jvp_f64 on a general P, the forward-mode form of dense.hip's backward team kernel: 64/T problems per
// wave, every matrix in the team's LDS slice (dense_core.h), the reference's operation order.  The duals, active sets and the
// matrix are the backward's (bwd_systems.h); the refinement receives the matrix transposed (At^T), the right-hand side
// s = R^T(tangents), and dx is read off the solution where the backward placed grad_x (bwd_systems.h: forward mode).
// A translation unit of its own: the backward's instantiations in dense.hip stay what they are.
#include "dense_core.h"
#include "launch.h"

namespace dqq {

// (dP x)_lane by row_dot on dP staged in M (row stride ld); 0 without a tangent of P.  Ends fenced: M may be overwritten.
template <int T>
static DQQ_D double jvp_dpx(const double* __restrict__ dP, long prob, int n, double* M, int ld, const double* vx, int lane)
{
#pragma clang fp contract(off)
    double r = 0.0;
    if (dP != nullptr) {
        load_matrix<T>(M, ld, dP + prob * (long)n * n, n, lane);
        DQQ_SYNC();
        if (lane < n) r = row_dot(M, ld, lane, vx, n);
        DQQ_SYNC();
    }
    return r;
}

// The doubles of a team's slice dense_jvp_problem touches -- three matrices; vx, vt; s, va, vb; then gamma, the multiplier rows
// of s and the int list, per kind as laid out below.  The slice is sized by the BACKWARD's dense_bwd_lds_doubles (one launch
// geometry for both modes): a change of either layout that breaks "the JVP fits the backward's slice" fails here, not on a GPU.
constexpr int dense_jvp_lds_doubles(int kind, int n)
{
    const int m = bwd_system_rows(kind, n);
    const int tail = kind == 0 ? 3 * n + (n + 1) / 2 : (kind == 1 ? 3 * n + (n / 2 + 1) / 2 : 5 * n + n);
    return 3 * m * (m | 1) + 2 * n + 3 * m + tail;
}
constexpr bool dense_jvp_fits_the_backwards_slice()
{
    for (int kind = 0; kind < 4; ++kind)
        for (int n = 1; n <= kDenseMaxRows; ++n)
            if (dense_jvp_lds_doubles(kind, n) > dense_bwd_lds_doubles(kind, n)) return false;
    return true;
}
static_assert(dense_jvp_fits_the_backwards_slice(), "dense_jvp_problem's LDS layout outgrew dense_bwd_lds_doubles");

// One problem by one team.  smem: dense_bwd_lds_doubles(KIND, n), laid out as the backward lays it out (vg holds the
// coordinate rows of s instead of grad_x).  a, b: l_n, mu (QCQP) / l_min, l_max (box kinds); da, db: their tangents.
template <int KIND, int T>
static DQQ_D void dense_jvp_problem(const double* __restrict__ P, const double* __restrict__ q, const double* __restrict__ a,
                                    const double* __restrict__ b, const double* __restrict__ v_sign,
                                    const double* __restrict__ x, const double* __restrict__ dP,
                                    const double* __restrict__ dq, const double* __restrict__ da,
                                    const double* __restrict__ db, double* __restrict__ dx, int* __restrict__ ir_steps,
                                    long prob, int n, double dual_eps, double* smem, int lane)
{
#pragma clang fp contract(off)
    const int nc = n / 2;
    const int mmax = bwd_system_rows(KIND, n);
    const int ld = mmax | 1;
    double* At = smem;               // mmax*ld
    double* K = At + mmax * ld;      // mmax*ld (holds P while the system is assembled)
    double* Kinv = K + mmax * ld;    // mmax*ld
    double* vx = Kinv + mmax * ld;   // n
    double* vt = vx + n;             // n: jvp_coord of every coordinate
    double* vdd = vt + n;            // mmax: s
    double* va = vdd + mmax;         // mmax
    double* vb = va + mmax;          // mmax
    double* vgam = vb + mmax;        // QP, QCQP: n; box kinds: 2n (lower | upper)
    const unsigned long long below = (1ull << lane) - 1ull;
    const double* Pg = P + prob * (long)n * n;
    double* Pl = K;
    const bool actn = lane < n;
    const double xi = actn ? x[prob * n + lane] : 0.0;
    const double qi = actn ? q[prob * n + lane] : 0.0;
    const double dqi = (actn && dq != nullptr) ? dq[prob * n + lane] : 0.0;
    if (actn) vx[lane] = xi;
    DQQ_SYNC();
    const double ti = jvp_coord(jvp_dpx<T>(dP, prob, n, At, ld, vx, lane), dqi);
    load_matrix<T>(Pl, ld, Pg, n, lane);
    if (actn) vt[lane] = ti;
    DQQ_SYNC();
    int steps = 0;

    if constexpr (KIND == 0) {
        int* perm = reinterpret_cast<int*>(vgam + 3 * n);
        const double gamma = actn ? qp_dual(row_dot(Pl, ld, lane, vx, n) + qi, xi, dual_eps) : 0.0;
        const bool is_act = actn && qp_active(gamma);
        const unsigned long long am = team_ballot<T>(is_act);
        const unsigned long long im = team_ballot<T>(actn && !is_act);
        const int na = __popcll(am), m = n;
        const int pos = is_act ? __popcll(am & below) : na + __popcll(im & below);
        if (actn) perm[pos] = lane;
        DQQ_SYNC();
        for (int idx = lane; idx < m * m; idx += T)
            At[(idx / m) * ld + idx % m] = qp_system_A(idx / m, idx % m, na, perm, vx, Pl, ld);
        if (actn) vdd[lane] = qp_jvp_s(lane, na, perm, vt);
        DQQ_SYNC();
        const double w = ir_wave<T>(At, K, Kinv, vdd, va, vb, m, ld, lane, steps);
        if (actn) dx[prob * n + perm[lane]] = jvp_dx_qp(lane, na, w);
        if (ir_steps != nullptr && lane == 0) ir_steps[prob] = steps;
    } else if constexpr (KIND == 1) {
        double* vS = vgam + n;           // nc
        double* vsm = vS + n;            // nc: multiplier rows of s, by active slot
        int* perm = reinterpret_cast<int*>(vsm + n);
        const double plq = actn ? row_dot(Pl, ld, lane, vx, n) + qi : 0.0;
        if (actn) va[lane] = plq;
        DQQ_SYNC();
        const bool actc = lane < nc;
        const double ln = actc ? a[prob * nc + lane] : 1.0, mc = actc ? b[prob * nc + lane] : 1.0;
        const double xa = actc ? vx[2 * lane] : 0.0, xb = actc ? vx[2 * lane + 1] : 0.0;
        const double pla = actc ? va[2 * lane] : 0.0, plb = actc ? va[2 * lane + 1] : 0.0;
        const QcqpDual ct = qcqp_contact(xa, xb, pla, plb, ln, mc, dual_eps);
        const double gamma = actc ? ct.gamma : 0.0;
        const bool is_act = actc && ct.act;
        const unsigned long long am = team_ballot<T>(is_act);
        const int na = __popcll(am), m = n + na;
        const int slot = __popcll(am & below);
        DQQ_SYNC();
        if (actc) { vgam[lane] = gamma; vS[lane] = ct.S; }
        if (is_act) {
            perm[slot] = lane;
            const double dln = da != nullptr ? da[prob * nc + lane] : 0.0, dmu = db != nullptr ? db[prob * nc + lane] : 0.0;
            vsm[slot] = qcqp_jvp_mult(QcqpContact::e2(gamma, ln, mc), dln, QcqpContact::e1(gamma, ln, mc), dmu);
        }
        DQQ_SYNC();
        for (int idx = lane; idx < m * m; idx += T)
            At[(idx / m) * ld + idx % m] = qcqp_system_A(idx / m, idx % m, na, perm, vS, vgam, vx, Pl, ld);
        if (lane < m) vdd[lane] = system_jvp_s(lane, na, vsm, vt);
        DQQ_SYNC();
        const double w = ir_wave<T>(At, K, Kinv, vdd, va, vb, m, ld, lane, steps);
        if (lane >= na && lane < m) dx[prob * n + (lane - na)] = w;
        if (ir_steps != nullptr && lane == 0) ir_steps[prob] = steps;
    } else {
        double* vsm = vgam + 2 * n;      // 2n: multiplier rows of s, by not_null position
        int* nnl = reinterpret_cast<int*>(vsm + 3 * n);
        double lo = actn ? a[prob * n + lane] : 0.0, hi = actn ? b[prob * n + lane] : 0.0;
        double dlo = (actn && da != nullptr) ? da[prob * n + lane] : 0.0, dhi = (actn && db != nullptr) ? db[prob * n + lane] : 0.0;
        if constexpr (KIND == 3) {
            const SBoxBounds eb = sbox_bounds(lo, hi, actn ? v_sign[prob * n + lane] : 0.0);
            lo = eb.lo; hi = eb.hi;
            dlo = eb.keep_lo ? dlo : 0.0;
            dhi = eb.keep_hi ? dhi : 0.0;
        }
        if (actn) { vgam[lane] = 0.0; vgam[n + lane] = 0.0; }
        const BoxNotNull bnn = box_not_null(xi, lo, hi, dual_eps);
        const bool aL = actn && bnn.aL, aU = actn && bnn.aU;
        const unsigned long long mL = team_ballot<T>(aL), mU = team_ballot<T>(aU);
        const int nn = __popcll(mL) + __popcll(mU);
        const int posL = __popcll(mL & below) + __popcll(mU & below);
        const int posU = posL + (aL ? 1 : 0);
        if (aL) nnl[posL] = lane;
        if (aU) nnl[posU] = n + lane;
        DQQ_SYNC();
        // the dual recovery is not part of the linear map: the backward's, unchanged
        const double rhs = actn ? box_dual_rhs(Pl + lane * ld, vx, n, qi) : 0.0;
        for (int idx = lane; idx < n * nn; idx += T) At[(idx / nn) * ld + idx % nn] = box_dual_At(idx / nn, idx % nn, nnl, n);
        if (actn) vdd[lane] = rhs;
        DQQ_SYNC();
        int steps_dual = 1;
        if (nn > 0) {
            const double gnn = ir_wave<T>(At, K, Kinv, vdd, va, vb, nn, ld, lane, steps_dual, n);
            if (lane < nn) vgam[nnl[lane]] = gnn;
        }
        DQQ_SYNC();
        if (aL) vsm[posL] = box_jvp_mult(lane, n, vgam, dlo, dhi);
        if (aU) vsm[posU] = box_jvp_mult(n + lane, n, vgam, dlo, dhi);
        const int m = nn + n;
        load_matrix<T>(Pl, ld, Pg, n, lane); // the refinement above used K as workspace
        DQQ_SYNC();
        for (int idx = lane; idx < m * m; idx += T)
            At[(idx / m) * ld + idx % m] = box_system_A(idx / m, idx % m, nn, nnl, vgam, Pl, ld, n);
        if (lane < m) vdd[lane] = system_jvp_s(lane, nn, vsm, vt);
        DQQ_SYNC();
        const double w = ir_wave<T>(At, K, Kinv, vdd, va, vb, m, ld, lane, steps);
        if (lane >= nn && lane < m) dx[prob * n + (lane - nn)] = w;
        if (ir_steps != nullptr && lane == 0) { ir_steps[2 * prob] = steps_dual; ir_steps[2 * prob + 1] = steps; }
    }
    DQQ_SYNC();
}

template <int KIND, int T>
__global__ __launch_bounds__(256) void jvp_dense_kernel(
    const double* __restrict__ P, const double* __restrict__ q, const double* __restrict__ a, const double* __restrict__ b,
    const double* __restrict__ v_sign, const double* __restrict__ x, const double* __restrict__ dP,
    const double* __restrict__ dq, const double* __restrict__ da, const double* __restrict__ db, double* __restrict__ dx,
    long B, int n, double dual_eps, int* __restrict__ ir_steps, int lds_per_team)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int TP = 64 / T; // teams per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int team = lane / T, tl = lane % T;
    double* sw = smem + (wave * TP + team) * lds_per_team;
    const long nteams = (long)gridDim.x * wpb * TP;
    // (a team past the end of the batch idles through the wave's fences: they are wave-wide, never team-wide)
    for (long w = ((long)blockIdx.x * wpb + wave) * TP + team; w < B; w += nteams)
        dense_jvp_problem<KIND, T>(P, q, a, b, v_sign, x, dP, dq, da, db, dx, ir_steps, w, n, dual_eps, sw, tl);
}

// the geometry of dense.hip: launch_bwd_team
template <int KIND, int T>
static hipError_t launch_jvp_team(const JvpArgs& a, hipStream_t s)
{
    constexpr int TP = 64 / T;
    const int lds_per_team = (dense_bwd_lds_doubles(KIND, a.N) + 1) & ~1;
    const size_t per_wave = sizeof(double) * (size_t)lds_per_team * TP;
    int wpb = (int)((64 * 1024) / per_wave);
    wpb = wpb > 4 ? 4 : (wpb < 1 ? 1 : wpb);
    const size_t lds_bytes = per_wave * wpb;
    const long per_block = (long)wpb * TP;
    const long need = (a.B + per_block - 1) / per_block;
    const long cap = 256L * 8;
    const unsigned grid = (unsigned)(need < cap ? (need > 0 ? need : 1) : cap);
    return launch_lds(jvp_dense_kernel<KIND, T>, dim3(grid), dim3(64 * wpb), lds_bytes, s, a.P, a.q, a.a, a.b, a.v, a.x, a.dP,
                      a.dq, a.da, a.db, a.dx, a.B, a.N, a.epsilon, a.ir_steps, lds_per_team);
}

template <int KIND>
static hipError_t launch_jvp_kind(const JvpArgs& a, hipStream_t s)
{
    const int rows = bwd_system_rows(KIND, a.N); // lanes a problem needs
    if (rows <= 8) return launch_jvp_team<KIND, 8>(a, s);
    if (rows <= 16) return launch_jvp_team<KIND, 16>(a, s);
    if (rows <= 32) return launch_jvp_team<KIND, 32>(a, s);
    return launch_jvp_team<KIND, 64>(a, s);
}

hipError_t launch_jvp_dense(int kind, const JvpArgs& a, hipStream_t s)
{
    switch (kind) {
    case kKindQP: return launch_jvp_kind<0>(a, s);
    case kKindQCQP: return launch_jvp_kind<1>(a, s);
    case kKindBox: return launch_jvp_kind<2>(a, s);
    case kKindSignedBox: return launch_jvp_kind<3>(a, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace dqq
