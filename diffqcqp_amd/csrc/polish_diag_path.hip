// polish_diag_path.hip -- dqq_polish_path_f64 with DQQ_P_DIAG: the polish path (path_core.h: polish_problem_path -- the chain of
// smoothed damped polishes over a schedule of (kappa_s, steps_s), bit for bit) in one launch on the compact diagonal (B,N).
// polish_diag_smooth.hip's / polish_diag_ls.hip's tile, trial loop and launch geometry: a wave64 owns 128/N consecutive problems,
// lane = (problem, coordinate pair / contact), every vector one 16-byte access per lane, the lane's block of M solved in
// registers with polish_solve1 / polish_solve2, the problem's r taken by every one of its lanes from the wave's LDS slice in index
// order, a failed block found by a ballot.
//
// The inputs are loaded and classified once and x stays in registers from stage to stage.  The stage loop is the outer loop and
// its index, kappa_s and steps_s are kernel-uniform, so the branch between the two evaluators -- kappa_s == 0: polish_diag_ls.hip's
// hard F and, where the block is formed, the hard Jacobian of the kept z; kappa_s > 0: polish_diag_smooth.hip's F_k and D kept
// next to z -- is uniform over the wave.  What diverges is per lane, as in the parents: a problem that has used its stage's
// budget, reached r == 0, failed or found no step idles, masked, through the rest of the stage's steps while its tile neighbours
// go on, and enters the next stage with them by evaluating its own r there; a problem whose inputs are bad, or a tile slot past
// the end of the batch, idles through every stage.  A stage ends for the wave when none of its problems is live (or at the
// budget).  Ballots and fences are wave-wide and are reached by every lane of the wave in every trip: no lane leaves a loop
// that its neighbours still run.  Nothing here waits for another wave.
#include "diag_tile.h"
#include "path_core.h"

namespace dqq {

template <int KIND, int N, int WPB>
__global__ __launch_bounds__(64 * WPB) void polish_diag_path_kernel(const PolishArgs a, const PolishPathOpts o)
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
    const unsigned long long mine = diag_lane_mask<HL>(pl);   // the lanes of this problem
    const int S = o.n_stages;

    const long co = first * N + 2 * lane;
    const double2 zero2 = make_double2(0.0, 0.0);
    const double2 pv = valid ? *reinterpret_cast<const double2*>(a.P + co) : make_double2(1.0, 1.0);
    const double2 qv = valid ? *reinterpret_cast<const double2*>(a.q + co) : zero2;
    const double2 xv = valid ? *reinterpret_cast<const double2*>(a.x + co) : zero2;
    bool bad = !fin2(pv) || !fin2(qv) || !fin2(xv);
    double rad = 0.0;
    double2 av = zero2, bv = zero2, cv = zero2;
    if constexpr (KIND == 1) {
        const long cc = first * HL + lane;   // (B,N/2): element by element
        const double ln = valid ? a.a[cc] : 1.0, mc = valid ? a.b[cc] : 1.0;
        bad = bad || !__builtin_isfinite(ln) || !__builtin_isfinite(mc);
        rad = ln * mc;
    }
    if constexpr (KIND >= 2) {
        av = valid ? *reinterpret_cast<const double2*>(a.a + co) : zero2;
        bv = valid ? *reinterpret_cast<const double2*>(a.b + co) : zero2;
        bad = bad || !fin2(av) || !fin2(bv);   // one-sided boxes are not admitted by this entry
    }
    if constexpr (KIND == 3) {
        cv = valid ? *reinterpret_cast<const double2*>(a.c + co) : zero2;
        bad = bad || !fin2(cv);
    }
    double lo0 = 0.0, hi0 = 0.0, lo1 = 0.0, hi1 = 0.0;
    if constexpr (KIND != 1) {
        polish_bounds<KIND>(av.x, bv.x, cv.x, lo0, hi0);
        polish_bounds<KIND>(av.y, bv.y, cv.y, lo1, hi1);
    }
    bad = (__ballot(bad) & mine) != 0ull;
    // the diagonal of P' for the blocks of M; z and F below read pv
    const double pm0 = polish_reg(pv.x, o.reg), pm1 = polish_reg(pv.y, o.reg);

    // z and F (hard: F; else F_k and the Jacobian of PI_k -- box-like: D of the two coordinates in D[0], D[1]; a contact: d00,
    // d01, d11) at (x0, x1).  hard leaves D alone: the hard Jacobian is taken from z where the block is formed.
    auto eval = [&](bool hard, double kappa, double x0, double x1, double& z0, double& z1, double& F0, double& F1, double (&D)[3]) {
        z0 = polish_z(x0, polish_acc(0.0, pv.x, x0), qv.x);
        z1 = polish_z(x1, polish_acc(0.0, pv.y, x1), qv.y);
        if (hard) {
            if constexpr (KIND == 1) {
                polish_F_contact(x0, x1, z0, z1, rad, F0, F1);
            } else {
                F0 = polish_F<KIND>(x0, z0, lo0, hi0);
                F1 = polish_F<KIND>(x1, z1, lo1, hi1);
            }
        } else {
            if constexpr (KIND == 1) {
                const SmoothDisc s = smooth_disc(z0, z1, rad, kappa);
                F0 = smooth_F(x0, s.pa);
                F1 = smooth_F(x1, s.pb);
                D[0] = s.D[0]; D[1] = s.D[1]; D[2] = s.D[2];
            } else {
                const SmoothBox s0 = smooth_box<KIND>(z0, lo0, hi0, kappa), s1 = smooth_box<KIND>(z1, lo1, hi1, kappa);
                F0 = smooth_F(x0, s0.pi);
                F1 = smooth_F(x1, s1.pi);
                D[0] = s0.D; D[1] = s1.D; D[2] = 0.0;
            }
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

    double x0 = xv.x, x1 = xv.y, z0 = 0.0, z1 = 0.0, F0 = 0.0, F1 = 0.0, D[3] = {0.0, 0.0, 0.0};
    double r_first = 0.0, r = 0.0;
    int status0 = 1, steps_total = 0, halvings_total = 0;
    for (int s = 0; s < S; ++s) {   // kernel-uniform
        const double kappa = o.kappa[s];
        const bool hard = kappa == 0.0;
        const int budget = o.budget[s];
        // the stage opens as the call it stands for does: its own r at the current point
        eval(hard, kappa, x0, x1, z0, z1, F0, F1, D);
        const double r0 = residual(F0, F1, valid);
        r = r0;
        int steps = 0, halvings = 0;
        bool live = valid && !bad && __builtin_isfinite(r0);
        for (int it = 0; it < budget; ++it) {
            live = live && r != 0.0;
            if (__all(!live)) break;
            // the direction of the lane's block, once per step
            double d0 = -F0, d1 = -F1;
            bool ok = true;
            if (live) {
                if (hard) {
                    if constexpr (KIND == 1) {
                        double H[3];
                        polish_disc_jacobian(z0, z1, rad, H);
                        ok = polish_solve2(polish_contact_entry(true, H[0], H[0], H[1], pm0, 0.0),
                                           polish_contact_entry(false, H[1], H[0], H[1], 0.0, pm1),
                                           polish_contact_entry(false, H[1], H[1], H[2], pm0, 0.0),
                                           polish_contact_entry(true, H[2], H[1], H[2], 0.0, pm1), d0, d1);
                    } else {
                        ok = polish_solve1(polish_free(z0, lo0, hi0) ? pm0 : 1.0, d0);
                        ok = polish_solve1(polish_free(z1, lo1, hi1) ? pm1 : 1.0, d1) && ok;
                    }
                } else {
                    if constexpr (KIND == 1) {
                        double m[4];
                        newton_contact_block(D, pm0, pm1, m);
                        ok = polish_solve2(m[0], m[1], m[2], m[3], d0, d1);
                    } else {
                        ok = polish_solve1(smooth_box_entry(true, D[0], pm0), d0);
                        ok = polish_solve1(smooth_box_entry(true, D[1], pm1), d1) && ok;
                    }
                }
            }
            const bool failed = (__ballot(live && !ok) & mine) != 0ull;   // a failed block fails the problem's step
            bool search = live && !failed;
            double t = 1.0;
            for (int k = 0; k <= o.max_halvings; ++k, t = polish_half(t)) {
                if (__all(!search)) break;
                double xn0 = 0.0, xn1 = 0.0, zn0 = 0.0, zn1 = 0.0, Fn0 = 0.0, Fn1 = 0.0, Dn[3] = {0.0, 0.0, 0.0};
                if (search) {
                    xn0 = polish_trial(x0, t, d0);
                    xn1 = polish_trial(x1, t, d1);
                    if constexpr (KIND == 1) {
                        check_proj_circle(xn0, xn1, rad);
                    } else {
                        xn0 = polish_proj<KIND>(xn0, lo0, hi0);
                        xn1 = polish_proj<KIND>(xn1, lo1, hi1);
                    }
                    eval(hard, kappa, xn0, xn1, zn0, zn1, Fn0, Fn1, Dn);
                }
                const double rn = residual(Fn0, Fn1, search);
                if (search && rn < r) {   // accepted at this k: the problem idles through its neighbours' further trials
                    x0 = xn0; x1 = xn1; z0 = zn0; z1 = zn1; F0 = Fn0; F1 = Fn1;
                    D[0] = Dn[0]; D[1] = Dn[1]; D[2] = Dn[2];
                    r = rn;
                    ++steps;
                    halvings += k;
                    search = false;
                }
            }
            // a failed elimination, or no trial point accepted (`search` still set): the problem keeps x and stops this stage
            if (failed || search) live = false;
        }
        if (s == 0) { r_first = r0; status0 = polish_status(bad, r0, steps); }
        steps_total += steps;
        halvings_total += halvings;
        if (valid && j == 0) {
            const long e = (first + pl) * S + s;
            if (o.stage_resid != nullptr) { o.stage_resid[2 * e] = r0; o.stage_resid[2 * e + 1] = r; }
            if (o.stage_steps != nullptr) o.stage_steps[e] = steps;
        }
    }
    if (valid) {
        *reinterpret_cast<double2*>(a.x_out + co) = make_double2(x0, x1);
        if (j == 0) {
            const long b = first + pl;
            if (a.resid != nullptr) { a.resid[2 * b] = r_first; a.resid[2 * b + 1] = r; }
            if (a.steps != nullptr) a.steps[b] = steps_total;
            if (a.status != nullptr) a.status[b] = path_status(status0, steps_total);
            if (o.halvings != nullptr) o.halvings[b] = halvings_total;
        }
    }
}

template <int KIND, int N>
static hipError_t launch_one(const PolishArgs& a, const PolishPathOpts& o, hipStream_t s)
{
    constexpr int WPB = kDiagWPB;
    return launch((polish_diag_path_kernel<KIND, N, WPB>), dim3(diag_tile_grid<N, WPB>(a.B)), dim3(64 * WPB), 0, s, a, o);
}

template <int KIND>
static hipError_t launch_kind(const PolishArgs& a, const PolishPathOpts& o, hipStream_t s)
{
    return dispatch_diag_n(a.N, [&](auto n) { return launch_one<KIND, decltype(n)::value>(a, o, s); });
}

hipError_t launch_polish_diag_path(int kind, const PolishArgs& a, const PolishPathOpts& o, hipStream_t s)
{
    return dispatch_kind(kind, [&](auto k) { return launch_kind<decltype(k)::value>(a, o, s); });
}

} // namespace dqq
