// bwd_diag.hip -- batched implicit-function backward, diagonal-P fast path.
//
// One launch replaces the Python batch loop + torch.bmm gradient assembly of
// the reference (QPFn2.backward qcqp.py:36-52, QCQPFn2.backward qcqp.py:156-181).
// It is a streaming kernel: per problem it reads P (N^2), q, x, grad_x (and
// l_n, mu) once and writes grad_P (N^2), grad_q (and grad_l_n, grad_mu) once.
//
// A wave64 owns a tile of T = 128/N consecutive problems; lane = (problem,
// coordinate pair / contact), i.e. N/2 lanes per problem, so q, x, grad_x,
// grad_q are read/written as one fully coalesced 1 KiB double2 access per wave
// and each QCQP contact (3x3 KKT block, kkt_core.h) lives in one lane.
//   phase A  stream the tile of P (N coalesced 1 KiB loads per wave), verify the
//            off-diagonals are exactly +-0, park the diagonal in LDS;
//   phase B  per-lane KKT blocks + the refinement loop of Solver.cpp:15-44; the
//            problem-wide residual norm is summed from LDS in the reference's
//            entry order, so the loop exit is bit-identical to a dense solve;
//   phase C  stream grad_P = -dl x^T back with the access pattern of phase A
//            (dl and x are picked out of LDS).
// Tiles with a non-zero off-diagonal: N <= 8 -> solved in place by the general per-problem routine
// (dense_core.h); larger N -> queued for the general dense kernel.
//
// Compile with -ffp-contract=off (see kkt_core.h).
#include "dense_core.h"
#include "launch.h"
#include "sbox_bounds.h"
#include "stream_tile.h"
#include "worklist.h"

namespace dqq {

// A problem that could not be queued for the general kernel (worklist.h, work-list hygiene: a header that did not start at
// zero): it will not be solved by this call -- its gradients say so.  Lane j of the problem's N/2 lanes.
template <int KIND, int N>
static DQQ_D void poison_problem_grads(double* __restrict__ grad_P, double* __restrict__ grad_q, double* __restrict__ g0,
                                       double* __restrict__ g1, double* __restrict__ gamma_out,
                                       double* __restrict__ dgamma_out, int* __restrict__ ir_steps, long prob, int j)
{
    const double nan = __builtin_nan("");
    // the optional diagnostics too (they come from torch.empty): NaN duals, -1 refinement steps
    if (KIND == 1) {
        if (gamma_out != nullptr) gamma_out[prob * (N / 2) + j] = nan;
        if (dgamma_out != nullptr) dgamma_out[prob * (N / 2) + j] = nan;
    } else if (KIND >= 2) {
        for (int c = 0; c < 4; ++c) {   // (B, 2N): this lane's two coordinates of both halves
            const long o = prob * (2 * N) + (c >> 1) * N + 2 * j + (c & 1);
            if (gamma_out != nullptr) gamma_out[o] = nan;
            if (dgamma_out != nullptr) dgamma_out[o] = nan;
        }
    }
    if (ir_steps != nullptr && j == 0) {
        if (KIND >= 2) { ir_steps[2 * prob] = -1; ir_steps[2 * prob + 1] = -1; }
        else ir_steps[prob] = -1;
    }
    if (grad_q != nullptr) { grad_q[prob * N + 2 * j] = nan; grad_q[prob * N + 2 * j + 1] = nan; }
    if (grad_P != nullptr)
        for (int c = 0; c < 2 * N; ++c) grad_P[prob * (long)(N * N) + 2 * j * N + c] = nan;   // this lane's two rows
    if (KIND == 1) {
        if (g0 != nullptr) g0[prob * (N / 2) + j] = nan;
        if (g1 != nullptr) g1[prob * (N / 2) + j] = nan;
    } else if (KIND >= 2) {
        if (g0 != nullptr) { g0[prob * N + 2 * j] = nan; g0[prob * N + 2 * j + 1] = nan; }
        if (g1 != nullptr) { g1[prob * N + 2 * j] = nan; g1[prob * N + 2 * j + 1] = nan; }
    }
}

template <int KIND, int N, int WPB, bool FUSE>
__global__ __launch_bounds__(64 * WPB, (FUSE ? (KIND == 0 ? 5 : (KIND == 1 ? 4 : 2)) : 1)) void bwd_diag_kernel(
    const double* __restrict__ P, const double* __restrict__ q, const double* __restrict__ l_n,
    const double* __restrict__ mu_c, const double* __restrict__ x, const double* __restrict__ grad_x,
    double* __restrict__ grad_P, double* __restrict__ grad_q, double* __restrict__ grad_l_n,
    double* __restrict__ grad_mu, double* __restrict__ gamma_out, double* __restrict__ dgamma_out, long B,
    double dual_eps, int layout, int* __restrict__ ir_steps, int* __restrict__ ws,
    const double* __restrict__ pdiag, const unsigned char* __restrict__ flags, const double* __restrict__ v_sign)
{
    constexpr int HL = N / 2;          // lanes per problem
    constexpr int T = 64 / HL;         // problems per wave tile (T*N == 128)
    constexpr int NC = N / 2;          // contacts per problem
    constexpr int RS = (KIND == 0) ? N : (KIND >= 2 ? 3 * N : N + NC); // residual entries per problem
    static_assert(N >= 2 && (N & (N - 1)) == 0 && N <= 128, "N must be a power of two");
    __shared__ __attribute__((aligned(16))) double s_pd[WPB][128], s_dl[WPB][128], s_x[WPB][128], s_rs[WPB][T * RS];
    // FUSE (small N, small batches): a non-diagonal tile is handled right here by the general routine.  The
    // launch bound keeps the register budget of this streaming kernel at 5 (QP) / 4 (QCQP) waves per SIMD:
    // uncapped, the general routine would take it from 58 to 134 VGPRs.
    __shared__ __attribute__((aligned(16))) double s_dense[WPB][FUSE ? dense_bwd_lds_doubles(KIND, N) : 1];

    // the wave index is wave-uniform: in an SGPR, the tile's position (`first`, `nvalid`, pointers) is scalar arithmetic and
    // costs no vector registers -- as a VGPR value the fused forward kept `first` and `nvalid` in SCRATCH (spilled and
    // reloaded in front of the stream of P, on the path every tile takes)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long tile = (long)blockIdx.x * WPB + wave;
    const long first = tile * T;
    if (first >= B) return; // whole wave leaves; no workgroup barrier is used below
    // this launch may fill the work-list: the words only its drain writes must be zero (worklist.h, work-list hygiene) -- loaded
    // here by the first wave, looked at below, once its tile of P has been streamed
    [[maybe_unused]] WorklistIdle idle{0, 0, 0, 0};
    const bool prepares = !FUSE && tile == 0 && ws != nullptr && layout == DQQ_P_AUTO;
    if constexpr (!FUSE) {
        if (prepares) idle = worklist_prepare_begin(ws, threadIdx.x & 63);
    }
    const int nvalid = (B - first) < T ? (int)(B - first) : T;
    const int pl = lane / HL, j = lane % HL;
    bool valid = pl < nvalid;   // (narrowed below to the problems this kernel solves itself)
    double *pd = s_pd[wave], *dlv = s_dl[wave], *xs = s_x[wave], *rs = s_rs[wave];
    const int limit = nvalid * N * N;

    // ---------------- phase A: P -> diagonal (LDS), off-diagonal zero check
    double2 pv;
    // The forward of these problems may have left their verified diagonal behind (pdiag, flags): a tile all
    // of whose problems are flagged diagonal skips the stream of P -- 512 of its 1280 bytes per problem at
    // N=8 -- and is handled exactly like the stream would have ended.
    // A tile all of whose problems the forward saw in non-diagonal tiles (flag 2) is queued without a look at P
    // (for N >= 32 the forward's tiles are this kernel's, so that is the decision the stream would reach; below, a
    // diagonal problem that lands in the general kernel this way gets the same bits: both follow the reference's order).
    // A tile with BOTH kinds, every problem classified (round 4, late: the fused forward of N <= 8 classifies problem by
    // problem): only the flag-2 problems are queued, the others take the fast path with the forward's diagonal -- a batch
    // with a few non-diagonal problems no longer sends 16 problems to the general kernel for each of them.  (The same bits
    // either way, see above.)
    bool have_diag = false, known_dense = false, by_problem = false;
    int f = -1;
    if (pdiag != nullptr && flags != nullptr && layout == DQQ_P_AUTO) {
        f = valid ? flags[first + pl] : -1;
        have_diag = __all(f == 1 || f == -1);
        known_dense = __all(f == 2 || f == -1);
        by_problem = !FUSE && !worklist_segmented(N) && !have_diag && !known_dense && __all(f == 1 || f == 2 || f == -1);
    }
    constexpr bool AGG = !FUSE && WPB > 1; // queue non-diagonal tiles with ONE atomic per workgroup (see worklist.h)
    __shared__ int s_cnt[2];
    // (capacity of the segmented work-list: one tile per wave, grid = ceil(tiles / WPB), <= 256 problems per workgroup)
    static_assert(!worklist_segmented(N) || T * WPB <= 256, "segmented work-list: at most 256 problems per workgroup");
    if (layout == DQQ_P_DIAG) {
        pv = valid ? *reinterpret_cast<const double2*>(P + first * N + 2 * lane) : make_double2(1.0, 1.0);
    } else {
        bool tile_dense = known_dense;
        if (known_dense) {
            pv = make_double2(1.0, 1.0);
        } else if (have_diag || by_problem) {
            pv = (valid && f == 1) ? *reinterpret_cast<const double2*>(pdiag + first * N + 2 * lane) : make_double2(1.0, 1.0);
        } else {
            const double* Pw = P + first * (long)(N * N);
            const unsigned nz = (nvalid == T) ? stream_tile_diag<N, N, false>(Pw, limit, pd, lane)
                                              : stream_tile_diag<N, N, true>(Pw, limit, pd, lane);
            tile_dense = __any(nz != 0); // wave-uniform
        }
        if constexpr (!FUSE) {
            if (prepares) worklist_prepare_end(ws, lane, idle);
        }
        if constexpr (FUSE) {
            if (tile_dense) {
                for (int jj = 0; jj < nvalid; ++jj)
                    dense_bwd_problem<KIND>(P, q, l_n, mu_c, x, grad_x, grad_P, grad_q, grad_l_n, grad_mu, gamma_out,
                                            dgamma_out, ir_steps, first + jj, N, dual_eps, s_dense[wave], lane);
                return;
            }
        } else if (layout == DQQ_P_AUTO) {
            if (by_problem) {
                const bool queued = f == 2 && j == 0;                          // one lane per queued problem
                const unsigned long long qm = __ballot(queued);
                const bool ok = worklist_push_entries<AGG, worklist_segmented(N)>(ws, B, __popcll(qm), queued,
                                                                                  __popcll(qm & ((1ull << lane) - 1)), (int)(first + pl), lane, s_cnt);
                if (lane == 0 && qm != 0) ws[kWsPerProblem] = 1;   // (report.h: how the drain's report is to be read)
                if (!ok && valid && f == 2) poison_problem_grads<KIND, N>(grad_P, grad_q, grad_l_n, grad_mu, gamma_out, dgamma_out, ir_steps, first + pl, j);
                valid = valid && f == 1;
            } else {
                const bool ok = worklist_push<AGG, worklist_segmented(N)>(ws, B, first, tile_dense ? nvalid : 0, lane, s_cnt);
                if (tile_dense) {
                    if (!ok && valid) poison_problem_grads<KIND, N>(grad_P, grad_q, grad_l_n, grad_mu, gamma_out, dgamma_out, ir_steps, first + pl, j);
                    return;
                }
            }
        }
        if (!have_diag && !by_problem) {
            wave_lds_fence();
            pv = valid ? *reinterpret_cast<const double2*>(pd + 2 * lane) : make_double2(1.0, 1.0);
        }
    }

    // ---------------- phase B: per-lane KKT blocks + iterative refinement
    const long co = first * N + 2 * lane;
    const double2 zero2 = make_double2(0.0, 0.0);
    const double2 qv = valid ? *reinterpret_cast<const double2*>(q + co) : zero2;
    const double2 xv = valid ? *reinterpret_cast<const double2*>(x + co) : zero2;
    const double2 gv = valid ? *reinterpret_cast<const double2*>(grad_x + co) : zero2;
    double dl0, dl1;
    int steps = 0;
    IrControl ctl;
    ctl.init();
    bool done = !valid;

    if (KIND == 0) {
        QpCoord c0, c1;
        c0.setup(pv.x, qv.x, xv.x, gv.x, dual_eps);
        c1.setup(pv.y, qv.y, xv.y, gv.y, dual_eps);
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
        dl0 = c0.dl();
        dl1 = c1.dl();
    } else if (KIND >= 2) {
        // box QP: l_n = l_min, mu_c = l_max (per coordinate); two refinement loops (dual recovery, then the
        // derivative system), each with its own problem-wide exit
        double2 lov = valid ? *reinterpret_cast<const double2*>(l_n + co) : zero2;
        double2 hiv = valid ? *reinterpret_cast<const double2*>(mu_c + co) : zero2;
        // signed box QP (KIND 3): the box QP on the effective bounds of sbox_bounds.h; v is (B,N,1) like l_min / l_max, one
        // more 16-byte load at the same even element offset
        [[maybe_unused]] bool klo0 = true, klo1 = true, khi0 = true, khi1 = true;
        if constexpr (KIND == 3) {
            const double2 vv = valid ? *reinterpret_cast<const double2*>(v_sign + co) : zero2;
            const SBoxBounds b0 = sbox_bounds(lov.x, hiv.x, vv.x), b1 = sbox_bounds(lov.y, hiv.y, vv.y);
            lov = make_double2(b0.lo, b1.lo);
            hiv = make_double2(b0.hi, b1.hi);
            klo0 = b0.keep_lo; klo1 = b1.keep_lo; khi0 = b0.keep_hi; khi1 = b1.keep_hi;
        }
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
        c0.setup_derivative(pv.x, gv.x);
        c1.setup_derivative(pv.y, gv.y);
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
        dl0 = c0.dl();
        dl1 = c1.dl();
        if (valid) {
            // BoxQPFn2.backward as intended (qcqp.py:91-93; signs: tests/test_oracle.py)
            if (grad_l_n != nullptr) {
                double2 g = make_double2(-(c0.dgamma_lo() * c0.gamma_lo), -(c1.dgamma_lo() * c1.gamma_lo));
                if constexpr (KIND == 3) g = make_double2(klo0 ? g.x : 0.0, klo1 ? g.y : 0.0);   // sbox_bounds.h
                *reinterpret_cast<double2*>(grad_l_n + co) = g;
            }
            if (grad_mu != nullptr) {
                double2 g = make_double2(c0.dgamma_hi() * c0.gamma_hi, c1.dgamma_hi() * c1.gamma_hi);
                if constexpr (KIND == 3) g = make_double2(khi0 ? g.x : 0.0, khi1 ? g.y : 0.0);
                *reinterpret_cast<double2*>(grad_mu + co) = g;
            }
            const long go = (first + pl) * 2 * N + 2 * j; // gamma / dgamma: (B, 2N) = [lower (N) | upper (N)]
            if (gamma_out != nullptr) {
                *reinterpret_cast<double2*>(gamma_out + go) = make_double2(c0.gamma_lo, c1.gamma_lo);
                *reinterpret_cast<double2*>(gamma_out + go + N) = make_double2(c0.gamma_hi, c1.gamma_hi);
            }
            if (dgamma_out != nullptr) {
                *reinterpret_cast<double2*>(dgamma_out + go) = make_double2(c0.dgamma_lo(), c1.dgamma_lo());
                *reinterpret_cast<double2*>(dgamma_out + go + N) = make_double2(c0.dgamma_hi(), c1.dgamma_hi());
            }
            if (ir_steps != nullptr && j == 0) ir_steps[2 * (first + pl)] = steps_dual;
        }
    } else {
        const long cc = first * NC + lane;
        const double ln = valid ? l_n[cc] : 1.0, mc = valid ? mu_c[cc] : 1.0;
        QcqpContact ct;
        ct.setup(pv.x, pv.y, qv.x, qv.y, xv.x, xv.y, gv.x, gv.y, ln, mc, dual_eps);
        for (int it = 0; it < kIrMaxIter; ++it) {
            if (!done) {
                double dsq[3];
                ct.step(dsq);
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
        dl0 = ct.dla();
        dl1 = ct.dlb();
        if (valid) {
            const double dg = ct.dgamma();
            if (grad_l_n != nullptr) grad_l_n[cc] = QcqpContact::e2(ct.gamma, ln, mc) * dg; // qcqp.py:178
            if (grad_mu != nullptr) grad_mu[cc] = QcqpContact::e1(ct.gamma, ln, mc) * dg;   // qcqp.py:180
            if (gamma_out != nullptr) gamma_out[cc] = ct.gamma;
            if (dgamma_out != nullptr) dgamma_out[cc] = dg;
        }
    }
    if (valid) {
        if (grad_q != nullptr) *reinterpret_cast<double2*>(grad_q + co) = make_double2(-dl0, -dl1); // qcqp.py:51/176
        if (ir_steps != nullptr && j == 0) ir_steps[KIND >= 2 ? 2 * (first + pl) + 1 : first + pl] = steps;
    }
    if (grad_P == nullptr) return;

    // ---------------- phase C: grad_P = -dl x^T  (qcqp.py:49 / :174)
    if (layout == DQQ_P_DIAG) {
        if (valid) *reinterpret_cast<double2*>(grad_P + co) = make_double2(-(dl0 * xv.x), -(dl1 * xv.y));
        return;
    }
    dlv[2 * lane] = dl0;
    dlv[2 * lane + 1] = dl1;
    xs[2 * lane] = xv.x;
    xs[2 * lane + 1] = xv.y;
    wave_lds_fence();
    double* Gw = grad_P + first * (long)(N * N);
#pragma unroll 4
    for (int k = 0; k < N; ++k) {
        const int f = k * 128 + 2 * lane;
        if (f < limit) {
            const int row = f / N, col = (row / N) * N + f % N;
            const double d = dlv[row];
            const double2 xx = *reinterpret_cast<const double2*>(xs + col);
            // grad_P is written once and not read again by this launch: non-temporal, keep it out of L2
            __builtin_nontemporal_store(-(d * xx.x), Gw + f);
            __builtin_nontemporal_store(-(d * xx.y), Gw + f + 1);
        }
    }
}

template <int KIND, int N, int WPB, bool FUSE>
static hipError_t launch_one(const BwdArgs& a, hipStream_t s)
{
    constexpr int T = 128 / N;
    const long ntiles = (a.B + T - 1) / T;
    const long nblocks = (ntiles + WPB - 1) / WPB;
    return launch((bwd_diag_kernel<KIND, N, WPB, FUSE>), dim3((unsigned)nblocks), dim3(64 * WPB), 0, s, a.P, a.q, a.l_n,
                       a.mu, a.x, a.grad_x, a.grad_P, a.grad_q, a.grad_l_n, a.grad_mu, a.gamma, a.dgamma, a.B, a.epsilon, a.layout,
                       a.ir_steps, a.ws, a.pdiag, a.flags, a.v);
}

// Shipped build: four waves per workgroup, non-diagonal tiles always queued (route.cpp bwd_fuses); the one-wave
// workgroups ("wpb" = 1) and the in-kernel general routine ("fuse_fallback" = 1) exist in the developer build only.
template <int KIND, int N>
static hipError_t launch_wpb(const BwdArgs& a, int wpb, bool fuse, hipStream_t s)
{
    if constexpr (kTuning) {
        if constexpr (bwd_diag_fuses(N) && KIND < 2) {
            if (fuse) return wpb == 1 ? launch_one<KIND, N, 1, true>(a, s) : launch_one<KIND, N, 4, true>(a, s);
        }
        if (wpb == 1) return launch_one<KIND, N, 1, false>(a, s);
    }
    return launch_one<KIND, N, 4, false>(a, s);
}


template <int KIND>
static hipError_t launch_kind(const BwdArgs& a, int wpb, bool fuse, hipStream_t s)
{
    switch (a.N) {
    case 2: return launch_wpb<KIND, 2>(a, wpb, fuse, s);
    case 4: return launch_wpb<KIND, 4>(a, wpb, fuse, s);
    case 8: return launch_wpb<KIND, 8>(a, wpb, fuse, s);
    case 16: return launch_wpb<KIND, 16>(a, wpb, fuse, s);
    case 32: return launch_wpb<KIND, 32>(a, wpb, fuse, s);
    case 64: return launch_wpb<KIND, 64>(a, wpb, fuse, s);
    default: return hipErrorInvalidValue;
    }
}

// fuse: the route plan's (route.cpp); waves per workgroup: 4 (1 behind the developer build's "wpb")
hipError_t launch_bwd_diag(int kind, const BwdArgs& a, bool fuse, hipStream_t s)
{
    const int wpb = knob_wpb() == 1 ? 1 : 4;
    if (kind == kKindBox) return launch_kind<2>(a, wpb, false, s);
    if (kind == kKindSignedBox) return launch_kind<3>(a, wpb, false, s);
    return kind == 0 ? launch_kind<0>(a, wpb, fuse, s) : launch_kind<1>(a, wpb, fuse, s);
}

} // namespace dqq
