/*
 * diffqcqp_hip.h -- C ABI of libdiffqcqp_hip.so: batched ADMM QP / QCQP solve
 * and implicit-function backward on MI355X (gfx950), float64.
 *
 * This is the drop-in boundary for the batched path of quentinll/diffqcqp.
 * The reference crosses Python -> C++ once PER PROBLEM through the pybind11
 * module `diffqcqp` (reference pybindings.cpp:74-83) from the batch loops of
 * qcqp.py:29-31, 45-47, 149-151, 167-172.  Each entry point below replaces one
 * of those loops (loop + per-problem call + the torch.bmm gradient assembly
 * that follows it) with one asynchronous launch over the whole batch.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into memory the caller owns (borrowed
 *     for the duration of the stream-ordered work); tensors are contiguous and
 *     batch-major exactly as torch lays them out:
 *         P (B,N,N)   q, x, grad_x, grad_q (B,N,1)   l_n, mu, grad_l_n, grad_mu (B,N/2,1)
 *         l_min, l_max, v, grad_l_min, grad_l_max (B,N,1)
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL =
 *     the default stream) and the call returns without synchronising;
 *   - return value: 0 on success, <0 for an invalid argument (DQQ_E_*), >0 a
 *     hipError_t from the launch (the launch's own status: the calling thread's
 *     sticky HIP error is neither consumed nor cleared).  Nothing throws.  The library
 *     keeps no state that a result or a route depends on: a call's results, bit for
 *     bit, and the kernels it launches are a function of its arguments alone (no
 *     history, thread-safe, any stream).  The one piece of process state is three
 *     diagnostic route counters (dqq_get_option: "lane_list_drains",
 *     "bwd_whole_batches", "fwd_feedback_routes"), bumped on the launch path.  What
 *     adapts to the data -- a steady stream of mostly non-diagonal N <= 8 batches
 *     through DQQ_P_AUTO is faster on other kernels of identical results -- is in the
 *     CALLER's hands: an optional report word the backward fills and hint flags the
 *     caller derives from it (dqq_hint_flags, below).  There are no tuning knobs
 *     (a developer build, -DDQQ_TUNING, has them: csrc/tuning.h);
 *   - like the reference (Solver.cpp:76, :100), numerical failure is not
 *     signalled by the solves: a non-PD P or L=0 yields NaNs in the output
 *     (dqq_check_f64, below, classifies a batch's solutions on the device);
 *   - `warm_start` does not appear in the per-kind entry points: the reference
 *     accepts it and overwrites it before reading it (Solver.cpp:70/80, 529/539).
 *     dqq_fwd_warm_f64, below, is the extension that does start from a caller's x0.
 *
 * p_layout
 *   DQQ_P_AUTO  (0)  P is (B,N,N).  Tiles whose off-diagonals are all exactly
 *                    zero run the diagonal fast path; every other tile is
 *                    solved by the general dense kernel.  Never assumes.
 *   DQQ_P_DENSE (1)  P is (B,N,N); always the general dense kernel.
 *   DQQ_P_DIAG  (2)  extension: P is the compact diagonal (B,N); grad_P (if
 *                    requested) is the compact diagonal of -dl x^T, (B,N).
 */
#ifndef DIFFQCQP_HIP_H
#define DIFFQCQP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQQ_P_AUTO 0
#define DQQ_P_DENSE 1
#define DQQ_P_DIAG 2
/* Per-call flag, ORed into p_layout: for 16 < N <= 64 the general (non-diagonal) path runs its kernels in the REFERENCE's
 * summation order (LDS wave kernels; QCQP backward beyond N = 42: a global-memory kernel that needs dqq_scratch_bytes of
 * scratch) instead of the register-resident kernels on the f64 matrix cores, which re-associate sums: forward x within
 * 1e-6 with the oracle's iteration counts on >= 99 % of the problems (all 1024 sampled of BASELINE configs[4]), gradients of the cond ~1e9 Tikhonov systems within 5e-7 (grad_P, grad_q) /
 * 8e-6 (grad_l_n, grad_mu) relative of the reference-order evaluation -- the evaluation-order noise of the reference's own
 * formulas.  10-30x slower; for parity studies.  No effect for N <= 16 or on diagonal tiles.  The forwards in the
 * reference's arithmetic (its rho / tau_dec, Cholesky with square roots) are the LDS kernel (odd N <= 16, and 16 < N <= 64
 * with this flag) and the workgroup kernel (N > 64); the lane-per-problem (N = 2, 4, 6, 8), group (DENSE N = 8) and team
 * (N = 10..16 even) forwards and the diagonal path multiply by 1/tau_dec and seed their reciprocals in hardware, with or
 * without this flag (what either keeps on ill-conditioned input). */
#define DQQ_F_REFERENCE_ORDER 0x100
/* Per-call HINT flags, ORed into p_layout (DQQ_P_AUTO, QP / QCQP, N <= 8; ignored elsewhere).  They select between kernels of
 * IDENTICAL results -- bit for bit, on any input -- so a wrong hint costs time and nothing else.  Obtain them from
 * dqq_hint_flags(); never pass them on a stream that is being captured into a graph that will be replayed on other data.
 *   DQQ_F_EXPECT_DENSE      most of the batch is non-diagonal.  Forward (N = 8): one lane per problem, the general solve with a
 *                           problem's whole matrix in its lane's registers, the tile of P staged through LDS and read once.
 *                           Backward (B >= 16384; N = 8: 24576): no classifying launch, the lane-per-problem kernel takes the
 *                           whole batch (and recounts for `report`).
 *   DQQ_F_EXPECT_LONG_LIST  backward: the work-list of non-diagonal problems will be long enough to fill the chip: the drain
 *                           launch is the lane-per-problem kernel (2x faster there; its 512-register waves need an empty SIMD
 *                           each, so it is never launched "just in case": behind a diagonal batch it would stall). */
#define DQQ_F_EXPECT_DENSE 0x200
#define DQQ_F_EXPECT_LONG_LIST 0x400
/* Per-call flag, ORed into p_layout: one-sided boxes for the Newton family (dqq_polish_f64, dqq_newton_bwd_f64,
 * dqq_newton_jvp_f64, dqq_newton_jac_f64), box QP and signed box QP (kinds 2 and 3).  With it l_min[i] may be finite or -inf
 * and l_max[i] finite or +inf, per coordinate, as the forwards accept them; l_min = +inf, l_max = -inf and a NaN bound stay
 * status 2, and every other entry (P, q, x, v, grad_x, the tangents dP, dq, da, db, the polish's first r) stays finite-only.
 * An infinite side is never active: its grad_l_min / grad_l_max is +0.0, its column of Ja / Jb is zero and its tangent takes
 * no part -- bit for bit what the unflagged call gives with a finite bound no iterate reaches in its place (no arithmetic
 * takes a bound as an operand: csrc/polish_core.h).  Without the flag nothing changes: an infinite bound is status 2.
 * Who knows the bit: the four entries above for kinds 1, 2 and 3 -- the QCQP accepts and ignores it, its radii stay
 * finite-only with or without it.  For the QP, which has no bounds, and for every other entry it is an unknown bit of
 * p_layout: DQQ_E_BAD_LAYOUT. */
#define DQQ_F_INFINITE_BOUNDS 0x800

#define DQQ_E_NULLPTR (-1)     /* a required pointer is NULL */
#define DQQ_E_BAD_SIZE (-2)    /* B < 0, N < 1, odd N for QCQP */
#define DQQ_E_UNSUPPORTED_N (-3) /* DQQ_P_DIAG only: N is not one of the fast-path sizes 2, 4, 8, 16, 32, 64 */
#define DQQ_E_BAD_LAYOUT (-4)
#define DQQ_E_WORKSPACE (-5)   /* workspace missing or too small */
#define DQQ_E_BAD_OPTION (-6)
#define DQQ_E_BAD_KIND (-7)    /* dqq_check_f64, dqq_fwd_warm_f64: kind is not 0 .. 3 */

/* Bytes of device workspace the calls below need for a batch of B problems
 * (fallback work-list of the AUTO layout).  The workspace must be zero-filled
 * ONCE when it is allocated; every call leaves its work-list empty again.  One
 * workspace must not be shared by calls that may run concurrently on different
 * streams. */
size_t dqq_workspace_bytes(int64_t B);

/* Work-list hygiene.  The kernels do not trust the work-list header (csrc/launch.h): a header that did not start at zero --
 * a workspace that was never initialised, memory written over by someone else, a launch chain cut short by an error -- is
 * REPAIRED by the next DQQ_P_AUTO call where that is possible (exit tickets and pick-up counters are re-zeroed by the fast
 * kernel; a stale or out-of-range count is clamped; an entry that is not a problem of the batch is replaced by problem 0,
 * which is then solved once more to the same values) and REPORTED where it is not (problems that cannot be queued get NaN
 * outputs, -1 in iters / ir_steps): nothing is read or written out of bounds and no problem is silently left unsolved.  A
 * sticky "dirty" word is set in the header whenever a COUNT or an ENTRY had to be clamped, replaced or dropped; stale exit
 * tickets and pick-up counters alone (idle words of the drain, re-zeroed before they are used) are repaired silently.
 *   dqq_workspace_reset   zero-fills the header on `stream` (asynchronous): the state a fresh workspace must be in.  The
 *                         recommended way to initialise one (a plain zero-fill of the first dqq_workspace_bytes(0) bytes is
 *                         equivalent).
 *   dqq_workspace_status  *dirty = 1 if any kernel has found the header inconsistent since the last reset.  SYNCHRONISES
 *                         `stream` (a 4-byte read-back): a diagnostic, never on a hot path, and not
 *                         allowed on a stream that is being captured (the synchronisation fails: a hipError_t is returned). */
int dqq_workspace_reset(void* workspace, size_t workspace_bytes, void* stream);
int dqq_workspace_status(const void* workspace, size_t workspace_bytes, void* stream, int* dirty);

/* The C ABI never allocates: every buffer, scratch included, is the caller's.  For sizes beyond the register / LDS
 * kernels of the general path (N > dqq_max_n(..), below) a workgroup-per-problem kernel works out of global memory and
 * needs this many bytes of scratch IN ADDITION to dqq_workspace_bytes(B), in the same `workspace` buffer (the work-list
 * first, the scratch behind it; no initialisation needed).  kind: 0 QP, 1 QCQP, 2 box QP, 3 signed box QP; pass: 0
 * forward, 1 backward; p_layout: as the call will pass it (only DQQ_F_REFERENCE_ORDER matters: QCQP backward 42 < N <= 64
 * needs scratch only with it).  A function of its arguments; 0 for every size the register / LDS kernels hold (all
 * BASELINE configs).  A call whose workspace is smaller than dqq_workspace_bytes(B) + dqq_scratch_bytes(..) returns
 * DQQ_E_WORKSPACE -- with DQQ_P_DENSE too, which otherwise needs no workspace at all.  Since nothing is allocated
 * or freed, a forward + backward pair can be captured into a HIP graph (tests/test_gpu_graph_capture.py). */
size_t dqq_scratch_bytes(int kind, int pass, int N, int64_t B, int p_layout);

/* There is no size limit (the reference has none, Solver.cpp:61): this returns the largest N the register / LDS
 * kernels of the general path hold -- kind 0 = QP forward/backward and the box forwards (64), 1 = QCQP forward (64),
 * 2 = QCQP backward (64; 42 with DQQ_F_REFERENCE_ORDER in p_layout), 3 = box QP backward (21).  Beyond it a
 * workgroup-per-problem kernel works out of global memory, in the reference's operation order, on the caller's scratch
 * (dqq_scratch_bytes). */
int dqq_max_n(int kind, int p_layout);

/* Replaces the loop qcqp.py:29-31 (QPFn2.forward -> diffqcqp.solveQP,
 * pybindings.cpp:17-22 -> Solver::solveQP, Solver.cpp:61-123).
 * iters (B ints, ADMM iterations executed per problem; -1 for a problem that could not be queued for the general kernel --
 * work-list hygiene above -- whose x is NaN) may be NULL.
 * pdiag_out (B,N doubles) / diag_flags_out (B bytes), both optional and DQQ_P_AUTO only: the forward leaves
 * the diagonal of every problem it verified to be diagonal (flag 1; flag 2: the problem sat in a tile with
 * non-zero off-diagonals; flag 0: not examined) for the backward of the SAME P, which then does not read P again
 * for tiles flagged 1 throughout (they take pdiag) or 2 throughout (they go to the general kernel); see
 * dqq_qp_bwd_f64. */
int dqq_qp_fwd_f64(const double* P, const double* q, double* x, int64_t B, int N, double eps, double mu_prox,
                   int max_iter, int adaptive_rho, int p_layout, int* iters, double* pdiag_out,
                   unsigned char* diag_flags_out, void* workspace, size_t workspace_bytes, void* stream);

/* Replaces the loop qcqp.py:45-47 + the assembly qcqp.py:48-51
 * (QPFn2.backward -> diffqcqp.solveDerivativesQP, pybindings.cpp:24-30 ->
 * Solver::dualFromPrimalQP / solveDerivativesQP, Solver.cpp:125-196):
 *   grad_P = -dl x^T (B,N,N), grad_q = -dl (B,N,1).  Either may be NULL
 * (ctx.needs_input_grad).  epsilon is the dual-recovery threshold of
 * solveDerivativesQP (pybindings.cpp:24, default 1e-10; qcqp.py never overrides
 * it).  ir_steps (B ints) may be NULL.  pdiag / diag_flags: optional, what the forward of the same
 * (unchanged) P stored; P itself must still be passed (non-flagged problems read it).
 * report: optional (NULL: none) -- the DEVICE address of one 8-byte word of pinned host memory the caller owns
 * (dqq_device_pointer); the launch that solves the batch's non-diagonal problems stores what it found there, for
 * dqq_hint_flags().  QP / QCQP, DQQ_P_AUTO, N <= 8; ignored otherwise. */
int dqq_qp_bwd_f64(const double* P, const double* q, const double* x, const double* grad_x, double* grad_P,
                   double* grad_q, int64_t B, int N, double epsilon, int p_layout, int* ir_steps,
                   const double* pdiag, const unsigned char* diag_flags, unsigned long long* report, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Replaces the loop qcqp.py:149-151 (QCQPFn2.forward -> diffqcqp.solveQCQP,
 * pybindings.cpp:54-60 -> Solver::solveQCQP, Solver.cpp:521-582).  l_n and mu
 * are the raw inputs; the radius l_n*mu is formed inside (pybindings.cpp:57). */
int dqq_qcqp_fwd_f64(const double* P, const double* q, const double* l_n, const double* mu, double* x,
                     int64_t B, int N, double eps, double mu_prox, int max_iter, int adaptive_rho,
                     int p_layout, int* iters, double* pdiag_out, unsigned char* diag_flags_out, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Replaces the loop qcqp.py:167-172 + the assembly qcqp.py:173-180
 * (QCQPFn2.backward -> diffqcqp.solveDerivativesQCQP, pybindings.cpp:62-71 ->
 * Solver.cpp:584-691):  grad_P = -dl x^T, grad_q = -dl, grad_l_n = E2 dgamma,
 * grad_mu = E1 dgamma.  Any output may be NULL.  gamma / dgamma (B,N/2,1, may be
 * NULL) expose the contact duals and their derivative terms, from which the
 * reference's per-problem return value (E1, E2, blgamma) can be rebuilt:
 * E1 = diag(2 gamma l_n^2 mu), E2 = diag(2 gamma l_n mu^2), blgamma = [dgamma; -grad_q].
 * epsilon: dual-recovery threshold (pybindings.cpp:62, default 1e-10).  report: as dqq_qp_bwd_f64. */
int dqq_qcqp_bwd_f64(const double* P, const double* q, const double* l_n, const double* mu, const double* x,
                     const double* grad_x, double* grad_P, double* grad_q, double* grad_l_n, double* grad_mu,
                     double* gamma, double* dgamma, int64_t B, int N, double epsilon, int p_layout,
                     int* ir_steps, const double* pdiag, const unsigned char* diag_flags, unsigned long long* report,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- the box-constrained members of the same solver family ------------------
 *
 * Replaces the loop qcqp.py:60-62 (BoxQPFn2.forward -> diffqcqp.solveBoxQP, pybindings.cpp:32-37 ->
 * Solver::solveBoxQP, Solver.cpp:198-261): min 1/2 x'Px + q'x, l_min <= x <= l_max.
 * l_min, l_max: (B,N,1).  Same loop as the QP with the projection of Solver.cpp:219-220. */
int dqq_boxqp_fwd_f64(const double* P, const double* q, const double* l_min, const double* l_max, double* x,
                      int64_t B, int N, double eps, double mu_prox, int max_iter, int adaptive_rho, int p_layout,
                      int* iters, double* pdiag_out, unsigned char* diag_flags_out, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Replaces the loop qcqp.py:103-105 (SignedBoxQPFn2.forward -> diffqcqp.solveSignedBoxQP,
 * pybindings.cpp:47-52 -> Solver::solveSignedBoxQP, Solver.cpp:374-439): the box QP with the extra
 * constraint sign(v_i) x_i <= 0 (projection of Solver.cpp:395-398).  v: (B,N,1), raw (its sign is taken
 * inside).  The reference has no backward for this problem (qcqp.py:111 "not implemented"); this library's is
 * dqq_signedboxqp_bwd_f64 below. */
int dqq_signedboxqp_fwd_f64(const double* P, const double* q, const double* l_min, const double* l_max,
                            const double* v, double* x, int64_t B, int N, double eps, double mu_prox,
                            int max_iter, int adaptive_rho, int p_layout, int* iters, double* pdiag_out,
                            unsigned char* diag_flags_out, void* workspace, size_t workspace_bytes, void* stream);

/* Replaces the loop + assembly of BoxQPFn2.backward (qcqp.py:67-94 -> diffqcqp.solveDerivativesBoxQP,
 * pybindings.cpp:39-45 -> Solver::dualFromPrimalBoxQP / solveDerivativesBoxQP, Solver.cpp:263-371).  The
 * shipped Python of that method does not run; the semantics here are the ones it
 * spells out, with the signs finite differences confirm (tests/test_oracle.py):
 *   grad_P = -dl x^T, grad_q = -dl, grad_l_min = -dgamma_lo o gamma_lo, grad_l_max = +dgamma_hi o gamma_hi.
 * Any output may be NULL.  gamma / dgamma (B,2N: lower multipliers | upper multipliers, may be NULL) are the
 * reference's per-problem return values: gamma, and blgamma[0:2N]; blgamma[2N:3N] = -grad_q.
 * ir_steps (B,2 ints, may be NULL): refinement steps of the dual recovery and of the derivative system.
 * General (non-diagonal) P: wave kernel up to dqq_max_n(3) = 21, global-memory workgroup kernel beyond. */
int dqq_boxqp_bwd_f64(const double* P, const double* q, const double* l_min, const double* l_max, const double* x,
                      const double* grad_x, double* grad_P, double* grad_q, double* grad_l_min, double* grad_l_max,
                      double* gamma, double* dgamma, int64_t B, int N, double epsilon, int p_layout, int* ir_steps,
                      const double* pdiag, const unsigned char* diag_flags, void* workspace, size_t workspace_bytes,
                      void* stream);

/* The signed box QP's backward -- the reference has none (qcqp.py:111 "not implemented"; its stub would differentiate the
 * plain box QP and ignore v).  Per coordinate, with s = sign(v), the forward's projection s min(s clamp(t, l_min, l_max), 0)
 * is, for l_min <= l_max, the clamp to the EFFECTIVE bounds
 *   s > 0: hi' = min(l_max, 0), lo' = min(l_min, hi');   s < 0: lo' = max(l_min, 0), hi' = max(l_max, lo');   s = 0
 * (v = +-0.0): lo' = hi' = 0
 * (csrc/sbox_bounds.h; min / max select, nothing is rounded), so the signed box QP is the box QP at (lo', hi') and
 * this call is dqq_boxqp_bwd_f64 at (P, q, lo', hi', x, grad_x), bit for bit on every route: the same active-set tests against
 * epsilon, the same two refinement loops, the same exits.  The bounds are transformed as they are loaded, inside the kernels.
 *   grad_P, grad_q, ir_steps (B,2): the box backward's.  gamma, dgamma (B,2N): the box backward's, as multipliers of the
 *   effective lower | upper bounds.
 *   grad_l_min = -dgamma_lo o gamma_lo where lo' == l_min (compared as values: -0.0 == +0.0), else +0.0;
 *   grad_l_max = +dgamma_hi o gamma_hi where hi' == l_max, else +0.0 -- where the sign constraint's 0 has replaced a bound,
 *   x does not depend on that bound.  A tie (l_min == 0 with s < 0, l_max == 0 with s > 0, a bound == 0 with s = 0) passes
 *   the gradient to the bound: a subgradient choice.  v gets no gradient (x is piecewise constant in it).
 * dqq_boxqp_bwd_f64's contract otherwise: every output may be NULL; v == NULL (B > 0) -> DQQ_E_NULLPTR; B = 0 returns 0 without
 * a launch; never allocates, never synchronises, may be captured into a HIP graph; pdiag / diag_flags: what
 * dqq_signedboxqp_fwd_f64 stored; DQQ_P_DIAG gives the compact grad_P (B,N).  Routes: the box QP backward's, dqq_max_n(3) = 21.
 * Scratch: N > 21 needs dqq_scratch_bytes(2, 1, N, B, p_layout) -- the BOX QP's query -- behind the work-list, DQQ_E_WORKSPACE
 * without it; dqq_scratch_bytes(3, 1, ...) is 0, as it was before this entry point existed. */
int dqq_signedboxqp_bwd_f64(const double* P, const double* q, const double* l_min, const double* l_max, const double* v,
                            const double* x, const double* grad_x, double* grad_P, double* grad_q, double* grad_l_min,
                            double* grad_l_max, double* gamma, double* dgamma, int64_t B, int N, double epsilon,
                            int p_layout, int* ir_steps, const double* pdiag, const unsigned char* diag_flags,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- how each solve ended -----------------------------------------------------------------------------------------------
 *
 * The solution check: given a batch's inputs and an x (from any route of the forwards above, or from anywhere else), ONE
 * streaming launch writes a status word and four residual scalars per problem.  Additive: no other entry point changes.
 * kind: 0 QP, 1 QCQP, 2 box QP, 3 signed box QP.  a, b, c are the kind's extra inputs, in the forwards' order: none (QP; pass
 * NULL), l_n, mu (QCQP), l_min, l_max (box), l_min, l_max, v (signed box).  p_layout: DQQ_P_DIAG reads P as the compact
 * diagonal (B,N), at any N; DQQ_P_DENSE and DQQ_P_AUTO read (B,N,N); DQQ_F_* flags are accepted and ignored.
 *
 * Definitions, all float64.  For problem i let g = P x + q and PI the Euclidean projection onto the kind's feasible set:
 * QP max(., 0); box clamp to [l_min, l_max]; signed box the same clamp, then sg min(sg t, 0) with sg = sign(v); QCQP per
 * contact the scaling onto the disc of radius l_n mu (tested on the squares, |t|^2 > r |r|, as the solver's prox_circle).
 *   resid (B,4):  [0] max |x - PI(x - g)|   the natural residual: zero exactly at a solution
 *                 [1] max |x - PI(x)|       the infeasibility
 *                 [2] 1/2 x'Px + q'x        the objective
 *                 [3] max(max_i (|P||x|)_i, max |q|)   the scale [0] is to be read against
 *   status (B ints), the first that applies:
 *                 2  an entry of x or of resid is not finite (a NaN anywhere in the inputs the sums touch ends here);
 *                 1  iters was given and iters[i] >= max_iter (the forward's iters output and its max_iter argument; an
 *                    iters[i] of -1 -- a problem that could not be queued -- has a NaN x: status 2);
 *                 0  otherwise.  max_iter is not looked at when iters is NULL.
 *   counts:       optional; 3 words on the device that THE CALLER ZEROED; counts[s] += problems of status s (one atomic per
 *                 wave and status present, not one per problem).
 * resid and status may each be NULL, not both.  The sums are taken in an order fixed by (N, layout) alone (csrc/check_core.h),
 * so the bits of resid do not depend on B, on the position in the batch or on the stream.  No workspace; never allocates, never
 * synchronises; may be captured into a HIP graph; B = 0 returns 0 without a launch.  Errors: DQQ_E_BAD_KIND, then those of the
 * forwards (DQQ_E_BAD_SIZE, DQQ_E_BAD_LAYOUT, DQQ_E_NULLPTR for a pointer the kind requires). */
int dqq_check_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                  const double* x, const int* iters, int max_iter, int64_t B, int N, int p_layout, double* resid,
                  int* status, unsigned long long* counts, void* stream);

/* Warm-started forward, every kind (an extension: the reference has no such entry, see the top of this file).
 *
 * kind, a, b, c: as dqq_check_f64 -- none (QP), l_n, mu (QCQP), l_min, l_max (box), l_min, l_max, v (signed box).  Everything
 * else is the kind's cold forward: the same route for the same (kind, N, B, p_layout | flags), the same loop, stopping rule,
 * workspace (dqq_workspace_bytes + dqq_scratch_bytes(kind, 0, ...)), iters / pdiag_out / diag_flags_out.  Only the state at
 * entry differs.  With x0 of shape (B,N,1) -- in every layout, DQQ_P_DIAG included --
 *     l_2 = l_2_pred = x0   (as given: NOT projected onto the feasible set)
 *     u      = -(P x0 + q)
 *     q_prox = q - mu_prox x0
 * and L, rho, tau_inc, tau_dec, rho_up, cpt as in the cold start.  In exact arithmetic the first x-update then returns x0
 * ((P + (rho + mu) I) x0 = rho x0 - u - q_prox) and the first projection is a projected-gradient step of length 1 / rho from
 * x0: a start at (or near) the solution stops after one (or a few) iterations.  Consequences:
 *   - max_iter = 0 returns x0 bit for bit (iters 0);
 *   - x0 = 0 is NOT the cold start: u = -q there, not 0;
 *   - a NaN or infinite entry of x0 gives a NaN x for that problem and for no other (dqq_check_f64: status 2); how many
 *     iterations such a problem is charged is not specified (the register kernels stop it after the first);
 *   - x0 must not overlap x: on a work-list that had to be repaired (csrc/worklist.h: a stale or foreign entry is replaced by
 *     problem 0) problem 0 can be solved twice, and the second solve must still find its start point, not the first one's result.
 * The per-kind entry points keep ignoring warm starts, bit for bit.  Never allocates, never synchronises; may be captured into
 * a HIP graph; B = 0 returns 0 without a launch.  Errors: DQQ_E_BAD_KIND, then the cold forward's (DQQ_E_BAD_SIZE,
 * DQQ_E_BAD_LAYOUT, DQQ_E_NULLPTR -- a NULL x0 with B > 0 included --, DQQ_E_UNSUPPORTED_N, DQQ_E_WORKSPACE). */
int dqq_fwd_warm_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                     const double* x0, double* x, int64_t B, int N, double eps, double mu_prox, int max_iter,
                     int adaptive_rho, int p_layout, int* iters, double* pdiag_out, unsigned char* diag_flags_out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Power-of-two equilibration, every kind (an extension: the reference solves P as it is handed over, and ADMM's iteration
 * count follows the scaling of P).  dqq_equilibrate_f64 writes the problem in the units x = D y, D = diag(2^e_i):
 *     P~ = D P D,  q~ = D q,  bounds D^-1 l,  start D^-1 x0          dqq_unscale_f64:  x = D y
 * with e_i = -round_half_even(log2(P_ii) / 2), from the exponent and mantissa of P_ii alone (csrc/equil_core.h has the exact
 * rule): P~_ii lies in [1/2, 2].  e_i = 0 where P_ii is <= 0, NaN or infinite; |e_i| <= 255.  Every factor is a power of two,
 * so every product is exact (but for results that are subnormal or overflow): the scaled problem is the caller's problem in
 * other units, y solves it exactly when D y solves the caller's, and the backward, the JVP, the Newton family and the solution
 * check run on the caller's (P, q, x) unchanged.  What changes is what the forward's eps is measured on: the scaled problem's
 * residuals.
 * kind, a, b, c: as dqq_check_f64.  Per kind: QCQP -- the two coordinates of a contact share the exponent of the larger of their
 * two diagonal entries (a disc stays a disc); a_out = 2^-e_c l_n, b_out = mu.  Box kinds -- a_out = D^-1 l_min, b_out = D^-1 l_max,
 * an infinite bound stays infinite; signed box: c_out = v (only its sign is used).  x0 (B,N,1): a warm start, optional.
 *   P_out (as P), q_out (B,N,1), e_out (B,N) int32: required.  a_out, b_out, c_out, x0_out: optional, each of its input's shape;
 *   an input whose output is NULL is not read (pass mu and v on to the forward as they are); an output whose input is NULL, or
 *   that the kind has no input for: DQQ_E_NULLPTR.
 *   No output may overlap any input (DQQ_E_BAD_LAYOUT).  dqq_unscale_f64: y, x_out (B,N,1), e (B,N) as e_out; x_out may be y
 *   itself (the operation is elementwise).
 * p_layout: DQQ_P_AUTO and DQQ_P_DENSE read and write (B,N,N), any N, each entry of P read once and written once; DQQ_P_DIAG
 * the compact diagonal (B,N) -- p~_i = 2^(2 e_i) p_i --, N in {2, 4, 8, 16, 32, 64} (DQQ_E_UNSUPPORTED_N otherwise).  DQQ_F_*
 * flags are accepted and ignored.  A diagonal P stays diagonal, a symmetric one symmetric: the scaled batch takes the route the
 * caller's would.  One launch each; no workspace; never allocates, never synchronises; may be captured into a HIP graph; B = 0
 * returns 0 without a launch.  Errors: DQQ_E_BAD_KIND, DQQ_E_BAD_SIZE, DQQ_E_BAD_LAYOUT (p_layout), then DQQ_E_NULLPTR,
 * DQQ_E_UNSUPPORTED_N, DQQ_E_BAD_LAYOUT (an overlap); dqq_unscale_f64: DQQ_E_BAD_SIZE, DQQ_E_NULLPTR.
 * Extra traffic of a scaled solve, bytes per problem: 16 N^2 (DQQ_P_DIAG: 16 N) for P, 20 N for q and e_out, 16 N per scaled
 * extra and for x0, 20 N for the unscale. */
int dqq_equilibrate_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                        const double* x0, int64_t B, int N, int p_layout, double* P_out, double* q_out, double* a_out,
                        double* b_out, double* c_out, double* x0_out, int32_t* e_out, void* stream);
int dqq_unscale_f64(const double* y, const int32_t* e, int64_t B, int N, double* x_out, void* stream);

/* Forward-mode derivative (JVP), every kind (an extension: the reference differentiates in reverse mode only).
 *
 * kind, a, b, c: as dqq_check_f64.  x: the solution (B,N,1).  dP, dq, da, db: the tangents of P, q and of the kind's first two
 * extras (l_n, mu / l_min, l_max), each of its input's shape; a NULL tangent is a zero tangent, da / db must be NULL for the
 * QP (DQQ_E_NULLPTR otherwise), v takes none.  dx (B,N,1), required: the directional derivative of x.
 *
 * Definition: the exact transpose of the kind's backward.  That call builds the matrix At and right-hand side rhs(g) of
 * csrc/bwd_systems.h from x, runs b = iterative_refinement(At, rhs(g)) (Solver.cpp:15-44) and assembles every gradient as a
 * linear map R(b).  This one forms s = R^T(tangents) -- the same placement, permutation and signs; dP enters as dP x, full and
 * not symmetrised, summed in index order --, runs w = iterative_refinement(At^T, s) with the same constants (mu_ir, the
 * epsilon-driven active sets, 10 steps at most, the exit after 1 or 3 bodies) and returns dx = rhs^T(w).  The box kinds' dual
 * recovery (their first refinement run) is not part of the linear map and runs unchanged; the signed box QP is the box QP at
 * the effective bounds, the bound tangents masked where dqq_signedboxqp_bwd_f64 masks the bound gradients.  Since both calls
 * return a Tikhonov iterate, <g, dx> and sum <grad, tangent> agree to the refinement's accuracy, not to the last bit.
 * ir_steps: as the kind's backward, (B) or, box kinds, (B,2); may be NULL.
 *
 * Routes: DQQ_P_DIAG -- P AND dP the compact diagonals (B,N), N in {2, 4, 8, 16, 32, 64}: the streaming kernel.  DQQ_P_DENSE
 * and DQQ_P_AUTO -- (B,N,N), never classified: the reference-order LDS kernel up to N = 64 (QP), 42 (QCQP), 21 (box kinds), the
 * global-memory kernel beyond, which needs the scratch dqq_scratch_bytes(kind == 3 ? 2 : kind, 1, N, B, p_layout |
 * DQQ_F_REFERENCE_ORDER) behind dqq_workspace_bytes(B) in `workspace` (DQQ_E_WORKSPACE without it; the work-list itself is not
 * touched, and no other route looks at `workspace`).  DQQ_F_* flags are accepted and ignored.
 * Never allocates, never synchronises; may be captured into a HIP graph; B = 0 returns 0 without a launch.  Errors:
 * DQQ_E_BAD_KIND, then the backward's (DQQ_E_BAD_SIZE, DQQ_E_BAD_LAYOUT, DQQ_E_UNSUPPORTED_N, DQQ_E_NULLPTR, DQQ_E_WORKSPACE). */
int dqq_jvp_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                const double* x, const double* dP, const double* dq, const double* da, const double* db, double* dx,
                int64_t B, int N, double epsilon, int p_layout, int* ir_steps, void* workspace, size_t workspace_bytes,
                void* stream);

/* Polish: a Newton finish that drives an approximate solution to machine-precision KKT (an extension: first-order QP solvers
 * usually ship one; the reference does not).
 *
 * kind, a, b, c: as dqq_check_f64.  x: an approximate solution (B,N,1), e.g. a forward's at a loose eps.  x_out (B,N,1),
 * required: may be x itself (in place), must not otherwise overlap x.  resid_out (B,2): the natural residual
 * r = max |x - PI(x - (P x + q))| before and after; steps_out (B): accepted steps; status (B): 0 at least one step accepted,
 * 1 x kept, 2 an entry of P, q, the kind's extras or x, or r, is not finite (x_out = x).  Each may be NULL.  An INFINITE
 * bound or radius is such an entry: a one-sided box (l_max = +inf), which the forwards accept, is never polished and says so
 * with status 2 -- pass DQQ_F_INFINITE_BOUNDS (above; box kinds: l_min = -inf and l_max = +inf are then ordinary input) or a
 * large finite bound instead.  A radius stays finite-only.
 *
 * Definition (csrc/polish_core.h has the order of evaluation): from x, up to max_steps times: F = x - PI(x - g), g = P x + q;
 * D the generalised Jacobian of PI at x - g (box-like kinds: 1 strictly inside the bounds, else 0; a QCQP contact: I_2 inside
 * the disc, (rad / |z|)(I_2 - z z' / |z|^2) outside it, 0 for rad <= 0); M = (I - D) + D P; M d = -F by Gaussian elimination
 * with partial pivoting; x+ = PI(x + d).  The step is kept only if it lowers r (strictly); the first step that does not, or
 * whose elimination meets a zero or non-finite pivot, ends the problem, as does r == 0.  So r after <= r before always, every
 * accepted x_out is a projected point, max_steps = 0 copies x, and an x_out that was not accepted is x bit for bit.  Polish is
 * a local method: from a rough x it may accept nothing.  A bad problem touches only its own rows.  l_n mu >= 0 is the contract
 * for the radii; a negative one leaves its own problem unspecified.  The signed box QP runs on its effective bounds.
 *
 * Routes: DQQ_P_DIAG -- P the compact diagonal (B,N), N in {2, 4, 8, 16, 32, 64}.  DQQ_P_DENSE and DQQ_P_AUTO -- (B,N,N), never
 * classified (a diagonal P gives DQQ_P_DIAG's bits): the matrix in LDS up to N = 64, beyond it a workgroup per problem on
 * `workspace`, which must hold dqq_polish_scratch_bytes(kind, N, B) bytes (0 up to N = 64; the scratch starts at `workspace`:
 * no work-list is involved, and dqq_scratch_bytes knows nothing of this entry).  DQQ_F_REFERENCE_ORDER and the hint flags are
 * accepted and ignored; DQQ_F_INFINITE_BOUNDS as described at its definition.
 * Never allocates, never synchronises; may be captured into a HIP graph; B = 0 returns 0 without a launch.  Errors:
 * DQQ_E_BAD_KIND, then dqq_check_f64's in its order (DQQ_E_BAD_SIZE, DQQ_E_BAD_LAYOUT, DQQ_E_NULLPTR), DQQ_E_UNSUPPORTED_N,
 * DQQ_E_WORKSPACE. */
size_t dqq_polish_scratch_bytes(int kind, int N, int64_t B);
int dqq_polish_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                   const double* x, double* x_out, int64_t B, int N, int max_steps, int p_layout, double* resid_out,
                   int* steps_out, int* status, void* workspace, size_t workspace_bytes, void* stream);
/* dqq_polish_f64 with a proximal weight: `reg` after p_layout, every other argument, route, scratch query, flag and error as
 * above.  reg >= 0 and finite; negative, NaN or infinite: DQQ_E_BAD_SIZE, after the kind, size and layout errors and before all
 * others, B = 0 included.  The step solves M_reg d = -F with M_reg = (I - D) + D (P + reg I): reg is added, one rounded add, to
 * the diagonal entries of P where M is formed and nowhere else -- g, z, F, r, D and the acceptance test (r+ < r on the true
 * residual) read the caller's P, so r after <= r before still holds.  For P positive semidefinite and reg > 0, M_reg is
 * nonsingular; on a fixed active set the iteration is a proximal-point method on the free block: it converges where a solution
 * exists, linearly, not quadratically.  reg = 0 (either sign) adds nothing and launches dqq_polish_f64's kernels: its bits.
 * dqq_polish_f64 is this entry with reg = 0. */
int dqq_polish_reg_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                       const double* x, double* x_out, int64_t B, int N, int max_steps, int p_layout, double reg,
                       double* resid_out, int* steps_out, int* status, void* workspace, size_t workspace_bytes, void* stream);
/* dqq_polish_reg_f64 with backtracking on the step length, so that the polish also works from outside the Newton basin (a cold
 * start x = PI(0) included): `max_halvings` after reg and `halvings` after status, every other argument, layout, route, scratch
 * query (dqq_polish_scratch_bytes), flag and error as above.  0 <= max_halvings <= 60, else DQQ_E_BAD_OPTION -- after the kind,
 * size and layout errors and reg's DQQ_E_BAD_SIZE, before all others, B = 0 included.  Per step, with d from M_reg d = -F: trial
 * points x_k = PI(x + 2^-k d), k = 0 .. max_halvings (the product and the sum rounded one by one); the first k whose residual is
 * below the current one is accepted (a NaN is not); if none is, x is kept and the problem is done.  The direction is solved for
 * once per step.  steps_out counts accepted steps, max_steps bounds them; status and resid_out mean what they mean above, and r
 * after <= r before still holds.  halvings (B) int32, optional (NULL): per problem the number of rejected trial points that
 * came before its accepted ones (those of a last step that accepts none are not counted).  max_halvings = 0 gives
 * dqq_polish_reg_f64's result bit for bit (from kernels of its own), and so does any max_halvings on a problem whose full
 * steps are all accepted.  The merit is the max-norm residual r: it cannot be lowered along d everywhere (DESIGN.md 4.16 has
 * the counts) -- a problem left with status 1 still wants ADMM. */
int dqq_polish_ls_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                      const double* x, double* x_out, int64_t B, int N, int max_steps, int p_layout, double reg, int max_halvings,
                      double* resid_out, int* steps_out, int* status, int32_t* halvings, void* workspace, size_t workspace_bytes,
                      void* stream);

/* Newton derivatives: the exact backward and JVP from the polish's Jacobian (an extension; opt-in -- the backward and JVP
 * entries above stay the reference's regularised, epsilon-thresholded and refined systems).
 *
 * kind, a, b, c, x: as dqq_polish_f64; x is used as given (meant to be a polished point, it does not have to be).
 * Definition (csrc/newton_core.h has the order of evaluation): at a solution F(x) = x - PI(x - (P x + q)) = 0; with z, D and
 * M = (I - D) + D P exactly the polish's at x, and E = dPI/dtheta at z (box-like kinds: 1 on the bound a coordinate that is not
 * free sits on, lower bound first; signed box: only where the effective bound is the caller's l_min / l_max, as
 * dqq_signedboxqp_bwd_f64 masks, v takes nothing; QCQP contact outside its disc with rad = l_n mu > 0: u = z / |z| towards rad,
 * d rad = mu dl_n + l_n dmu; else 0), implicit differentiation gives  M dx = -D (dP x + dq) + E dtheta.
 *   dqq_newton_jvp_f64: dx = M^-1 (-D (dP x + dq) + E dtheta).  dP (as P: (B,N,N), DQQ_P_DIAG (B,N)), dq, da, db: the tangents of P,
 *     q, a, b; each may be NULL (a zero tangent, bit for bit).  dx (B,N,1), required.
 *   dqq_newton_bwd_f64: M' w = grad_x, v = D w; grad_q = -v, grad_P = -v x' (DQQ_P_DIAG: the compact -v_i x_i), grad_a / grad_b
 *     = w where E is 1, +0.0 elsewhere (QCQP: t = u'w, grad_l_n = mu t, grad_mu = l_n t).  grad_x (B,N,1) required; every output
 *     may be NULL.  The signs are the backward entries' above.
 * For the QP, grad_a, grad_b, da and db must be NULL (DQQ_E_NULLPTR otherwise).  There is no epsilon and no ir_steps: one
 * Gaussian elimination with partial pivoting per problem (the polish's), no regularisation, no refinement; the two modes are
 * each other's transpose to rounding.  For P positive definite M is nonsingular.
 * status (B), optional: 0 done; 1 the elimination met a zero or non-finite pivot; 2 an entry of P, q, the extras, x, grad_x or
 * a given tangent is not finite (infinite bounds included, as the polish, unless DQQ_F_INFINITE_BOUNDS is given).  With 1 and 2 every requested output of that problem
 * is NaN; a bad problem touches only its own rows.
 *
 * Routes: dqq_polish_f64's -- DQQ_P_DIAG: N in {2, 4, 8, 16, 32, 64}; DQQ_P_DENSE and DQQ_P_AUTO, never classified (a diagonal
 * P gives DQQ_P_DIAG's bits): the matrix in LDS up to N = 64, beyond it a workgroup per problem on `workspace`, which must hold
 * dqq_newton_scratch_bytes(kind, N, B) bytes (0 up to N = 64; the scratch starts at `workspace`: no work-list is involved, and
 * dqq_scratch_bytes knows nothing of these entries).  Flags: as dqq_polish_f64.  Never allocates, never
 * synchronises; may be captured into a HIP graph; B = 0 returns 0 without a launch.  Errors: dqq_polish_f64's, in its order. */
size_t dqq_newton_scratch_bytes(int kind, int N, int64_t B);
int dqq_newton_bwd_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                       const double* x, const double* grad_x, double* grad_P, double* grad_q, double* grad_a, double* grad_b,
                       int64_t B, int N, int p_layout, int* status, void* workspace, size_t workspace_bytes, void* stream);
int dqq_newton_jvp_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                       const double* x, const double* dP, const double* dq, const double* da, const double* db, double* dx,
                       int64_t B, int N, int p_layout, int* status, void* workspace, size_t workspace_bytes, void* stream);
/* The Newton derivatives with a proximal weight: `reg` after p_layout, every other argument, route, scratch query, flag and
 * error as above; reg's own rule and error as dqq_polish_reg_f64's.  M_reg = (I - D) + D (P + reg I) replaces M in the one
 * elimination: backward M_reg' w = grad_x, v = D w; JVP M_reg dx = -D (dP x + dq) + E dtheta.  z, D, E, the right-hand sides and
 * grad_P = -v x' read the caller's P.  Both modes share M_reg and stay each other's transpose to rounding.  For P positive
 * semidefinite and reg > 0 M_reg is nonsingular, so status 1 does not occur there.  What it is: a solution x of the problem
 * also solves the problem with P + reg I and q - reg x; the entries return that problem's exact derivative with x held fixed in
 * q - reg x -- one proximal-point step's derivative.  For P positive definite it differs from the unregularised one by
 * O(reg |M^-1|); a tangent outside the range of a singular free block gives a finite dx of size |rhs| / reg.  No refinement is
 * done.  reg = 0 launches the parents' kernels: their bits.  The parents are these entries with reg = 0. */
int dqq_newton_bwd_reg_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                           const double* x, const double* grad_x, double* grad_P, double* grad_q, double* grad_a, double* grad_b,
                           int64_t B, int N, int p_layout, double reg, int* status, void* workspace, size_t workspace_bytes,
                           void* stream);
int dqq_newton_jvp_reg_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                           const double* x, const double* dP, const double* dq, const double* da, const double* db, double* dx,
                           int64_t B, int N, int p_layout, double reg, int* status, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- the Newton family on the central path: smoothed derivatives, kappa > 0 (an extension; opt-in) -----------------------
 *
 * dqq_polish_ls_f64, dqq_newton_bwd_reg_f64 and dqq_newton_jvp_reg_f64 with `double kappa` after reg: every other argument,
 * layout, route, scratch query (dqq_polish_scratch_bytes / dqq_newton_scratch_bytes) and error as the parent's.  The projection
 * PI of F(x) = x - PI(x - (P x + q)) is replaced by its Chen-Harker-Kanzow-Smale smoothing PI_k (csrc/smooth_core.h has the
 * formulas and the order of evaluation): with s(t) = sqrt(t^2 + 4 kappa^2), p(t) = (s + t) / 2 smooths max(t, 0), p' lies in
 * (0, 1); a box-like coordinate on [lo, hi] has PI_k = lo + p(z - lo) - p(z - hi), D = p'(z - lo) - p'(z - hi),
 * E_lo = 1 - p'(z - lo), E_hi = p'(z - hi) (the QP: PI_k = p(z), whose solution has x_i g_i = kappa^2 -- the log-barrier central
 * path); a QCQP contact with rad = l_n mu > 0 has PI_k = z rad / (rad + p(|z| - rad)).  D and E are the derivatives of PI_k, so an
 * inactive bound or radius gets a gradient that is not zero, a coordinate on its bound a grad_q that is not zero, and nothing
 * jumps at a kink.  M = (I - D) + D (P + reg I), the elimination, the status words, the damped step rule and both derivative modes
 * are the parents'; the smoothed polish drives r_k = max |x - PI_k(z)| down, its trial points stay PI(x + 2^-k d) with the hard
 * projection.  Differentiate at the point the smoothed polish returns, with the same kappa.
 * kappa: one scalar per call, finite and >= 0, else DQQ_E_BAD_OPTION -- where dqq_polish_ls_f64 refuses max_halvings: after the
 * kind, size and layout errors and reg's DQQ_E_BAD_SIZE, before all others, B = 0 included.  kappa = 0 launches the parents'
 * kernels: their bits.  kappa^2 must not underflow.
 * One-sided boxes under smoothing are out of scope: DQQ_F_INFINITE_BOUNDS is an unknown bit to these three entries, for every
 * kind (DQQ_E_BAD_LAYOUT), and an infinite bound is status 2.
 * On (B,N,N) M has no unit rows any more: the elimination is dense for every problem.  A diagonal P given as (B,N,N) still gives
 * DQQ_P_DIAG's bits (an entry of M is an exact zero wherever P's is). */
int dqq_polish_smooth_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                          const double* x, double* x_out, int64_t B, int N, int max_steps, int p_layout, double reg, double kappa,
                          int max_halvings, double* resid_out, int* steps_out, int* status, int32_t* halvings, void* workspace,
                          size_t workspace_bytes, void* stream);
int dqq_newton_bwd_smooth_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                              const double* x, const double* grad_x, double* grad_P, double* grad_q, double* grad_a,
                              double* grad_b, int64_t B, int N, int p_layout, double reg, double kappa, int* status,
                              void* workspace, size_t workspace_bytes, void* stream);
int dqq_newton_jvp_smooth_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                              const double* x, const double* dP, const double* dq, const double* da, const double* db, double* dx,
                              int64_t B, int N, int p_layout, double reg, double kappa, int* status, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- the polish path: kappa continuation in one launch, a cold-start Newton solve (an extension; opt-in) -----------------
 *
 * dqq_polish_path_f64 with stages (kappa_s, steps_s), s = 0 .. S-1, is bit for bit the chain of S calls of dqq_polish_smooth_f64:
 * call s has kappa = kappa_s and max_steps = steps_s, all calls share reg and max_halvings, and each call starts from the previous
 * call's x_out.  A stage with kappa_s == 0 is the hard damped polish (dqq_polish_ls_f64's functions, chosen by a run-time branch as
 * dqq_polish_smooth_f64 chooses them; the smoothed formulas at 0 are not the hard bits).  kappa_s need not be monotone.  What it is
 * for: the schedule 1e-1, 1e-2, 1e-3, 1e-4, 0 with budgets 4, 4, 4, 4, 60 from the cold start x = PI(0) solves problems the hard
 * damped polish alone leaves at status 1 -- a cold-start solver without ADMM -- in one launch: P is read once and x
 * stays on the chip between stages.  csrc/path_core.h is the definition on one thread.
 * kappas, stage_steps: HOST arrays of n_stages entries, read during the call and copied by value into the launch: the call stays
 * capturable into a HIP graph, and a replay uses the captured schedule.  1 <= n_stages <= 8; every kappa_s finite and >= 0; every
 * stage_steps[s] >= 0; max_halvings in 0 .. 60 -- else DQQ_E_BAD_OPTION, and DQQ_E_NULLPTR for a NULL kappas or stage_steps, where
 * dqq_polish_smooth_f64 refuses kappa: after the kind, size and layout errors and reg's DQQ_E_BAD_SIZE, before all others, B = 0
 * included.  Every other argument, layout, route, scratch query (dqq_polish_scratch_bytes) and error as dqq_polish_smooth_f64's;
 * DQQ_F_INFINITE_BOUNDS is an unknown bit (DQQ_E_BAD_LAYOUT) even when every kappa_s is 0.  The path's own kernels run whatever
 * the schedule is, a single stage included (which gives dqq_polish_smooth_f64's / dqq_polish_ls_f64's bits).
 * Outputs, each optional but x_out:
 *   x_out (B,N,1): the chain's last x_out; may be x.
 *   stage_resid_out (B,S,2), stage_steps_out (B,S): call s's resid_out and steps_out.
 *   resid_out (B,2): stage 0's r before and stage S-1's r after, each measured in its own stage's kappa.
 *   steps_out (B): accepted steps summed over the stages;  halvings (B): the stages' halvings summed.
 *   status (B): 2 if an input entry is not finite or stage 0's r before is not finite; else 0 if any stage accepted a step; else 1.
 * An input entry that is not finite leaves x_out = x, and every stage records what its call would.  A stage whose own r before is
 * not finite accepts nothing, as in the chain (stage 0 too: status stays 2 whatever the later stages do).  A bad problem touches
 * only its own rows.  Never allocates, never synchronises; B = 0 returns 0 without a launch. */
int dqq_polish_path_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                        const double* x, double* x_out, int64_t B, int N, int p_layout, double reg, const double* kappas,
                        const int* stage_steps, int n_stages, int max_halvings, double* resid_out, int* steps_out, int* status,
                        int32_t* halvings, double* stage_resid_out, int* stage_steps_out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- the Newton Jacobians: dx/dq, dx/da, dx/db from one elimination ---------------------------------------------------
 *
 * The sensitivity matrices of the solution map at x, per problem: column j of Jq (Ja, Jb) is dqq_newton_jvp_f64's dx for the
 * unit tangent dq = e_j (da = e_j, db = e_j) with every other tangent NULL, all columns carried through ONE elimination of
 * M = (I - D) + D P (csrc/newton_core.h: newton_jac_problem; the row operations depend on M only).  kind, a, b, c, x: as above.
 * Each of Jq, Ja, Jb may be NULL (not requested; all three NULL: DQQ_E_NULLPTR); for the QP Ja and Jb must be NULL
 * (DQQ_E_NULLPTR otherwise).  v of the signed box takes nothing.  A requested output has the same bits whatever else is
 * requested.
 *   DQQ_P_DENSE / DQQ_P_AUTO:  Jq (B,N,N) row-major, Jq[b,i,j] = dx_i/dq_j;  Ja, Jb (B,N,N) for the box kinds (l_min, l_max),
 *                              (B,N,N/2) for the QCQP (l_n, mu; through d rad = mu dl_n + l_n dmu).
 *   DQQ_P_DIAG (the Jacobians are block-diagonal; the outputs are compact):
 *                              Jq (B,N): dx_i/dq_i (QP, box kinds);  Jq (B,N,2) (QCQP): row i holds dx_i/dq_2k, dx_i/dq_2k+1,
 *                              k = i/2;  Ja, Jb (B,N): dx_i/da_i, dx_i/db_i (box kinds), dx_i/dl_n_k, dx_i/dmu_k (QCQP).
 * A diagonal P given as (B,N,N) yields DQQ_P_DIAG's bits on the diagonal blocks and zeros elsewhere.
 * dx/dP is not an output and is never materialised: d x_i / d P_jk = Jq[i,j] x_k  (DQQ_P_DIAG: d x_i / d p_j = Jq_ij x_j).
 * status (B), optional: 0 done; 1 the elimination met a zero or non-finite pivot; 2 an entry of P, q, the extras or x is not
 * finite (infinite bounds included, unless DQQ_F_INFINITE_BOUNDS is given).  With 1 and 2 every requested output of that problem is NaN; a bad problem touches only
 * its own rows.
 *
 * Routes, errors and their order: dqq_newton_jvp_f64's, on kernels of their own -- DQQ_P_DIAG: N in {2, 4, 8, 16, 32, 64};
 * DQQ_P_DENSE and DQQ_P_AUTO, never classified: the matrix and the block of right-hand sides in LDS up to N = 64, beyond it a
 * workgroup per problem on `workspace`, which must hold dqq_newton_jac_scratch_bytes(kind, N, B) bytes (0 up to N = 64; sized
 * for every column the kind has -- N, 2N or 3N -- whatever is requested, so that the size depends on (kind, N, B) alone).
 * Flags: as dqq_polish_f64.  Never allocates, never synchronises; may be captured into a HIP graph; B = 0
 * returns 0 without a launch. */
size_t dqq_newton_jac_scratch_bytes(int kind, int N, int64_t B);
int dqq_newton_jac_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                       const double* x, double* Jq, double* Ja, double* Jb, int64_t B, int N, int p_layout, int* status,
                       void* workspace, size_t workspace_bytes, void* stream);
/* dqq_newton_jac_f64 with a proximal weight: `reg` after p_layout, everything else as above; reg's rule and error as
 * dqq_polish_reg_f64's.  All columns ride through one elimination of M_reg, and column j has the bits of
 * dqq_newton_jvp_reg_f64's dx for the unit tangent e_j at the same reg.  reg = 0: dqq_newton_jac_f64's kernels and bits. */
int dqq_newton_jac_reg_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                           const double* x, double* Jq, double* Ja, double* Jb, int64_t B, int N, int p_layout, double reg,
                           int* status, void* workspace, size_t workspace_bytes, void* stream);
/* The Jacobians on the central path: dqq_newton_jac_reg_f64 with `double kappa` after reg; the layouts (dense, and compact
 * block-diagonal on DQQ_P_DIAG: smoothing keeps D in 1 x 1 / 2 x 2 blocks), the requests, status, the NaN fill, routes and the
 * scratch query (dqq_newton_jac_scratch_bytes) are the parent's.  Column j of Jq (Ja, Jb) has, bit for bit, the dx of
 * dqq_newton_jvp_smooth_f64 for the unit tangent dq = e_j (da = e_j, db = e_j) with every other tangent NULL at the same reg and
 * kappa; all requested columns ride through one elimination of the smoothed M = (I - D) + D (P + reg I)
 * (csrc/smooth_core.h: newton_jac_problem_smooth).  At kappa > 0 no column of Ja / Jb is a signed zero: an inactive bound or
 * radius has the relaxed-complementarity gradient.  d x_i / d P_jk = Jq[i,j] x_k still holds.  Differentiate at the point the
 * smoothed polish returns, with the same kappa.
 * kappa's rule, error (DQQ_E_BAD_OPTION) and its place in the order are dqq_newton_jvp_smooth_f64's; kappa = 0 launches
 * dqq_newton_jac_reg_f64's kernels: their bits.  DQQ_F_INFINITE_BOUNDS is an unknown bit for every kind (DQQ_E_BAD_LAYOUT) and
 * an infinite bound is status 2.  A diagonal P given as (B,N,N) still yields DQQ_P_DIAG's bits on the diagonal blocks and zeros
 * elsewhere.  Never allocates, never synchronises; may be captured into a HIP graph; B = 0 returns 0 without a launch. */
int dqq_newton_jac_smooth_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                              const double* x, double* Jq, double* Ja, double* Jb, int64_t B, int N, int p_layout, double reg,
                              double kappa, int* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the Newton family's active set, multipliers and kink margin ------------------------------------------------------
 *
 * The Newton derivatives above are exact while the active set stays put: which coordinates sit on which bound, which contacts
 * slide.  The solution map is piecewise smooth; at a kink they return one of the one-sided derivatives.  This entry reports,
 * per problem and from the cores' own comparisons (csrc/active_core.h has the order of evaluation), the active set the Newton
 * kernels use at x, the multipliers there, and how far the problem is from a kink.  kind, a, b, c, x: as dqq_polish_f64; x is
 * used as given.  An element is a coordinate (QP, box kinds) or a contact (QCQP); z = x - (P x + q) exactly as the polish
 * forms it.
 *   state  int32 (B,N), QCQP (B,N/2).  Coordinate: 0 free (the Newton kernels used D_ii = 1), 1 on the caller's lower bound,
 *          2 on the caller's upper bound, 3 on a constant (the QP's 0, the sign constraint's 0).  Contact, rad = l_n mu: 0 inside
 *          the disc (D = I), 1 outside with rad > 0 (sliding), 3 outside with rad <= 0 (D = 0).  grad_a / grad_b of
 *          dqq_newton_bwd_f64 is +0.0 wherever state is not 1 / 2.
 *   mult   double, as state: the multiplier in the normal-cone sense, one rounded operation -- +0.0 where free / inside;
 *          lo - z where z <= lo, z - hi where z >= hi (on the effective bounds); contact outside: |z| - rad if rad > 0, else |z|.
 *          At a solution this is |g_i| on an active coordinate, ||g_c|| on a sliding contact (g = P x + q).  The dual of the
 *          reference's squared-form contact constraint is gamma = mult / (2 rad).
 *   margin double (B), where int32 (B): the distance z can move, in the max norm per element, before `state` changes --
 *          coordinate min(|z - lo|, |z - hi|) (an infinite side: +inf), contact | |z| - rad | (rad <= 0: |z|) -- and the index
 *          of the first element, in index order, that attains the smallest (a coordinate, or a contact).  A fully unbounded
 *          box: +inf and 0.  With Jq of dqq_newton_jac_f64, dx = Jq dq and dz = dx - P dx - dq: max |dz_i| < margin implies
 *          that x + dx solves the problem at q + dq with the same state -- exactly for the QP and the box kinds, which are
 *          piecewise linear, to first order for the QCQP.
 *   status int32 (B): 0 done; 2 an entry of P, q, the extras or x is not finite (infinite bounds included, unless
 *          DQQ_F_INFINITE_BOUNDS is given), or a z_i is not.  There is no status 1: nothing is eliminated.  With 2 the
 *          problem's state and where are -1, its mult and margin NaN; a bad problem touches only its own rows.
 * Each output may be NULL (not requested; all five NULL: DQQ_E_NULLPTR).  A requested output has the same bits whatever else
 * is requested.
 *
 * Routes: DQQ_P_DIAG: N in {2, 4, 8, 16, 32, 64}; DQQ_P_DENSE and DQQ_P_AUTO, never classified (a diagonal P gives
 * DQQ_P_DIAG's bits): the matrix in LDS up to N = 64, beyond it a workgroup per problem.  No route needs scratch: there is no
 * workspace.  Flags: as dqq_polish_f64.  Never allocates, never synchronises; may be captured into a HIP graph; B = 0 returns
 * 0 without a launch.  Errors: dqq_polish_f64's, in its order, but DQQ_E_WORKSPACE. */
int dqq_newton_active_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                          const double* x, int* state, double* mult, double* margin, int* where, int* status, int64_t B, int N,
                          int p_layout, void* stream);

/* ---- adapting to the data without state in the library -------------------------------------------------------------
 *
 * Behind the diagonal fast path's backward, a second launch solves the problems whose P is not diagonal.  Two kernels can do
 * it -- a team of lanes per problem (best for up to a few thousand such problems) and a lane per problem (2x faster once they
 * fill the chip: 65536 dense 8x8 QCQP problems 110 -> ~55 us) -- and how many there are is known on the device only.  A
 * caller that presents the same kind of batch step after step (a training loop) can close that loop itself:
 *   1. keep one 8-byte word of pinned host memory per (kind, N) -- zero-initialised; per device, per stream or per module as
 *      it sees fit -- and pass its device address (dqq_device_pointer) as `report` to the backward calls;
 *   2. before a call of (kind, pass, N, B), read the word (a plain host load: nothing waits for the device) and OR
 *      dqq_hint_flags(kind, pass, N, B, word) into p_layout.
 * dqq_hint_flags is a pure function; the flags only ever select between kernels of identical results.  First calls, other
 * batch sizes, stream capture (pass no hints there): the argument-determined routes.  Measured, dense 8x8 QCQP, B = 65536,
 * forward + backward: DQQ_P_DENSE 0.131 ms; DQQ_P_AUTO with hints 0.134 ms (from the third step on), without 0.231 ms.
 * diffqcqp_amd/_capi.py does exactly this for the Python layer (one word per (device, kind, N); DQQ_FEEDBACK=0 turns it off).
 *
 * Word format (for the curious; callers only pass it through): bits 0..30 problems found, bit 31 "counted singly",
 * 32..61 B mod 2^30, 62..63 consecutive earlier reports of >= 3/4 B. */
int dqq_hint_flags(int kind, int pass, int N, int64_t B, unsigned long long last_report);

/* The device-side address of 8-byte-aligned pinned (hipHostMalloc / hipHostRegister / torch pin_memory()) host memory:
 * 0, DQQ_E_NULLPTR, DQQ_E_BAD_SIZE (misaligned) or the hipError_t of hipHostGetDevicePointer (not pinned memory). */
int dqq_device_pointer(void* pinned_host, void** device);

/* Route counters (diagnostics): how many launches the hint flags have sent down their alternative routes since the counter
 * was last reset.  Names: "lane_list_drains" (drain launches on the lane-per-problem backward), "bwd_whole_batches"
 * (DQQ_P_AUTO backwards solved whole by that kernel), "fwd_feedback_routes" (N = 8 forwards on one lane per problem).
 * dqq_set_option(name, v) stores v (0 resets); any other name -> DQQ_E_BAD_OPTION.  These are the only names this library
 * knows and none of them changes what a call does.  (A developer build, -DDQQ_TUNING, also accepts the kernel-selection knobs
 * of csrc/tuning.h; they change time, never results.) */
int dqq_set_option(const char* name, int value);
int dqq_get_option(const char* name, int* value);

/* "diffqcqp_hip <version> gfx950" */
const char* dqq_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DIFFQCQP_HIP_H */
