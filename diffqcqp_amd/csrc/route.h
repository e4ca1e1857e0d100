// route.h -- which kernels a call launches: a pure function of (kind, pass, N, B, p_layout | flags) and, in the developer
// build, the knobs of tuning.h.  Plain C++ (no HIP): capi.hip executes the plan, the CPU tests (tests/test_routes.py) check
// it, and dqq_scratch_bytes / dqq_max_n / dqq_hint_flags answer from the same rules.  DESIGN.md section 3 is the table.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/diffqcqp_hip.h"

namespace dqq {

// kind: 0 QP, 1 QCQP, 2 box QP, 3 signed box QP (its backward: the box QP's routes, dqq_signedboxqp_bwd_f64)
constexpr int kKindQP = 0, kKindQCQP = 1, kKindBox = 2, kKindSignedBox = 3;

// Which N can solve their non-diagonal tiles inside the fast kernel (no fallback launch: an empty
// work-list launch still costs ~4.6 us behind a 13-35 us kernel).  Whether they do is the plan's choice.
constexpr bool fwd_diag_fuses(int N) { return N <= 16; }
constexpr bool bwd_diag_fuses(int N) { return N <= 8; }

enum class Family : unsigned char {
    None,
    FwdDiag,   // fwd_diag.hip           diagonal fast path (lpp, fuse)
    FwdLane,   // fwd_lane_dense.hip     a lane per problem, N = 2, 4, 6, 8
    FwdSmall,  // fwd_small.hip          a team per problem, N = 10 .. 16 even
    FwdWave64, // dense_wave64.hip       a wave per problem, f64 MFMA, 16 < N <= 64
    FwdLds,    // dense.hip              LDS wave kernel, reference summation order
    FwdAny,    // general_any.hip        global memory, caller's scratch
    BwdDiag,   // bwd_diag.hip           diagonal fast path (fuse)
    BwdLane,   // bwd_lane_dense.hip     a lane per problem (lane_mode)
    BwdSmall,  // bwd_small.hip          a team per problem, even N <= 16
    BwdChol,   // dense_wave64.hip       QP, 16 < N <= 64, block Cholesky on MFMA
    BwdQcqp,   // bwd_wave_qcqp.hip      QCQP, 16 < N <= 32
    BwdQcqpBig,// bwd_wave_qcqp_big.hip  QCQP, 32 < N <= 64
    BwdTeam,   // dense.hip              LDS team kernel, reference summation order
    BwdAny,    // general_any.hip        global memory, caller's scratch
    Check,     // check.hip              solution check, P (B,N,N): lanes per problem
    CheckDiag, // check.hip              solution check, P the compact diagonal (B,N)
    JvpDiag,   // jvp_diag.hip           forward-mode form of BwdDiag, P and dP the compact diagonals
    JvpTeam,   // jvp_dense.hip          forward-mode form of BwdTeam (LDS teams, reference order)
    JvpAny,    // jvp_any.hip            forward-mode form of BwdAny, caller's scratch
    PolishDiag,// polish_diag.hip        Newton polish, P the compact diagonal
    PolishTeam,// polish_dense.hip       Newton polish, LDS teams, N <= 64
    PolishAny, // polish_dense.hip       Newton polish, a workgroup per problem on the caller's scratch
    NewtonDiag,// newton_diag.hip        Newton derivatives (both modes), P the compact diagonal
    NewtonTeam,// newton_dense.hip       Newton derivatives, LDS teams, N <= 64
    NewtonAny, // newton_dense.hip       Newton derivatives, a workgroup per problem on the caller's scratch
    NewtonJacDiag, // newton_jac_diag.hip  Newton Jacobians, P the compact diagonal
    NewtonJacTeam, // newton_jac_dense.hip Newton Jacobians, LDS teams, N <= 64
    NewtonJacAny,  // newton_jac_dense.hip Newton Jacobians, a workgroup per problem on the caller's scratch
    ActiveDiag,    // active_diag.hip      active set, multipliers and margin, P the compact diagonal
    ActiveTeam,    // active_dense.hip     active set, multipliers and margin, LDS teams, N <= 64
    ActiveAny,     // active_dense.hip     active set, multipliers and margin, a workgroup per problem, no scratch
    PolishLsDiag,  // polish_diag_ls.hip   damped Newton polish (backtracking on the step length), P the compact diagonal
    PolishLsTeam,  // polish_dense_ls.hip  damped Newton polish, LDS teams, N <= 64
    PolishLsAny,   // polish_dense_ls.hip  damped Newton polish, a workgroup per problem on the caller's scratch
    PolishSmoothDiag,  // polish_diag_smooth.hip   smoothed damped polish (kappa > 0), P the compact diagonal
    PolishSmoothTeam,  // polish_dense_smooth.hip  smoothed damped polish, LDS teams, N <= 64
    PolishSmoothAny,   // polish_dense_smooth.hip  smoothed damped polish, a workgroup per problem on the caller's scratch
    NewtonSmoothDiag,  // newton_diag_smooth.hip   smoothed Newton derivatives (both modes), P the compact diagonal
    NewtonSmoothTeam,  // newton_dense_smooth.hip  smoothed Newton derivatives, LDS teams, N <= 64
    NewtonSmoothAny,   // newton_dense_smooth.hip  smoothed Newton derivatives, a workgroup per problem on the caller's scratch
    PolishPathDiag,    // polish_diag_path.hip     polish path (a kappa schedule in one launch), P the compact diagonal
    PolishPathTeam,    // polish_dense_path.hip    polish path, LDS teams, N <= 64
    PolishPathAny,     // polish_dense_path.hip    polish path, a workgroup per problem on the caller's scratch
    NewtonJacSmoothDiag,  // newton_jac_diag_smooth.hip   smoothed Newton Jacobians (kappa > 0), P the compact diagonal
    NewtonJacSmoothTeam,  // newton_jac_dense_smooth.hip  smoothed Newton Jacobians, LDS teams, N <= 64
    NewtonJacSmoothAny,   // newton_jac_dense_smooth.hip  smoothed Newton Jacobians, a workgroup per problem on the caller's scratch
};

// route counters (diagnostics, tuning.h): a hint flag moved this launch to another kernel
enum class Counter : unsigned char { None, FwdFeedbackRoutes, BwdWholeBatches, LaneListDrains };

struct Launch {
    Family family = Family::None;
    int lpp = 0;          // FwdDiag: lanes per problem
    bool fuse = false;    // FwdDiag / BwdDiag: non-diagonal tiles solved inside the kernel
    int lane_mode = 0;    // BwdLane: 0 the whole batch (declared dense), 1 the work-list, 2 the whole DQQ_P_AUTO batch, reporting
    Counter counter = Counter::None;
};

struct Plan {
    int err = 0;              // DQQ_E_UNSUPPORTED_N or 0
    Launch first;             // Family::None: nothing to launch (B = 0)
    Launch drain;             // behind `first`, in work-list mode: the problems it queued
    bool worklist = false;    // the kernels get the work-list of the caller's workspace
    bool scratch = false;     // ... and the global-memory scratch behind it (dqq_scratch_bytes)
    bool keep = false;        // forward: pdiag_out / diag_flags_out are written (else the flags are zeroed)
};

// the kernel-selection knobs of tuning.h that decide a route (the caller fills them from knob_*()).  "wpb" and
// "dense_teams" are not here: waves per workgroup and team width are launch geometry, read by the launchers themselves.
struct Knobs {
    int fwd_lpp, fuse_fallback, lane_dense, small_fwd, small_bwd, lane_bwd, fwd_feedback, bwd_skip_classify;
};

// argument errors (DQQ_E_BAD_SIZE / DQQ_E_BAD_LAYOUT) of a call, before anything else is looked at
// more_flags: per-call flags this entry knows besides the ones every entry knows (newton_family_flags below)
int check_call(int kind, int64_t B, int N, int p_layout, int more_flags = 0);
// the route of a call check_call accepted
Plan plan_fwd(int kind, int N, int64_t B, int p_layout, const Knobs& k);
Plan plan_bwd(int kind, int N, int64_t B, int p_layout, const Knobs& k);
// dqq_fwd_warm_f64: the route of a forward that starts from the caller's x0.  The cold plan's, family by family; a family
// without a warm form (fwd_family_warm: none today) is replaced by the LDS wave kernel / the global-memory kernel.
bool fwd_family_warm(Family f);
Plan plan_fwd_warm(int kind, int N, int64_t B, int p_layout, const Knobs& k);

// dqq_check_f64: the solution check of a batch (check.hip).  err: check_call's codes, DQQ_E_BAD_KIND; Family::None: B = 0.
// DQQ_P_AUTO is read as (B,N,N); the flags are accepted and ignored; any N in either layout.
struct CheckPlan {
    int err = 0;
    Family family = Family::None;
    int lanes = 0;   // per problem: check_lanes(N)
};
// The check's lane mapping (check_core.h has the order of evaluation that follows from it): 2 adjacent columns per lane for even N
// (16-byte loads), 1 for odd N; the fewest lanes, a power of two <= 64, that hold a row -- so that small N still fill a wave.
constexpr int check_cols_per_lane(int N) { return (N % 2) == 0 ? 2 : 1; }
constexpr int check_lanes(int N)
{
    const int need = (N + check_cols_per_lane(N) - 1) / check_cols_per_lane(N);
    int L = 1;
    while (L < need && L < 64) L *= 2;
    return L;
}
CheckPlan plan_check(int kind, int N, int64_t B, int p_layout);

// dqq_jvp_f64: the route of a forward-mode derivative.  err: DQQ_E_BAD_KIND, then check_call's codes and DQQ_E_UNSUPPORTED_N
// (DQQ_P_DIAG off the fast N); Family::None: B = 0.  DQQ_P_DIAG: JvpDiag; DQQ_P_AUTO and DQQ_P_DENSE: the reference-order
// kernels whatever the flags say -- JvpTeam up to max_n(., true) of the kind's backward (QP 64, QCQP 42, box kinds 21), JvpAny
// beyond, on the scratch of the backward's global-memory kernel.
struct JvpPlan {
    int err = 0;
    Family family = Family::None;
    bool scratch = false;   // JvpAny: dqq_scratch_bytes(kind == 3 ? 2 : kind, 1, N, B, p_layout | DQQ_F_REFERENCE_ORDER)
};
JvpPlan plan_jvp(int kind, int N, int64_t B, int p_layout);

// DQQ_F_INFINITE_BOUNDS is a flag of the Newton family alone (dqq_polish_f64, dqq_newton_bwd_f64, dqq_newton_jvp_f64,
// dqq_newton_jac_f64) and of the kinds that have extras: the box kinds (2, 3) honour it -- their plans carry it as inf_bounds
// --, the QCQP accepts and ignores it (its radii stay finite-only).  To the QP, which has no bounds, and to every other entry
// the bit stays an unknown one: DQQ_E_BAD_LAYOUT, as before the flag existed.
constexpr int newton_family_flags(int kind) { return kind >= kKindQCQP && kind <= kKindSignedBox ? DQQ_F_INFINITE_BOUNDS : 0; }
constexpr bool plan_inf_bounds(int kind, int p_layout)
{
    return (kind == kKindBox || kind == kKindSignedBox) && (p_layout & DQQ_F_INFINITE_BOUNDS) != 0;
}

// The Newton family's route: one table for its five entry groups (plan_newton_family, route.cpp).  err: DQQ_E_BAD_KIND, then
// check_call's codes and DQQ_E_UNSUPPORTED_N (DQQ_P_DIAG off the fast N); Family::None: B = 0.  DQQ_P_DIAG: the group's diagonal
// family; DQQ_P_AUTO and DQQ_P_DENSE, never classified: the group's team family up to N = 64 (the matrix in LDS), its any-N family
// beyond (a workgroup per problem), on the group's dqq_*_scratch_bytes of the caller's scratch.  B plays no part.  Flags: ignored,
// but DQQ_F_INFINITE_BOUNDS (above).
//   group        entries                                      diagonal       team           any-N          scratch
//   Polish       dqq_polish_f64, dqq_polish_reg_f64           PolishDiag     PolishTeam     PolishAny      dqq_polish_scratch_bytes
//   PolishLs     dqq_polish_ls_f64                            PolishLsDiag   PolishLsTeam   PolishLsAny    dqq_polish_scratch_bytes
//   Derivative   dqq_newton_bwd*_f64, dqq_newton_jvp*_f64     NewtonDiag     NewtonTeam     NewtonAny      dqq_newton_scratch_bytes
//   Jacobian     dqq_newton_jac*_f64                          NewtonJacDiag  NewtonJacTeam  NewtonJacAny   dqq_newton_jac_scratch_bytes
//   Active       dqq_newton_active_f64                        ActiveDiag     ActiveTeam     ActiveAny      none: no workspace
// The derivative's route is the same for both modes.  The active set needs scratch on no route: its `scratch` stays false and
// its entry has no workspace argument.
//   PolishSmooth      dqq_polish_smooth_f64, kappa > 0        PolishSmoothDiag / Team / Any              dqq_polish_scratch_bytes
//   DerivativeSmooth  dqq_newton_{bwd,jvp}_smooth_f64, > 0    NewtonSmoothDiag / Team / Any              dqq_newton_scratch_bytes
//   PolishPath        dqq_polish_path_f64, every schedule     PolishPathDiag / Team / Any                dqq_polish_scratch_bytes
//   JacobianSmooth    dqq_newton_jac_smooth_f64, kappa > 0    NewtonJacSmoothDiag / Team / Any           dqq_newton_jac_scratch_bytes
enum class NewtonGroup : unsigned char {
    Polish, PolishLs, Derivative, Jacobian, Active, PolishSmooth, DerivativeSmooth, PolishPath, JacobianSmooth
};
enum class NewtonRoute : unsigned char { None, Diag, Team, Any };   // which column of the table `family` is from
struct NewtonFamilyPlan {
    int err = 0;
    Family family = Family::None;
    bool scratch = false;      // the any-N family of every group but Active
    bool inf_bounds = false;   // box kinds with DQQ_F_INFINITE_BOUNDS: the kernels admit one-sided boxes (polish_core.h)
    bool reg = false;          // a *_reg_f64 call with reg != 0: the family's REG = true kernels (plan_polish_reg below)
    bool smooth = false;       // a *_smooth_f64 call with kappa != 0: the smoothed families (plan_polish_smooth below)
    NewtonRoute route = NewtonRoute::None;
};
using PolishPlan = NewtonFamilyPlan;
using NewtonPlan = NewtonFamilyPlan;
using NewtonJacPlan = NewtonFamilyPlan;
using NewtonActivePlan = NewtonFamilyPlan;
constexpr int kPolishTeamMaxN = 64;
constexpr int kNewtonTeamMaxN = 64;
// inf_flag: whether the entry knows DQQ_F_INFINITE_BOUNDS at all (the smoothed entries do not)
NewtonFamilyPlan plan_newton_family(NewtonGroup group, int kind, int N, int64_t B, int p_layout, bool inf_flag = true);
// ... under the entries' own names (one-line forwards)
PolishPlan plan_polish(int kind, int N, int64_t B, int p_layout);
NewtonPlan plan_newton(int kind, int N, int64_t B, int p_layout);
NewtonJacPlan plan_newton_jac(int kind, int N, int64_t B, int p_layout);
NewtonActivePlan plan_newton_active(int kind, int N, int64_t B, int p_layout);

// dqq_polish_reg_f64, dqq_newton_bwd_reg_f64 / dqq_newton_jvp_reg_f64, dqq_newton_jac_reg_f64: the parent's plan, and `reg` set
// where a kernel is launched with a proximal weight that is not a zero (either sign of zero: the parent's kernels).  A reg that
// is negative, a NaN or infinite is an argument error, DQQ_E_BAD_SIZE, after the parent's kind, size and layout errors and
// before everything else (a NULL pointer, DQQ_E_UNSUPPORTED_N, the workspace) -- with B = 0 too; nothing is launched.
constexpr bool reg_ok(double reg) { return reg >= 0.0 && reg <= 1.7976931348623157e308; }
PolishPlan plan_polish_reg(int kind, int N, int64_t B, int p_layout, double reg);
NewtonPlan plan_newton_reg(int kind, int N, int64_t B, int p_layout, double reg);
NewtonJacPlan plan_newton_jac_reg(int kind, int N, int64_t B, int p_layout, double reg);

// dqq_polish_ls_f64: plan_polish_reg's plan on the damped polish's own families, whatever max_halvings is -- 0 runs the damped
// kernels with no halving allowed, which give the parents' bits.  The kernels take reg as a run-time argument, so `reg` only
// reports reg != 0.  max_halvings outside 0 .. kPolishMaxHalvings is an argument error, DQQ_E_BAD_OPTION, after the kind, size
// and layout errors and reg's DQQ_E_BAD_SIZE and before everything else (a NULL pointer, DQQ_E_UNSUPPORTED_N, the workspace) --
// with B = 0 too; nothing is launched.  2^-60 is the smallest step length: t stays an exact power of two.
constexpr int kPolishMaxHalvings = 60;
PolishPlan plan_polish_ls(int kind, int N, int64_t B, int p_layout, double reg, int max_halvings);

// dqq_polish_smooth_f64, dqq_newton_bwd_smooth_f64 / dqq_newton_jvp_smooth_f64: the parents' plans (plan_polish_ls,
// plan_newton_reg) on the smoothed families where kappa is not a zero; kappa == 0 (either sign) is the parent's plan itself, on
// the parent's families, and `smooth` stays false: the entry then launches the parent's kernels.  The smoothed kernels take reg as
// a run-time argument, so `reg` only reports reg != 0.  DQQ_F_INFINITE_BOUNDS is an unknown bit to these entries for every kind
// (DQQ_E_BAD_LAYOUT): one-sided boxes under smoothing are out of scope.  A kappa that is negative, a NaN or infinite is an argument
// error, DQQ_E_BAD_OPTION, where plan_polish_ls refuses max_halvings: after the kind, size and layout errors and reg's
// DQQ_E_BAD_SIZE and before everything else -- with B = 0 too; nothing is launched.
constexpr bool kappa_ok(double kappa) { return kappa >= 0.0 && kappa <= 1.7976931348623157e308; }
PolishPlan plan_polish_smooth(int kind, int N, int64_t B, int p_layout, double reg, int max_halvings, double kappa);
NewtonPlan plan_newton_smooth(int kind, int N, int64_t B, int p_layout, double reg, double kappa);
// dqq_newton_jac_smooth_f64: by the same rules, plan_newton_jac_reg's plan on the NewtonJacSmooth families where kappa is not a
// zero (scratch: the any-N family on dqq_newton_jac_scratch_bytes); kappa == 0 is plan_newton_jac_reg's plan itself but for the
// flag rule -- DQQ_F_INFINITE_BOUNDS stays an unknown bit, one rule per entry.
NewtonJacPlan plan_newton_jac_smooth(int kind, int N, int64_t B, int p_layout, double reg, double kappa);

// dqq_polish_path_f64: the smoothed polish's plan (route, scratch, flags: DQQ_F_INFINITE_BOUNDS is an unknown bit here too, even
// when every kappa is 0 -- one rule per entry) on the path's own families, whatever the schedule is: a single stage, and a
// schedule of zeros, run the path kernels too.  `smooth` stays false and `reg` only reports reg != 0: the kernels look at every
// kappa_s and at reg at run time.  kappas, stage_steps: the caller's HOST arrays of n_stages entries.  The schedule's own errors
// stand where plan_polish_smooth refuses kappa -- after the kind, size and layout errors and reg's DQQ_E_BAD_SIZE, before
// everything else, with B = 0 too; nothing is launched: DQQ_E_BAD_OPTION for n_stages outside 1 .. kPolishPathMaxStages or
// max_halvings outside 0 .. kPolishMaxHalvings, then DQQ_E_NULLPTR for a NULL kappas or stage_steps, then DQQ_E_BAD_OPTION for a
// kappa_s that is negative, a NaN or infinite or a stage_steps[s] < 0.
constexpr int kPolishPathMaxStages = 8;
PolishPlan plan_polish_path(int kind, int N, int64_t B, int p_layout, double reg, const double* kappas, const int* stage_steps,
                            int n_stages, int max_halvings);

// dqq_max_n: which 0 QP forward/backward and the box forwards, 1 QCQP forward, 2 QCQP backward, 3 box QP backward
int max_n(int which, bool ref_order);
// beyond max_n the global-memory kernels take the general path's problems (dqq_scratch_bytes)
bool general_needs_scratch(int kind, int pass, int N, bool ref_order);
// the lane-per-problem backward fills the chip with a batch (or a work-list) of B problems (dqq_hint_flags)
bool bwd_lane_fills_chip(int kind, int N, int64_t B);

// The pure queries of the C ABI (capi.hip forwards to them; tests/test_routes.py reaches them without a GPU).
// dqq_hint_flags: the flags for a call of (kind, pass, N, B) from the caller's report word (report.h)
int hint_flags(int kind, int pass, int N, int64_t B, unsigned long long last_report);
// dqq_workspace_bytes: the work-list's header and entry area (worklist.h), rounded up to 64 ints
size_t workspace_bytes(int64_t B);
// dqq_scratch_bytes is not 0 for these arguments (how much then: any_scratch_bytes, general_any.hip)
bool scratch_applies(int kind, int pass, int N, int64_t B, int p_layout);

} // namespace dqq
