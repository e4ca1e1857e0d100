// launch.h -- the launch() wrapper, the argument bundles and the launcher prototypes shared by the kernel translation units
// and capi.hip.  The work-list protocol is worklist.h, the report word report.h: a unit includes what it uses.
#pragma once

#include "../../include/diffqcqp_hip.h"
#include "common.h"
#include "route.h"
#include "tuning.h"

#include <tuple>
#include <type_traits>
#include <utility>

namespace dqq {

// Kernel launch that reports ITS OWN status: hipLaunchKernel's return value, not hipGetLastError() -- the
// thread's sticky error slot belongs to the caller (a stale error of theirs is neither returned as ours nor
// cleared).
template <typename... KArgs, typename... Args, size_t... I>
static inline hipError_t launch_impl(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t s,
                                     std::index_sequence<I...>, Args&&... args)
{
    std::tuple<KArgs...> params{static_cast<KArgs>(args)...};
    void* ptrs[] = {static_cast<void*>(&std::get<I>(params))...};
    return hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, ptrs, lds, s);
}
template <typename... KArgs, typename... Args>
static inline hipError_t launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t s, Args&&... args)
{
    static_assert(sizeof...(KArgs) == sizeof...(Args), "kernel argument count");
    return launch_impl(kernel, grid, block, lds, s, std::index_sequence_for<KArgs...>{}, std::forward<Args>(args)...);
}
// launch() of a kernel that may need more than 48 KiB of dynamic LDS: such a kernel has to opt in first.  The attribute is
// set on every such launch (the library keeps no state), and only above 48 KiB.
template <typename... KArgs, typename... Args>
static inline hipError_t launch_lds(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t s, Args&&... args)
{
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        if (e != hipSuccess) return e;
    }
    return launch(kernel, grid, block, lds, s, std::forward<Args>(args)...);
}

// The switch over the kinds of the Newton family's launchers: f(std::integral_constant<int, KIND>) with KIND = 0 .. 3 for
// kKindQP .. kKindSignedBox.  A generic lambda takes it: [&](auto k) { return launch_x<decltype(k)::value>(...); }.
template <typename F>
static inline hipError_t dispatch_kind(int kind, F&& f)
{
    switch (kind) {
    case kKindQP: return f(std::integral_constant<int, 0>{});
    case kKindQCQP: return f(std::integral_constant<int, 1>{});
    case kKindBox: return f(std::integral_constant<int, 2>{});
    case kKindSignedBox: return f(std::integral_constant<int, 3>{});
    default: return hipErrorInvalidValue;
    }
}

struct FwdArgs {
    const double* P;
    const double* q;
    const double* l_n; // QCQP: (B,N/2) normal forces; box kinds: (B,N) l_min
    const double* mu;  // QCQP: (B,N/2) friction coefficients; box kinds: (B,N) l_max
    const double* v;   // signed box QP only: (B,N)
    double* x;
    long B;
    int N;
    double eps, mu_prox;
    int max_iter, adaptive, layout;
    int* iters;
    int* ws;
    double* pdiag_out;         // optional (B,N): the diagonal of P, for the backward of the same problems
    unsigned char* flags_out;  // optional (B): 1 = the problem's tile was verified diagonal
    double* scratch = nullptr; // caller's scratch behind the work-list (dqq_scratch_bytes), global-memory kernels only
    const double* x0 = nullptr; // dqq_fwd_warm_f64 only: (B,N,1) start point of every problem; NULL = the cold start
};

struct BwdArgs {
    const double* P;
    const double* q;
    const double* l_n;
    const double* mu;
    const double* v = nullptr;  // signed box QP only: (B,N,1), see FwdArgs
    const double* x;
    const double* grad_x;
    double* grad_P;
    double* grad_q;
    double* grad_l_n;
    double* grad_mu;
    const double* pdiag;        // optional: what the forward stored (see FwdArgs)
    const unsigned char* flags; // optional
    double* gamma;   // QCQP only, optional
    double* dgamma;  // QCQP only, optional
    long B;
    int N;
    double epsilon;  // dual-recovery threshold (reference default 1e-10)
    int layout;
    int* ir_steps;
    int* ws;
    double* scratch = nullptr; // see FwdArgs
    unsigned long long* report = nullptr;   // optional: where the drain launch stores what it found (device-writable host word)
};

// dqq_check_f64 (check.hip): a, b, c are the kind's extras -- QCQP l_n, mu (B,N/2); box l_min, l_max (B,N); signed box also v
struct CheckArgs {
    const double* P;
    const double* q;
    const double* a;
    const double* b;
    const double* c;
    const double* x;
    const int* iters;   // optional
    int max_iter;
    long B;
    int N;
    double* resid;                // (B,4), optional
    int* status;                  // (B), optional
    unsigned long long* counts;   // 3 words the caller zeroed, optional
};

// dqq_jvp_f64 (jvp_diag.hip, jvp_dense.hip, jvp_any.hip): a, b the kind's first two extras, v the signed box QP's; dP, dq, da, db
// the tangents of P, q, a, b (NULL = zero)
struct JvpArgs {
    const double* P;
    const double* q;
    const double* a;
    const double* b;
    const double* v;
    const double* x;
    const double* dP;
    const double* dq;
    const double* da;
    const double* db;
    double* dx;
    long B;
    int N;
    double epsilon;
    int* ir_steps;             // optional: (B), box kinds (B,2)
    double* scratch = nullptr; // JvpAny: the caller's scratch behind the work-list (dqq_scratch_bytes of the backward)
};

// dqq_polish_f64 (polish_diag.hip, polish_dense.hip): a, b, c the kind's extras as CheckArgs has them; x_out may be x
struct PolishArgs {
    const double* P;
    const double* q;
    const double* a;
    const double* b;
    const double* c;
    const double* x;
    double* x_out;
    long B;
    int N;
    int max_steps;
    double* resid;             // (B,2), optional: r before and after
    int* steps;                // (B), optional: accepted steps
    int* status;               // (B), optional
    double* scratch = nullptr; // PolishAny: the caller's scratch (dqq_polish_scratch_bytes)
    int inf_bounds = 0;        // DQQ_F_INFINITE_BOUNDS of a box kind (the plan's inf_bounds): polish_core.h's inf_ok
};

// dqq_newton_bwd_f64 / dqq_newton_jvp_f64 (newton_diag.hip, newton_dense.hip): a, b, c the kind's extras as CheckArgs has
// them.  Backward: in0 = grad_x, out0 .. out3 = grad_P, grad_q, grad_a, grad_b (each optional).  JVP: in0 .. in3 = dP, dq, da, db
// (each optional: NULL = zero), out0 = dx.
struct NewtonArgs {
    const double* P;
    const double* q;
    const double* a;
    const double* b;
    const double* c;
    const double* x;
    const double* in0;
    const double* in1;
    const double* in2;
    const double* in3;
    double* out0;
    double* out1;
    double* out2;
    double* out3;
    long B;
    int N;
    int* status;               // (B), optional
    double* scratch = nullptr; // NewtonAny: the caller's scratch (dqq_newton_scratch_bytes)
    int inf_bounds = 0;        // DQQ_F_INFINITE_BOUNDS of a box kind (the plan's inf_bounds): polish_core.h's inf_ok
};

// dqq_newton_jac_f64 (newton_jac_diag.hip, newton_jac_dense.hip): a, b, c the kind's extras as CheckArgs has them; Jq, Ja, Jb each
// optional (NULL = not requested), shaped as include/diffqcqp_hip.h says.
struct NewtonJacArgs {
    const double* P;
    const double* q;
    const double* a;
    const double* b;
    const double* c;
    const double* x;
    double* Jq;
    double* Ja;
    double* Jb;
    long B;
    int N;
    int* status;               // (B), optional
    double* scratch = nullptr; // NewtonJacAny: the caller's scratch (dqq_newton_jac_scratch_bytes)
    int inf_bounds = 0;        // DQQ_F_INFINITE_BOUNDS of a box kind (the plan's inf_bounds): polish_core.h's inf_ok
};

// dqq_newton_active_f64 (active_diag.hip, active_dense.hip): a, b, c the kind's extras as CheckArgs has them; every output
// optional (NULL = not requested), shaped as include/diffqcqp_hip.h says.  No scratch: no family of this entry needs any.
struct ActiveArgs {
    const double* P;
    const double* q;
    const double* a;
    const double* b;
    const double* c;
    const double* x;
    int* state;                // (B,N), QCQP (B,N/2)
    double* mult;              // as state
    double* margin;            // (B)
    int* where;                // (B)
    int* status;               // (B)
    long B;
    int N;
    int inf_bounds = 0;        // DQQ_F_INFINITE_BOUNDS of a box kind (the plan's inf_bounds): polish_core.h's inf_ok
};

// dqq_equilibrate_f64 (equil.hip): a, b, c the kind's extras as CheckArgs has them; P (B,N,N) or the compact diagonal (B,N), P_out
// as P.  x0 and the extras are optional: an input whose output is NULL is not read.
struct EquilArgs {
    const double* P;
    const double* q;
    const double* a;
    const double* b;
    const double* c;
    const double* x0;
    double* P_out;
    double* q_out;
    double* a_out;
    double* b_out;
    double* c_out;
    double* x0_out;
    int* e_out;                // (B,N): the exponents (equil_core.h)
    long B;
    int N;
};

// One launcher per kernel family of route.h: what the plan decided comes in, each keeps its own geometry and its switch over
// the instantiated (KIND, N).  use_worklist: solve only the problems the fast path queued in a.ws, then re-zero the work-list
// header.  B > 0: the plan launches nothing for an empty batch (Family::None, tests/test_routes.py).
hipError_t launch_fwd_diag(int kind, const FwdArgs& a, int lpp, bool fuse, hipStream_t s);        // fwd_diag.hip
hipError_t launch_fwd_diag_warm(int kind, const FwdArgs& a, int lpp, bool fuse, hipStream_t s);   // fwd_diag_warm.hip (a.x0)
hipError_t launch_fwd_lane_dense(int kind, const FwdArgs& a, bool use_worklist, hipStream_t s);   // fwd_lane_dense.hip
hipError_t launch_fwd_small(int kind, const FwdArgs& a, bool use_worklist, hipStream_t s);        // fwd_small.hip
hipError_t launch_fwd_dense_wave64(int kind, const FwdArgs& a, bool use_worklist, hipStream_t s); // dense_wave64.hip
hipError_t launch_fwd_dense(int kind, const FwdArgs& a, bool use_worklist, hipStream_t s);        // dense.hip
hipError_t launch_fwd_any(int kind, const FwdArgs& a, bool use_worklist, hipStream_t s);          // general_any.hip
hipError_t launch_bwd_diag(int kind, const BwdArgs& a, bool fuse, hipStream_t s);                 // bwd_diag.hip
// mode 0: the whole batch, declared dense; 1: the entries of the work-list; 2: the whole batch of a DQQ_P_AUTO call, reporting
hipError_t launch_bwd_lane_dense(int kind, const BwdArgs& a, int mode, hipStream_t s);            // bwd_lane_dense.hip
hipError_t launch_bwd_small(int kind, const BwdArgs& a, bool use_worklist, hipStream_t s);        // bwd_small.hip
hipError_t launch_bwd_dense_wave64(int kind, const BwdArgs& a, bool use_worklist, hipStream_t s); // dense_wave64.hip (QP)
hipError_t launch_bwd_wave_qcqp(const BwdArgs& a, bool use_worklist, hipStream_t s);              // bwd_wave_qcqp.hip
hipError_t launch_bwd_wave_qcqp_big(const BwdArgs& a, bool use_worklist, hipStream_t s);          // bwd_wave_qcqp_big.hip
hipError_t launch_bwd_dense(int kind, const BwdArgs& a, bool use_worklist, hipStream_t s);        // dense.hip
hipError_t launch_bwd_any(int kind, const BwdArgs& a, bool use_worklist, hipStream_t s);          // general_any.hip
// Family::Check / Family::CheckDiag (diag: P is (B,N)), `lanes` per problem as plan_check decided
hipError_t launch_check(int kind, const CheckArgs& a, bool diag, int lanes, hipStream_t s);       // check.hip
// diag: P is (B,N), N even; else (B,N,N) on check.hip's lane mapping (check_lanes(N)).  unscale: n = B N elements, x may be y
hipError_t launch_equil(int kind, const EquilArgs& a, bool diag, hipStream_t s);                  // equil.hip
hipError_t launch_unscale(const double* y, const int* e, double* x, long n, hipStream_t s);       // equil.hip
hipError_t launch_jvp_diag(int kind, const JvpArgs& a, hipStream_t s);                            // jvp_diag.hip
hipError_t launch_jvp_dense(int kind, const JvpArgs& a, hipStream_t s);                           // jvp_dense.hip
hipError_t launch_jvp_any(int kind, const JvpArgs& a, hipStream_t s);                             // jvp_any.hip
hipError_t launch_polish_diag(int kind, const PolishArgs& a, hipStream_t s);                      // polish_diag.hip
// any: Family::PolishAny (a workgroup per problem on a.scratch), else Family::PolishTeam (LDS teams, N <= 64)
hipError_t launch_polish_dense(int kind, const PolishArgs& a, bool any, hipStream_t s);           // polish_dense.hip
// bytes of scratch PolishAny needs for (N, B): a slice per workgroup of any_grid (0 for B <= 0)
size_t polish_scratch_bytes(int N, long B);
// jvp: dqq_newton_jvp_f64, else dqq_newton_bwd_f64
hipError_t launch_newton_diag(int kind, bool jvp, const NewtonArgs& a, hipStream_t s);            // newton_diag.hip
// any: Family::NewtonAny (a workgroup per problem on a.scratch), else Family::NewtonTeam (LDS teams, N <= 64)
hipError_t launch_newton_dense(int kind, bool jvp, const NewtonArgs& a, bool any, hipStream_t s); // newton_dense.hip
// bytes of scratch NewtonAny needs for (N, B): a slice per workgroup of any_grid (0 for B <= 0)
size_t newton_scratch_bytes(int N, long B);
hipError_t launch_newton_jac_diag(int kind, const NewtonJacArgs& a, hipStream_t s);              // newton_jac_diag.hip
// any: Family::NewtonJacAny (a workgroup per problem on a.scratch), else Family::NewtonJacTeam (LDS teams, N <= 64)
hipError_t launch_newton_jac_dense(int kind, const NewtonJacArgs& a, bool any, hipStream_t s);   // newton_jac_dense.hip
// bytes of scratch NewtonJacAny needs for (kind, N, B): a slice per workgroup of any_grid (0 for B <= 0)
size_t newton_jac_scratch_bytes(int kind, int N, long B);
// The *_reg_f64 entries with reg != 0 (the plan's `reg` field): the same kernels instantiated with REG = true, each family in a
// translation unit of its own; reg is a plain kernel argument.  Geometry, scratch and LDS are the parents'.
hipError_t launch_polish_diag_reg(int kind, const PolishArgs& a, double reg, hipStream_t s);                      // polish_diag_reg.hip
hipError_t launch_polish_dense_reg(int kind, const PolishArgs& a, double reg, bool any, hipStream_t s);           // polish_dense_reg.hip
hipError_t launch_newton_diag_reg(int kind, bool jvp, const NewtonArgs& a, double reg, hipStream_t s);            // newton_diag_reg.hip
hipError_t launch_newton_dense_reg(int kind, bool jvp, const NewtonArgs& a, double reg, bool any, hipStream_t s); // newton_dense_reg.hip
hipError_t launch_newton_jac_diag_reg(int kind, const NewtonJacArgs& a, double reg, hipStream_t s);               // newton_jac_diag_reg.hip
hipError_t launch_newton_jac_dense_reg(int kind, const NewtonJacArgs& a, double reg, bool any, hipStream_t s);    // newton_jac_dense_reg.hip
// dqq_polish_ls_f64 (Family::PolishLs*): what the damped polish takes besides PolishArgs -- kernel arguments of their own, so
// that PolishArgs and with it the parents' kernels stay what they are.  Geometry, scratch and LDS are the parents'.
struct PolishLsOpts {
    double reg;         // the proximal weight, looked at at run time (polish_reg)
    int max_halvings;   // 0 .. kPolishMaxHalvings
    int* halvings;      // (B), optional
};
hipError_t launch_polish_diag_ls(int kind, const PolishArgs& a, const PolishLsOpts& o, hipStream_t s);            // polish_diag_ls.hip
hipError_t launch_polish_dense_ls(int kind, const PolishArgs& a, const PolishLsOpts& o, bool any, hipStream_t s); // polish_dense_ls.hip
// dqq_polish_smooth_f64, dqq_newton_bwd_smooth_f64 / dqq_newton_jvp_smooth_f64 with kappa > 0 (Family::*Smooth*; smooth_core.h):
// kappa travels in the second kernel argument, next to what the parents carry there.  Geometry, scratch and LDS are the parents'.
struct PolishSmoothOpts {
    double reg;         // the proximal weight, looked at at run time (polish_reg)
    double kappa;       // > 0, finite
    int max_halvings;   // 0 .. kPolishMaxHalvings
    int* halvings;      // (B), optional
};
struct NewtonSmoothOpts {
    double reg;         // the proximal weight, looked at at run time (polish_reg)
    double kappa;       // > 0, finite
};
hipError_t launch_polish_diag_smooth(int kind, const PolishArgs& a, const PolishSmoothOpts& o, hipStream_t s);            // polish_diag_smooth.hip
hipError_t launch_polish_dense_smooth(int kind, const PolishArgs& a, const PolishSmoothOpts& o, bool any, hipStream_t s); // polish_dense_smooth.hip
hipError_t launch_newton_diag_smooth(int kind, bool jvp, const NewtonArgs& a, const NewtonSmoothOpts& o, hipStream_t s);            // newton_diag_smooth.hip
hipError_t launch_newton_dense_smooth(int kind, bool jvp, const NewtonArgs& a, const NewtonSmoothOpts& o, bool any, hipStream_t s); // newton_dense_smooth.hip
// dqq_newton_jac_smooth_f64 with kappa != 0 (Family::NewtonJacSmooth*): what the smoothed Jacobians take besides NewtonJacArgs -- a
// kernel argument of its own, so that NewtonJacArgs and with it the parents' kernels stay what they are.  Geometry, scratch
// (dqq_newton_jac_scratch_bytes) and LDS are the hard Jacobian kernels'.
struct NewtonJacSmoothOpts {
    double reg;         // the proximal weight, looked at at run time (polish_reg)
    double kappa;       // > 0, finite
};
hipError_t launch_newton_jac_diag_smooth(int kind, const NewtonJacArgs& a, const NewtonJacSmoothOpts& o, hipStream_t s);            // newton_jac_diag_smooth.hip
hipError_t launch_newton_jac_dense_smooth(int kind, const NewtonJacArgs& a, const NewtonJacSmoothOpts& o, bool any, hipStream_t s); // newton_jac_dense_smooth.hip
// dqq_polish_path_f64 (Family::PolishPath*; path_core.h): the whole schedule by value in the second kernel argument -- the
// caller's host arrays are copied here, so a captured launch replays the captured schedule.  PolishArgs' max_steps is not read;
// resid, steps and status there are the path's summary outputs.  Geometry, scratch and LDS are the smoothed polish's.
struct PolishPathOpts {
    double reg;                              // the proximal weight, looked at at run time (polish_reg)
    double kappa[kPolishPathMaxStages];      // per stage, >= 0 and finite; 0: the hard damped polish's functions
    int budget[kPolishPathMaxStages];        // per stage: the cap on accepted steps, >= 0
    int n_stages;                            // 1 .. kPolishPathMaxStages
    int max_halvings;                        // 0 .. kPolishMaxHalvings
    int* halvings;                           // (B), optional: summed over the stages
    double* stage_resid;                     // (B,S,2), optional
    int* stage_steps;                        // (B,S), optional
};
hipError_t launch_polish_diag_path(int kind, const PolishArgs& a, const PolishPathOpts& o, hipStream_t s);            // polish_diag_path.hip
hipError_t launch_polish_dense_path(int kind, const PolishArgs& a, const PolishPathOpts& o, bool any, hipStream_t s); // polish_dense_path.hip
hipError_t launch_active_diag(int kind, const ActiveArgs& a, hipStream_t s);                     // active_diag.hip
// any: Family::ActiveAny (a workgroup per problem, rows in chunks), else Family::ActiveTeam (LDS teams, N <= 64)
hipError_t launch_active_dense(int kind, const ActiveArgs& a, bool any, hipStream_t s);          // active_dense.hip
// bytes of scratch the global-memory kernels need for (kind, N, B): a slice per workgroup of a grid that depends on (N, B) only
size_t any_scratch_bytes(int kind, bool backward, int N, long B);
// ... the backward's slice in doubles, and the persistent grid of (B, slice) -- jvp_any.hip runs on the same geometry
long any_bwd_stride(int kind, int N);
unsigned any_grid(long B, long stride);

} // namespace dqq
