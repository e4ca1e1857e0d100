// capi.hip -- the extern "C" boundary declared in include/diffqcqp_hip.h: argument checks, then the route plan of the call
// (route.cpp: diagonal fast path / general dense kernel / both, chained through the fallback work-list) executed on the
// caller's stream.
#include <atomic>
#include <cstring>

#include "launch.h"
#include "worklist.h"

namespace dqq {
// route counters (tuning.h)
std::atomic<int> g_bwd_whole_batches{0};
std::atomic<int> g_lane_list_drains{0};
std::atomic<int> g_fwd_feedback_routes{0};
#if defined(DQQ_TUNING)
// developer build: the knobs of tuning.h as process-wide atomics (defined here, declared there)
#define DQQ_KNOB_DEF(name, dflt) std::atomic<int> g_##name{dflt};
DQQ_KNOBS(DQQ_KNOB_DEF)
#undef DQQ_KNOB_DEF
#endif
}

namespace {

struct Option {
    const char* name;
    std::atomic<int>* slot;
};
// What dqq_set_option / dqq_get_option know.  Shipped build: the three route counters (diagnostics; "set" resets them) and
// nothing else -- no name here changes what a call does.  Developer build (-DDQQ_TUNING): also the knobs of tuning.h.
Option g_options[] = {{"lane_list_drains", &dqq::g_lane_list_drains},
                      {"bwd_whole_batches", &dqq::g_bwd_whole_batches},
                      {"fwd_feedback_routes", &dqq::g_fwd_feedback_routes},
#if defined(DQQ_TUNING)
#define DQQ_KNOB_OPT(name, dflt) {#name, &dqq::g_##name},
                      DQQ_KNOBS(DQQ_KNOB_OPT)
#undef DQQ_KNOB_OPT
#endif
};

// p_layout as passed = layout | flags
bool ref_order_of(int p_layout) { return (p_layout & DQQ_F_REFERENCE_ORDER) != 0; }

// the knobs of tuning.h that decide routes (compile-time constants in the shipped build)
dqq::Knobs knobs()
{
    return {dqq::knob_fwd_lpp(),  dqq::knob_fuse_fallback(), dqq::knob_lane_dense(),  dqq::knob_small_fwd(),
            dqq::knob_small_bwd(), dqq::knob_lane_bwd(),     dqq::knob_fwd_feedback(), dqq::knob_bwd_skip_classify()};
}

int check_ws(const void* ws, size_t bytes, int64_t B, size_t scratch_bytes = 0)
{
    if (ws == nullptr || bytes < dqq_workspace_bytes(B) + scratch_bytes) return DQQ_E_WORKSPACE;
    return 0;
}

// the scratch slice behind the work-list (dqq_scratch_bytes)
double* scratch_of(void* ws, int64_t B)
{
    return reinterpret_cast<double*>(static_cast<char*>(ws) + dqq_workspace_bytes(B));
}

// A launch of the work-list chain failed: the entries the fast kernel queued will never be drained.  Re-zero the header
// so that the stale count cannot leak into the next call on this workspace (best effort; the error is what is returned).
void reset_worklist(void* ws, hipStream_t s)
{
    if (ws != nullptr) (void)hipMemsetAsync(ws, 0, sizeof(int) * dqq::kWsEntries, s);
}

void count(dqq::Counter c)
{
    switch (c) {
    case dqq::Counter::FwdFeedbackRoutes: dqq::g_fwd_feedback_routes.fetch_add(1, std::memory_order_relaxed); break;
    case dqq::Counter::BwdWholeBatches: dqq::g_bwd_whole_batches.fetch_add(1, std::memory_order_relaxed); break;
    case dqq::Counter::LaneListDrains: dqq::g_lane_list_drains.fetch_add(1, std::memory_order_relaxed); break;
    default: break;
    }
}

hipError_t launch(const dqq::Launch& l, int kind, const dqq::FwdArgs& a, bool wl, hipStream_t s)
{
    using dqq::Family;
    count(l.counter);
    switch (l.family) {
    case Family::FwdDiag:   // (the warm instantiations are a translation unit of their own; the others branch on a.x0 themselves)
        return a.x0 != nullptr ? dqq::launch_fwd_diag_warm(kind, a, l.lpp, l.fuse, s) : dqq::launch_fwd_diag(kind, a, l.lpp, l.fuse, s);
    case Family::FwdLane: return dqq::launch_fwd_lane_dense(kind, a, wl, s);
    case Family::FwdSmall: return dqq::launch_fwd_small(kind, a, wl, s);
    case Family::FwdWave64: return dqq::launch_fwd_dense_wave64(kind, a, wl, s);
    case Family::FwdLds: return dqq::launch_fwd_dense(kind, a, wl, s);
    case Family::FwdAny: return dqq::launch_fwd_any(kind, a, wl, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch(const dqq::Launch& l, int kind, const dqq::BwdArgs& a, bool wl, hipStream_t s)
{
    using dqq::Family;
    count(l.counter);
    switch (l.family) {
    case Family::BwdDiag: return dqq::launch_bwd_diag(kind, a, l.fuse, s);
    case Family::BwdLane: return dqq::launch_bwd_lane_dense(kind, a, l.lane_mode, s);
    case Family::BwdSmall: return dqq::launch_bwd_small(kind, a, wl, s);
    case Family::BwdChol: return dqq::launch_bwd_dense_wave64(kind, a, wl, s);
    case Family::BwdQcqp: return dqq::launch_bwd_wave_qcqp(a, wl, s);
    case Family::BwdQcqpBig: return dqq::launch_bwd_wave_qcqp_big(a, wl, s);
    case Family::BwdTeam: return dqq::launch_bwd_dense(kind, a, wl, s);
    case Family::BwdAny: return dqq::launch_bwd_any(kind, a, wl, s);
    default: return hipErrorInvalidValue;
    }
}

// Executes a plan: the workspace check, the first launch, the drain behind it.
template <typename Args>
int run(const dqq::Plan& p, int kind, bool backward, Args& a, void* ws, size_t ws_bytes, hipStream_t s)
{
    if (p.err != 0 || p.first.family == dqq::Family::None) return p.err;
    if (p.worklist || p.scratch) {
        // (a signed box backward: any_scratch_bytes sizes kind 3 as kind 2 -- the scratch dqq_scratch_bytes(2, 1, ...) states)
        const size_t scratch = p.scratch ? dqq::any_scratch_bytes(kind, backward, a.N, a.B) : 0;
        if (int rc = check_ws(ws, ws_bytes, a.B, scratch)) return rc;
        if (p.worklist) a.ws = static_cast<int*>(ws);
        if (p.scratch) a.scratch = scratch_of(ws, a.B);
    }
    hipError_t e = launch(p.first, kind, a, false, s);
    if (e != hipSuccess) {
        if (p.first.lane_mode == 2) reset_worklist(ws, s);   // (the lane kernel's report counters live in the header)
        return (int)e;
    }
    if (p.drain.family == dqq::Family::None) return 0;
    e = launch(p.drain, kind, a, true, s);
    if (e != hipSuccess) reset_worklist(ws, s);
    return (int)e;
}

// The forward / backward entry points past their per-kind part (`missing`: a pointer the kind requires is NULL).  The
// forward leaves pdiag_out / diag_flags_out to the fast path when it verifies the batch, else flags every problem 0.
// warm: a.x0 is the start point of every problem (dqq_fwd_warm_f64, plan_fwd_warm); otherwise a.x0 is NULL.
int fwd_call(int kind, bool missing, dqq::FwdArgs& a, int p_layout, void* ws, size_t ws_bytes, void* stream, bool warm = false)
{
    if (int rc = dqq::check_call(kind, a.B, a.N, p_layout)) return rc;
    if (a.B > 0 && missing) return DQQ_E_NULLPTR;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const dqq::Plan p = warm ? dqq::plan_fwd_warm(kind, a.N, a.B, p_layout, knobs()) : dqq::plan_fwd(kind, a.N, a.B, p_layout, knobs());
    a.layout = p_layout & 0xff;
    if (!p.keep) {
        if (a.flags_out != nullptr && a.B > 0) {
            hipError_t e = hipMemsetAsync(a.flags_out, 0, (size_t)a.B, s);
            if (e != hipSuccess) return (int)e;
        }
        a.pdiag_out = nullptr;
        a.flags_out = nullptr;
    }
    return run(p, kind, false, a, ws, ws_bytes, s);
}

int bwd_call(int kind, bool missing, dqq::BwdArgs& a, int p_layout, void* ws, size_t ws_bytes, void* stream)
{
    if (int rc = dqq::check_call(kind, a.B, a.N, p_layout)) return rc;
    if (a.B > 0 && missing) return DQQ_E_NULLPTR;
    a.layout = p_layout & 0xff;
    return run(dqq::plan_bwd(kind, a.N, a.B, p_layout, knobs()), kind, true, a, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

// How many extra inputs a kind has -- a, b, c of dqq_check_f64 / dqq_fwd_warm_f64: none (QP); l_n, mu (QCQP); l_min, l_max (box);
// l_min, l_max, v (signed box) -- and whether one that the kind requires is NULL.
constexpr int kExtras[4] = {0, 2, 2, 3};

bool extras_missing(int kind, const double* a, const double* b, const double* c)
{
    return (kExtras[kind] >= 2 && (a == nullptr || b == nullptr)) || (kExtras[kind] == 3 && c == nullptr);
}

// Every forward entry point: the kernels' arguments and `missing` from (kind, P, q, a, b, c, ...).  warm: dqq_fwd_warm_f64, x0
// required; the per-kind (cold) entry points pass x0 = NULL.  c reaches the kernels as v for the signed box QP only.
int fwd_entry(int kind, bool warm, const double* P, const double* q, const double* a, const double* b, const double* c,
              const double* x0, double* x, int64_t B, int N, double eps, double mu_prox, int max_iter, int adaptive_rho,
              int p_layout, int* iters, double* pdiag_out, unsigned char* diag_flags_out, void* ws, size_t ws_bytes, void* stream)
{
    dqq::FwdArgs args{.P = P, .q = q, .l_n = a, .mu = b, .v = kind == dqq::kKindSignedBox ? c : nullptr, .x = x, .B = (long)B,
                      .N = N, .eps = eps, .mu_prox = mu_prox, .max_iter = max_iter, .adaptive = adaptive_rho ? 1 : 0,
                      .iters = iters, .pdiag_out = pdiag_out, .flags_out = diag_flags_out};
    args.x0 = x0;
    const bool missing = P == nullptr || q == nullptr || x == nullptr || (warm && x0 == nullptr) || extras_missing(kind, a, b, c);
    return fwd_call(kind, missing, args, p_layout, ws, ws_bytes, stream, warm);
}

// Every backward entry point.  ga, gb: grad_l_n, grad_mu / grad_l_min, grad_l_max; report: NULL from the box kinds (they take no
// hint flags, route.cpp).  The signed box QP (c = v) is the box QP backward on the effective bounds of sbox_bounds.h.
int bwd_entry(int kind, const double* P, const double* q, const double* a, const double* b, const double* c, const double* x,
              const double* grad_x, double* gP, double* gq, double* ga, double* gb, double* gamma, double* dgamma, int64_t B, int N,
              double epsilon, int p_layout, int* ir_steps, const double* pdiag, const unsigned char* diag_flags,
              unsigned long long* report, void* ws, size_t ws_bytes, void* stream)
{
    dqq::BwdArgs args{.P = P, .q = q, .l_n = a, .mu = b, .v = kind == dqq::kKindSignedBox ? c : nullptr, .x = x, .grad_x = grad_x,
                      .grad_P = gP, .grad_q = gq, .grad_l_n = ga, .grad_mu = gb, .pdiag = pdiag, .flags = diag_flags,
                      .gamma = gamma, .dgamma = dgamma, .B = (long)B, .N = N, .epsilon = epsilon, .ir_steps = ir_steps,
                      .report = report};
    const bool missing = P == nullptr || q == nullptr || x == nullptr || grad_x == nullptr || extras_missing(kind, a, b, c);
    return bwd_call(kind, missing, args, p_layout, ws, ws_bytes, stream);
}

// The order in which every Newton-family entry, and dqq_jvp_f64 up to its workspace, looks at its arguments (include/diffqcqp_hip.h:
// "DQQ_E_BAD_KIND, then dqq_check_f64's in its order (DQQ_E_BAD_SIZE, DQQ_E_BAD_LAYOUT, DQQ_E_NULLPTR), DQQ_E_UNSUPPORTED_N,
// DQQ_E_WORKSPACE"), stated once:
//   1. err, the plan's: DQQ_E_BAD_KIND first (`kind` indexes nothing before it), then size, layout, reg and max_halvings
//   2. B = 0: 0, nothing is launched
//   3. DQQ_E_NULLPTR, before the N as in the backward: `missing` (a pointer the entry requires is NULL), one of the kind's extras
//      is NULL, or `qp_extras`: the QP has no extras to move (a tangent, gradient or Jacobian of inputs it does not have)
//   4. DQQ_E_UNSUPPORTED_N, the plan's other err
//   5. DQQ_E_WORKSPACE: `workspace` does not hold scratch_bytes (0: the route needs none and `workspace` is not looked at)
// -> go with the scratch (`workspace` itself: no work-list in front of it; NULL for none), or !go with rc, what the entry returns
struct Entered { bool go; int rc; double* scratch; };
Entered enter(int err, int kind, int64_t B, bool missing, const double* a, const double* b, const double* c, bool qp_extras,
              size_t scratch_bytes = 0, void* workspace = nullptr, size_t workspace_bytes = 0)
{
    if ((err != 0 && err != DQQ_E_UNSUPPORTED_N) || B == 0) return {false, err, nullptr};
    if (missing || extras_missing(kind, a, b, c) || qp_extras) return {false, DQQ_E_NULLPTR, nullptr};
    if (err != 0) return {false, err, nullptr};
    if (scratch_bytes != 0 && (workspace == nullptr || workspace_bytes < scratch_bytes)) return {false, DQQ_E_WORKSPACE, nullptr};
    return {true, 0, scratch_bytes != 0 ? static_cast<double*>(workspace) : nullptr};
}

// dqq_polish_reg_f64 (ls NULL) and dqq_polish_ls_f64 past their plans: the entry order, one PolishArgs, the plan's family
int polish_call(const dqq::PolishPlan& p, int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                const double* x, double* x_out, int64_t B, int N, int max_steps, double reg, const dqq::PolishLsOpts* ls,
                double* resid_out, int* steps_out, int* status, void* workspace, size_t workspace_bytes, void* stream,
                double kappa = 0.0)
{
    const Entered e = enter(p.err, kind, B, P == nullptr || q == nullptr || x == nullptr || x_out == nullptr, a, b, c, false,
                            p.scratch ? dqq::polish_scratch_bytes(N, (long)B) : 0, workspace, workspace_bytes);
    if (!e.go) return e.rc;
    const dqq::PolishArgs args{.P = P, .q = q, .a = a, .b = b, .c = c, .x = x, .x_out = x_out, .B = (long)B, .N = N,
                               .max_steps = max_steps, .resid = resid_out, .steps = steps_out, .status = status,
                               .scratch = e.scratch, .inf_bounds = p.inf_bounds ? 1 : 0};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const bool diag = p.route == dqq::NewtonRoute::Diag, any = p.route == dqq::NewtonRoute::Any;
    if (p.smooth) {   // dqq_polish_smooth_f64 with kappa != 0 (ls given): the smoothed families
        const dqq::PolishSmoothOpts sm{reg, kappa, ls->max_halvings, ls->halvings};
        return (int)(diag ? dqq::launch_polish_diag_smooth(kind, args, sm, s) : dqq::launch_polish_dense_smooth(kind, args, sm, any, s));
    }
    if (ls != nullptr)
        return (int)(diag ? dqq::launch_polish_diag_ls(kind, args, *ls, s) : dqq::launch_polish_dense_ls(kind, args, *ls, any, s));
    if (diag) return (int)(p.reg ? dqq::launch_polish_diag_reg(kind, args, reg, s) : dqq::launch_polish_diag(kind, args, s));
    return (int)(p.reg ? dqq::launch_polish_dense_reg(kind, args, reg, any, s) : dqq::launch_polish_dense(kind, args, any, s));
}

// dqq_newton_bwd_reg_f64 / dqq_newton_jvp_reg_f64 past their arguments (`missing`: a pointer the mode requires is NULL)
// kappa (NULL: the entry has none): dqq_newton_bwd_smooth_f64 / dqq_newton_jvp_smooth_f64, plan_newton_smooth's plan
int newton_call(int kind, bool jvp, bool missing, dqq::NewtonArgs& args, int p_layout, double reg, void* workspace,
                size_t workspace_bytes, void* stream, const double* kappa = nullptr)
{
    const dqq::NewtonPlan p = kappa != nullptr ? dqq::plan_newton_smooth(kind, args.N, args.B, p_layout, reg, *kappa)
                                               : dqq::plan_newton_reg(kind, args.N, args.B, p_layout, reg);
    const bool qp_extras =
        kind == dqq::kKindQP && (args.in2 != nullptr || args.in3 != nullptr || args.out2 != nullptr || args.out3 != nullptr);
    const Entered e = enter(p.err, kind, args.B, missing, args.a, args.b, args.c, qp_extras,
                            p.scratch ? dqq::newton_scratch_bytes(args.N, args.B) : 0, workspace, workspace_bytes);
    if (!e.go) return e.rc;
    args.inf_bounds = p.inf_bounds ? 1 : 0;
    args.scratch = e.scratch;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const bool any = p.route == dqq::NewtonRoute::Any;
    if (p.smooth) {   // kappa != 0: the smoothed families
        const dqq::NewtonSmoothOpts sm{reg, *kappa};
        return (int)(p.route == dqq::NewtonRoute::Diag ? dqq::launch_newton_diag_smooth(kind, jvp, args, sm, s)
                                                       : dqq::launch_newton_dense_smooth(kind, jvp, args, sm, any, s));
    }
    if (p.route == dqq::NewtonRoute::Diag)
        return (int)(p.reg ? dqq::launch_newton_diag_reg(kind, jvp, args, reg, s) : dqq::launch_newton_diag(kind, jvp, args, s));
    return (int)(p.reg ? dqq::launch_newton_dense_reg(kind, jvp, args, reg, any, s) : dqq::launch_newton_dense(kind, jvp, args, any, s));
}

} // namespace

extern "C" {

// the pure queries: route.cpp answers them from the rules of the plans
size_t dqq_workspace_bytes(int64_t B) { return dqq::workspace_bytes(B); }

size_t dqq_scratch_bytes(int kind, int pass, int N, int64_t B, int p_layout)
{
    return dqq::scratch_applies(kind, pass, N, B, p_layout) ? dqq::any_scratch_bytes(kind, pass == 1, N, (long)B) : 0;
}

int dqq_hint_flags(int kind, int pass, int N, int64_t B, unsigned long long last_report)
{
    return dqq::hint_flags(kind, pass, N, B, last_report);
}

int dqq_workspace_reset(void* workspace, size_t workspace_bytes, void* stream)
{
    if (workspace == nullptr) return DQQ_E_NULLPTR;
    const size_t head = sizeof(int) * (size_t)dqq::kWsEntries;
    if (workspace_bytes < head) return DQQ_E_WORKSPACE;
    return (int)hipMemsetAsync(workspace, 0, head, static_cast<hipStream_t>(stream));
}

int dqq_workspace_status(const void* workspace, size_t workspace_bytes, void* stream, int* dirty)
{
    if (workspace == nullptr || dirty == nullptr) return DQQ_E_NULLPTR;
    if (workspace_bytes < sizeof(int) * (size_t)dqq::kWsEntries) return DQQ_E_WORKSPACE;
    int word = 0;
    hipError_t e = hipMemcpyAsync(&word, static_cast<const int*>(workspace) + dqq::kWsDirty, sizeof(int),
                                  hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return (int)e;
    *dirty = word != 0 ? 1 : 0;
    return 0;
}

int dqq_max_n(int kind, int p_layout) { return dqq::max_n(kind, ref_order_of(p_layout)); }

const char* dqq_version(void) { return "diffqcqp_hip 0.2.0 gfx950"; }

int dqq_set_option(const char* name, int value)
{
    if (name == nullptr) return DQQ_E_NULLPTR;
    for (auto& o : g_options)
        if (std::strcmp(o.name, name) == 0) { o.slot->store(value); return 0; }
    return DQQ_E_BAD_OPTION;
}

int dqq_device_pointer(void* pinned_host, void** device)
{
    if (pinned_host == nullptr || device == nullptr) return DQQ_E_NULLPTR;
    if ((reinterpret_cast<uintptr_t>(pinned_host) & 7) != 0) return DQQ_E_BAD_SIZE;
    return (int)hipHostGetDevicePointer(device, pinned_host, 0);   // (pinned / registered host memory only)
}

int dqq_get_option(const char* name, int* value)
{
    if (name == nullptr || value == nullptr) return DQQ_E_NULLPTR;
    for (auto& o : g_options)
        if (std::strcmp(o.name, name) == 0) { *value = o.slot->load(); return 0; }
    return DQQ_E_BAD_OPTION;
}

// The per-kind entry points: one statement each over fwd_entry / bwd_entry (no extras: NULL)
#define DQQ_FWD_TAIL B, N, eps, mu_prox, max_iter, adaptive_rho, p_layout, iters, pdiag_out, diag_flags_out, workspace, workspace_bytes, stream
#define DQQ_BWD_TAIL B, N, epsilon, p_layout, ir_steps, pdiag, diag_flags
#define DQQ_WS workspace, workspace_bytes, stream

int dqq_qp_fwd_f64(const double* P, const double* q, double* x, int64_t B, int N, double eps, double mu_prox,
                   int max_iter, int adaptive_rho, int p_layout, int* iters, double* pdiag_out,
                   unsigned char* diag_flags_out, void* workspace, size_t workspace_bytes, void* stream)
{
    return fwd_entry(dqq::kKindQP, false, P, q, nullptr, nullptr, nullptr, nullptr, x, DQQ_FWD_TAIL);
}

int dqq_qcqp_fwd_f64(const double* P, const double* q, const double* l_n, const double* mu, double* x, int64_t B,
                     int N, double eps, double mu_prox, int max_iter, int adaptive_rho, int p_layout, int* iters,
                     double* pdiag_out, unsigned char* diag_flags_out, void* workspace, size_t workspace_bytes,
                     void* stream)
{
    return fwd_entry(dqq::kKindQCQP, false, P, q, l_n, mu, nullptr, nullptr, x, DQQ_FWD_TAIL);
}

int dqq_boxqp_fwd_f64(const double* P, const double* q, const double* l_min, const double* l_max, double* x, int64_t B,
                      int N, double eps, double mu_prox, int max_iter, int adaptive_rho, int p_layout, int* iters,
                      double* pdiag_out, unsigned char* diag_flags_out, void* workspace, size_t workspace_bytes,
                      void* stream)
{
    return fwd_entry(dqq::kKindBox, false, P, q, l_min, l_max, nullptr, nullptr, x, DQQ_FWD_TAIL);
}

int dqq_signedboxqp_fwd_f64(const double* P, const double* q, const double* l_min, const double* l_max,
                            const double* v, double* x, int64_t B, int N, double eps, double mu_prox, int max_iter,
                            int adaptive_rho, int p_layout, int* iters, double* pdiag_out,
                            unsigned char* diag_flags_out, void* workspace, size_t workspace_bytes, void* stream)
{
    return fwd_entry(dqq::kKindSignedBox, false, P, q, l_min, l_max, v, nullptr, x, DQQ_FWD_TAIL);
}

// The warm-started forward of every kind: the cold forward's plan and kernels, entered with the state x0 defines.
int dqq_fwd_warm_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                     const double* x0, double* x, int64_t B, int N, double eps, double mu_prox, int max_iter,
                     int adaptive_rho, int p_layout, int* iters, double* pdiag_out, unsigned char* diag_flags_out,
                     void* workspace, size_t workspace_bytes, void* stream)
{
    return kind < dqq::kKindQP || kind > dqq::kKindSignedBox ? DQQ_E_BAD_KIND
                                                             : fwd_entry(kind, true, P, q, a, b, c, x0, x, DQQ_FWD_TAIL);
}

int dqq_qp_bwd_f64(const double* P, const double* q, const double* x, const double* grad_x, double* grad_P,
                   double* grad_q, int64_t B, int N, double epsilon, int p_layout, int* ir_steps, const double* pdiag,
                   const unsigned char* diag_flags, unsigned long long* report, void* workspace, size_t workspace_bytes,
                   void* stream)
{
    return bwd_entry(dqq::kKindQP, P, q, nullptr, nullptr, nullptr, x, grad_x, grad_P, grad_q, nullptr, nullptr, nullptr, nullptr,
                     DQQ_BWD_TAIL, report, DQQ_WS);
}

int dqq_qcqp_bwd_f64(const double* P, const double* q, const double* l_n, const double* mu, const double* x,
                     const double* grad_x, double* grad_P, double* grad_q, double* grad_l_n, double* grad_mu,
                     double* gamma, double* dgamma, int64_t B, int N, double epsilon, int p_layout, int* ir_steps,
                     const double* pdiag, const unsigned char* diag_flags, unsigned long long* report, void* workspace,
                     size_t workspace_bytes, void* stream)
{
    return bwd_entry(dqq::kKindQCQP, P, q, l_n, mu, nullptr, x, grad_x, grad_P, grad_q, grad_l_n, grad_mu, gamma, dgamma,
                     DQQ_BWD_TAIL, report, DQQ_WS);
}

int dqq_boxqp_bwd_f64(const double* P, const double* q, const double* l_min, const double* l_max, const double* x,
                      const double* grad_x, double* grad_P, double* grad_q, double* grad_l_min, double* grad_l_max,
                      double* gamma, double* dgamma, int64_t B, int N, double epsilon, int p_layout, int* ir_steps,
                      const double* pdiag, const unsigned char* diag_flags, void* workspace, size_t workspace_bytes,
                      void* stream)
{
    return bwd_entry(dqq::kKindBox, P, q, l_min, l_max, nullptr, x, grad_x, grad_P, grad_q, grad_l_min, grad_l_max, gamma, dgamma,
                     DQQ_BWD_TAIL, nullptr, DQQ_WS);
}

int dqq_signedboxqp_bwd_f64(const double* P, const double* q, const double* l_min, const double* l_max, const double* v,
                            const double* x, const double* grad_x, double* grad_P, double* grad_q, double* grad_l_min,
                            double* grad_l_max, double* gamma, double* dgamma, int64_t B, int N, double epsilon, int p_layout,
                            int* ir_steps, const double* pdiag, const unsigned char* diag_flags, void* workspace,
                            size_t workspace_bytes, void* stream)
{
    return bwd_entry(dqq::kKindSignedBox, P, q, l_min, l_max, v, x, grad_x, grad_P, grad_q, grad_l_min, grad_l_max, gamma, dgamma,
                     DQQ_BWD_TAIL, nullptr, DQQ_WS);
}

// The solution check: one launch of check.hip on the caller's stream.  No workspace, no allocation, no synchronisation.
int dqq_check_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                  const double* x, const int* iters, int max_iter, int64_t B, int N, int p_layout, double* resid,
                  int* status, unsigned long long* counts, void* stream)
{
    const dqq::CheckPlan p = dqq::plan_check(kind, N, B, p_layout);   // (DQQ_E_BAD_KIND first: `kind` indexes nothing before it)
    if (p.err != 0 || p.family == dqq::Family::None) return p.err;
    if (P == nullptr || q == nullptr || x == nullptr || extras_missing(kind, a, b, c) || (resid == nullptr && status == nullptr))
        return DQQ_E_NULLPTR;
    const dqq::CheckArgs args{.P = P, .q = q, .a = a, .b = b, .c = c, .x = x, .iters = iters, .max_iter = max_iter,
                              .B = (long)B, .N = N, .resid = resid, .status = status, .counts = counts};
    return (int)dqq::launch_check(kind, args, p.family == dqq::Family::CheckDiag, p.lanes, static_cast<hipStream_t>(stream));
}

// The power-of-two equilibration and its inverse: one launch of equil.hip each on the caller's stream.  No workspace, no
// allocation, no synchronisation; no route: the layout alone says which kernel.  Errors in the order of the header:
// DQQ_E_BAD_KIND, check_call's, B = 0 (nothing is launched), DQQ_E_NULLPTR, DQQ_E_UNSUPPORTED_N, DQQ_E_BAD_LAYOUT for an output
// that overlaps an input.
int dqq_equilibrate_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                        const double* x0, int64_t B, int N, int p_layout, double* P_out, double* q_out, double* a_out,
                        double* b_out, double* c_out, double* x0_out, int32_t* e_out, void* stream)
{
    if (kind < dqq::kKindQP || kind > dqq::kKindSignedBox) return DQQ_E_BAD_KIND;
    if (int rc = dqq::check_call(kind, B, N, p_layout)) return rc;
    if (B == 0) return 0;
    const bool diag = (p_layout & 0xff) == DQQ_P_DIAG;
    double* const ex_out[3] = {a_out, b_out, c_out};
    const double* const ex_in[3] = {a, b, c};
    bool missing = P == nullptr || q == nullptr || P_out == nullptr || q_out == nullptr || e_out == nullptr ||
                   (x0_out != nullptr && x0 == nullptr);
    for (int k = 0; k < 3; ++k)   // an output the kind has no input for, or whose input is NULL
        missing = missing || (ex_out[k] != nullptr && (k >= kExtras[kind] || ex_in[k] == nullptr));
    if (missing) return DQQ_E_NULLPTR;
    if (diag && !(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64)) return DQQ_E_UNSUPPORTED_N;
    // no output may overlap an input: a lane reads the diagonal entries of P, and each array of a problem, more than once
    const size_t vec = sizeof(double) * (size_t)B * (size_t)N, mat = diag ? vec : vec * (size_t)N;
    const size_t ext = kind == dqq::kKindQCQP ? vec / 2 : vec;
    struct Span { const void* p; size_t bytes; };
    const Span in[6] = {{P, mat}, {q, vec}, {a, ext}, {b, ext}, {c, ext}, {x0, vec}};
    const Span out[7] = {{P_out, mat}, {q_out, vec}, {a_out, ext}, {b_out, ext}, {c_out, ext}, {x0_out, vec},
                         {e_out, sizeof(int32_t) * (size_t)B * (size_t)N}};
    for (const Span& o : out)
        for (const Span& i : in) {
            if (o.p == nullptr || i.p == nullptr) continue;
            const uintptr_t ob = reinterpret_cast<uintptr_t>(o.p), ib = reinterpret_cast<uintptr_t>(i.p);
            if (ob < ib + i.bytes && ib < ob + o.bytes) return DQQ_E_BAD_LAYOUT;
        }
    const dqq::EquilArgs args{.P = P, .q = q, .a = a, .b = b, .c = c, .x0 = x0, .P_out = P_out, .q_out = q_out, .a_out = a_out,
                              .b_out = b_out, .c_out = c_out, .x0_out = x0_out, .e_out = e_out, .B = (long)B, .N = N};
    return (int)dqq::launch_equil(kind, args, diag, static_cast<hipStream_t>(stream));
}

int dqq_unscale_f64(const double* y, const int32_t* e, int64_t B, int N, double* x_out, void* stream)
{
    if (B < 0 || N < 1 || B > 0x7fffffffLL) return DQQ_E_BAD_SIZE;
    if (B == 0) return 0;
    if (y == nullptr || e == nullptr || x_out == nullptr) return DQQ_E_NULLPTR;
    return (int)dqq::launch_unscale(y, e, x_out, (long)B * N, static_cast<hipStream_t>(stream));
}

// The forward-mode derivative of every kind: one launch of the plan's family (route.cpp: plan_jvp) on the caller's stream.
int dqq_jvp_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c, const double* x,
                const double* dP, const double* dq, const double* da, const double* db, double* dx, int64_t B, int N,
                double epsilon, int p_layout, int* ir_steps, void* workspace, size_t workspace_bytes, void* stream)
{
    const dqq::JvpPlan p = dqq::plan_jvp(kind, N, B, p_layout);   // (DQQ_E_BAD_KIND first: `kind` indexes nothing before it)
    const Entered e = enter(p.err, kind, B, P == nullptr || q == nullptr || x == nullptr || dx == nullptr, a, b, c,
                            kind == dqq::kKindQP && (da != nullptr || db != nullptr));   // (its scratch is work-list relative: below)
    if (!e.go) return e.rc;
    dqq::JvpArgs args{.P = P, .q = q, .a = a, .b = b, .v = kind == dqq::kKindSignedBox ? c : nullptr, .x = x, .dP = dP, .dq = dq,
                      .da = da, .db = db, .dx = dx, .B = (long)B, .N = N, .epsilon = epsilon, .ir_steps = ir_steps};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.family == dqq::Family::JvpDiag) return (int)dqq::launch_jvp_diag(kind, args, s);
    if (p.family == dqq::Family::JvpTeam) return (int)dqq::launch_jvp_dense(kind, args, s);
    // the backward's global-memory slice behind the work-list (any_scratch_bytes sizes kind 3 as kind 2); the list is not touched
    if (int rc = check_ws(workspace, workspace_bytes, B, dqq::any_scratch_bytes(kind, true, N, (long)B))) return rc;
    args.scratch = scratch_of(workspace, B);
    return (int)dqq::launch_jvp_any(kind, args, s);
}

// The polish of every kind: one launch of the plan's family (route.cpp: plan_polish) on the caller's stream.  `workspace` is
// scratch only (PolishAny): there is no work-list in front of it.
size_t dqq_polish_scratch_bytes(int kind, int N, int64_t B)
{
    const dqq::PolishPlan p = dqq::plan_polish(kind, N, B, DQQ_P_DENSE);
    return p.err == 0 && p.scratch ? dqq::polish_scratch_bytes(N, (long)B) : 0;
}

int dqq_polish_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c, const double* x,
                   double* x_out, int64_t B, int N, int max_steps, int p_layout, double* resid_out, int* steps_out, int* status,
                   void* workspace, size_t workspace_bytes, void* stream)
{
    return dqq_polish_reg_f64(kind, P, q, a, b, c, x, x_out, B, N, max_steps, p_layout, 0.0, resid_out, steps_out, status, workspace,
                              workspace_bytes, stream);
}

// ... with the proximal weight reg on the diagonal of P where M is formed (polish_core.h); reg = 0: the parent's kernels
int dqq_polish_reg_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c, const double* x,
                       double* x_out, int64_t B, int N, int max_steps, int p_layout, double reg, double* resid_out, int* steps_out,
                       int* status, void* workspace, size_t workspace_bytes, void* stream)
{
    return polish_call(dqq::plan_polish_reg(kind, N, B, p_layout, reg), kind, P, q, a, b, c, x, x_out, B, N, max_steps, reg, nullptr,
                       resid_out, steps_out, status, workspace, workspace_bytes, stream);
}

// ... with backtracking on the step length (polish_core.h: polish_problem_ls): the damped polish's own kernels, whatever
// max_halvings is
int dqq_polish_ls_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c, const double* x,
                      double* x_out, int64_t B, int N, int max_steps, int p_layout, double reg, int max_halvings, double* resid_out,
                      int* steps_out, int* status, int32_t* halvings, void* workspace, size_t workspace_bytes, void* stream)
{
    const dqq::PolishLsOpts opts{reg, max_halvings, halvings};
    return polish_call(dqq::plan_polish_ls(kind, N, B, p_layout, reg, max_halvings), kind, P, q, a, b, c, x, x_out, B, N, max_steps, reg,
                       &opts, resid_out, steps_out, status, workspace, workspace_bytes, stream);
}

// ... on the central path (smooth_core.h): F_k = x - PI_k(z) in place of F.  kappa = 0: dqq_polish_ls_f64's kernels
int dqq_polish_smooth_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c, const double* x,
                          double* x_out, int64_t B, int N, int max_steps, int p_layout, double reg, double kappa, int max_halvings,
                          double* resid_out, int* steps_out, int* status, int32_t* halvings, void* workspace, size_t workspace_bytes,
                          void* stream)
{
    const dqq::PolishLsOpts opts{reg, max_halvings, halvings};
    return polish_call(dqq::plan_polish_smooth(kind, N, B, p_layout, reg, max_halvings, kappa), kind, P, q, a, b, c, x, x_out, B, N,
                       max_steps, reg, &opts, resid_out, steps_out, status, workspace, workspace_bytes, stream, kappa);
}

// The polish path (path_core.h): the chain of dqq_polish_smooth_f64 calls over the schedule, bit for bit, in one launch of the
// plan's family (route.cpp: plan_polish_path).  kappas and stage_steps are HOST arrays: the plan reads them, and they travel by
// value in the kernel argument, so the call stays capturable and a replay uses the captured schedule.
int dqq_polish_path_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c, const double* x,
                        double* x_out, int64_t B, int N, int p_layout, double reg, const double* kappas, const int* stage_steps,
                        int n_stages, int max_halvings, double* resid_out, int* steps_out, int* status, int32_t* halvings,
                        double* stage_resid_out, int* stage_steps_out, void* workspace, size_t workspace_bytes, void* stream)
{
    const dqq::PolishPlan p = dqq::plan_polish_path(kind, N, B, p_layout, reg, kappas, stage_steps, n_stages, max_halvings);
    const Entered e = enter(p.err, kind, B, P == nullptr || q == nullptr || x == nullptr || x_out == nullptr, a, b, c, false,
                            p.scratch ? dqq::polish_scratch_bytes(N, (long)B) : 0, workspace, workspace_bytes);
    if (!e.go) return e.rc;
    const dqq::PolishArgs args{.P = P, .q = q, .a = a, .b = b, .c = c, .x = x, .x_out = x_out, .B = (long)B, .N = N,
                               .max_steps = 0, .resid = resid_out, .steps = steps_out, .status = status, .scratch = e.scratch,
                               .inf_bounds = 0};
    dqq::PolishPathOpts o{};
    o.reg = reg;
    for (int s = 0; s < n_stages; ++s) { o.kappa[s] = kappas[s]; o.budget[s] = stage_steps[s]; }
    o.n_stages = n_stages;
    o.max_halvings = max_halvings;
    o.halvings = halvings;
    o.stage_resid = stage_resid_out;
    o.stage_steps = stage_steps_out;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.route == dqq::NewtonRoute::Diag) return (int)dqq::launch_polish_diag_path(kind, args, o, s);
    return (int)dqq::launch_polish_dense_path(kind, args, o, p.route == dqq::NewtonRoute::Any, s);
}

// The Newton derivatives of every kind: one launch of the plan's family (route.cpp: plan_newton) on the caller's stream, the
// same route for both modes (newton_call).  `workspace` is scratch only (NewtonAny): there is no work-list in front of it.
size_t dqq_newton_scratch_bytes(int kind, int N, int64_t B)
{
    const dqq::NewtonPlan p = dqq::plan_newton(kind, N, B, DQQ_P_DENSE);
    return p.err == 0 && p.scratch ? dqq::newton_scratch_bytes(N, (long)B) : 0;
}

int dqq_newton_bwd_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c, const double* x,
                       const double* grad_x, double* grad_P, double* grad_q, double* grad_a, double* grad_b, int64_t B, int N,
                       int p_layout, int* status, void* workspace, size_t workspace_bytes, void* stream)
{
    return dqq_newton_bwd_reg_f64(kind, P, q, a, b, c, x, grad_x, grad_P, grad_q, grad_a, grad_b, B, N, p_layout, 0.0, status, workspace,
                                  workspace_bytes, stream);
}

int dqq_newton_bwd_reg_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                           const double* x, const double* grad_x, double* grad_P, double* grad_q, double* grad_a, double* grad_b,
                           int64_t B, int N, int p_layout, double reg, int* status, void* workspace, size_t workspace_bytes,
                           void* stream)
{
    dqq::NewtonArgs args{.P = P, .q = q, .a = a, .b = b, .c = c, .x = x, .in0 = grad_x, .in1 = nullptr, .in2 = nullptr,
                         .in3 = nullptr, .out0 = grad_P, .out1 = grad_q, .out2 = grad_a, .out3 = grad_b, .B = (long)B, .N = N,
                         .status = status};
    const bool missing = P == nullptr || q == nullptr || x == nullptr || grad_x == nullptr;
    return newton_call(kind, false, missing, args, p_layout, reg, workspace, workspace_bytes, stream);
}

int dqq_newton_jvp_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c, const double* x,
                       const double* dP, const double* dq, const double* da, const double* db, double* dx, int64_t B, int N,
                       int p_layout, int* status, void* workspace, size_t workspace_bytes, void* stream)
{
    return dqq_newton_jvp_reg_f64(kind, P, q, a, b, c, x, dP, dq, da, db, dx, B, N, p_layout, 0.0, status, workspace, workspace_bytes,
                                  stream);
}

int dqq_newton_jvp_reg_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                           const double* x, const double* dP, const double* dq, const double* da, const double* db, double* dx,
                           int64_t B, int N, int p_layout, double reg, int* status, void* workspace, size_t workspace_bytes,
                           void* stream)
{
    dqq::NewtonArgs args{.P = P, .q = q, .a = a, .b = b, .c = c, .x = x, .in0 = dP, .in1 = dq, .in2 = da, .in3 = db, .out0 = dx,
                         .out1 = nullptr, .out2 = nullptr, .out3 = nullptr, .B = (long)B, .N = N, .status = status};
    const bool missing = P == nullptr || q == nullptr || x == nullptr || dx == nullptr;
    return newton_call(kind, true, missing, args, p_layout, reg, workspace, workspace_bytes, stream);
}

// ... on the central path (smooth_core.h): D and E of PI_k.  kappa = 0: the *_reg_f64 entries' kernels
int dqq_newton_bwd_smooth_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                              const double* x, const double* grad_x, double* grad_P, double* grad_q, double* grad_a, double* grad_b,
                              int64_t B, int N, int p_layout, double reg, double kappa, int* status, void* workspace,
                              size_t workspace_bytes, void* stream)
{
    dqq::NewtonArgs args{.P = P, .q = q, .a = a, .b = b, .c = c, .x = x, .in0 = grad_x, .in1 = nullptr, .in2 = nullptr,
                         .in3 = nullptr, .out0 = grad_P, .out1 = grad_q, .out2 = grad_a, .out3 = grad_b, .B = (long)B, .N = N,
                         .status = status};
    const bool missing = P == nullptr || q == nullptr || x == nullptr || grad_x == nullptr;
    return newton_call(kind, false, missing, args, p_layout, reg, workspace, workspace_bytes, stream, &kappa);
}

int dqq_newton_jvp_smooth_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                              const double* x, const double* dP, const double* dq, const double* da, const double* db, double* dx,
                              int64_t B, int N, int p_layout, double reg, double kappa, int* status, void* workspace,
                              size_t workspace_bytes, void* stream)
{
    dqq::NewtonArgs args{.P = P, .q = q, .a = a, .b = b, .c = c, .x = x, .in0 = dP, .in1 = dq, .in2 = da, .in3 = db, .out0 = dx,
                         .out1 = nullptr, .out2 = nullptr, .out3 = nullptr, .B = (long)B, .N = N, .status = status};
    const bool missing = P == nullptr || q == nullptr || x == nullptr || dx == nullptr;
    return newton_call(kind, true, missing, args, p_layout, reg, workspace, workspace_bytes, stream, &kappa);
}

// The Newton Jacobians of every kind: one launch of the plan's family (route.cpp: plan_newton_jac) on the caller's stream.
// `workspace` is scratch only (NewtonJacAny).
size_t dqq_newton_jac_scratch_bytes(int kind, int N, int64_t B)
{
    const dqq::NewtonJacPlan p = dqq::plan_newton_jac(kind, N, B, DQQ_P_DENSE);
    return p.err == 0 && p.scratch ? dqq::newton_jac_scratch_bytes(kind, N, (long)B) : 0;
}

int dqq_newton_jac_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c, const double* x,
                       double* Jq, double* Ja, double* Jb, int64_t B, int N, int p_layout, int* status, void* workspace,
                       size_t workspace_bytes, void* stream)
{
    return dqq_newton_jac_reg_f64(kind, P, q, a, b, c, x, Jq, Ja, Jb, B, N, p_layout, 0.0, status, workspace, workspace_bytes, stream);
}

int dqq_newton_jac_reg_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                           const double* x, double* Jq, double* Ja, double* Jb, int64_t B, int N, int p_layout, double reg,
                           int* status, void* workspace, size_t workspace_bytes, void* stream)
{
    const dqq::NewtonJacPlan p = dqq::plan_newton_jac_reg(kind, N, B, p_layout, reg);
    const Entered e = enter(p.err, kind, B, P == nullptr || q == nullptr || x == nullptr || (Jq == nullptr && Ja == nullptr && Jb == nullptr),
                            a, b, c, kind == dqq::kKindQP && (Ja != nullptr || Jb != nullptr),
                            p.scratch ? dqq::newton_jac_scratch_bytes(kind, N, (long)B) : 0, workspace, workspace_bytes);
    if (!e.go) return e.rc;
    const dqq::NewtonJacArgs args{.P = P, .q = q, .a = a, .b = b, .c = c, .x = x, .Jq = Jq, .Ja = Ja, .Jb = Jb, .B = (long)B, .N = N,
                                  .status = status, .scratch = e.scratch, .inf_bounds = p.inf_bounds ? 1 : 0};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const bool any = p.route == dqq::NewtonRoute::Any;
    if (p.route == dqq::NewtonRoute::Diag)
        return (int)(p.reg ? dqq::launch_newton_jac_diag_reg(kind, args, reg, s) : dqq::launch_newton_jac_diag(kind, args, s));
    return (int)(p.reg ? dqq::launch_newton_jac_dense_reg(kind, args, reg, any, s) : dqq::launch_newton_jac_dense(kind, args, any, s));
}

// ... on the central path (smooth_core.h): D and E of PI_k, every column through one elimination of the smoothed M.  kappa = 0:
// dqq_newton_jac_reg_f64's kernels
int dqq_newton_jac_smooth_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c,
                              const double* x, double* Jq, double* Ja, double* Jb, int64_t B, int N, int p_layout, double reg,
                              double kappa, int* status, void* workspace, size_t workspace_bytes, void* stream)
{
    const dqq::NewtonJacPlan p = dqq::plan_newton_jac_smooth(kind, N, B, p_layout, reg, kappa);
    const Entered e = enter(p.err, kind, B, P == nullptr || q == nullptr || x == nullptr || (Jq == nullptr && Ja == nullptr && Jb == nullptr),
                            a, b, c, kind == dqq::kKindQP && (Ja != nullptr || Jb != nullptr),
                            p.scratch ? dqq::newton_jac_scratch_bytes(kind, N, (long)B) : 0, workspace, workspace_bytes);
    if (!e.go) return e.rc;
    const dqq::NewtonJacArgs args{.P = P, .q = q, .a = a, .b = b, .c = c, .x = x, .Jq = Jq, .Ja = Ja, .Jb = Jb, .B = (long)B, .N = N,
                                  .status = status, .scratch = e.scratch, .inf_bounds = 0};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const bool diag = p.route == dqq::NewtonRoute::Diag, any = p.route == dqq::NewtonRoute::Any;
    if (p.smooth) {   // kappa != 0: the smoothed families
        const dqq::NewtonJacSmoothOpts sm{reg, kappa};
        return (int)(diag ? dqq::launch_newton_jac_diag_smooth(kind, args, sm, s) : dqq::launch_newton_jac_dense_smooth(kind, args, sm, any, s));
    }
    if (diag) return (int)(p.reg ? dqq::launch_newton_jac_diag_reg(kind, args, reg, s) : dqq::launch_newton_jac_diag(kind, args, s));
    return (int)(p.reg ? dqq::launch_newton_jac_dense_reg(kind, args, reg, any, s) : dqq::launch_newton_jac_dense(kind, args, any, s));
}

// The active set, multipliers and kink margin of every kind: one launch of the plan's family (route.cpp: plan_newton_active) on
// the caller's stream.  No family needs scratch: there is no workspace argument.
int dqq_newton_active_f64(int kind, const double* P, const double* q, const double* a, const double* b, const double* c, const double* x,
                          int* state, double* mult, double* margin, int* where, int* status, int64_t B, int N, int p_layout,
                          void* stream)
{
    const dqq::NewtonActivePlan p = dqq::plan_newton_active(kind, N, B, p_layout);
    const bool none = state == nullptr && mult == nullptr && margin == nullptr && where == nullptr && status == nullptr;
    const Entered e = enter(p.err, kind, B, P == nullptr || q == nullptr || x == nullptr || none, a, b, c, false);
    if (!e.go) return e.rc;
    const dqq::ActiveArgs args{.P = P, .q = q, .a = a, .b = b, .c = c, .x = x, .state = state, .mult = mult, .margin = margin,
                               .where = where, .status = status, .B = (long)B, .N = N, .inf_bounds = p.inf_bounds ? 1 : 0};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.route == dqq::NewtonRoute::Diag) return (int)dqq::launch_active_diag(kind, args, s);
    return (int)dqq::launch_active_dense(kind, args, p.route == dqq::NewtonRoute::Any, s);
}

} // extern "C"
