// inf_bounds_route_check.cpp -- TEST ARTEFACT.  route.cpp compiled for the host behind every plan, with the plan's inf_bounds
// word where it has one (tests/test_inf_bounds_routes.py).
#include "../../diffqcqp_amd/csrc/route.cpp"

extern "C" {

// entry: 0 polish, 1 newton (backward and JVP: one plan), 2 newton jacobians, 3 forward, 4 warm forward, 5 backward, 6 check,
// 7 reference JVP.  out: err, family (route.h: Family; the first launch's), scratch, inf_bounds (-1: the plan has no such word)
__attribute__((visibility("default"))) void any_plan(int entry, int kind, int N, long long B, int p_layout, int* out)
{
    const dqq::Knobs k{0, -1, 1, 1, 1, 1, 1, 1};
    out[3] = -1;
    if (entry == 0) {
        const dqq::PolishPlan p = dqq::plan_polish(kind, N, B, p_layout);
        out[0] = p.err; out[1] = (int)p.family; out[2] = p.scratch; out[3] = p.inf_bounds;
    } else if (entry == 1) {
        const dqq::NewtonPlan p = dqq::plan_newton(kind, N, B, p_layout);
        out[0] = p.err; out[1] = (int)p.family; out[2] = p.scratch; out[3] = p.inf_bounds;
    } else if (entry == 2) {
        const dqq::NewtonJacPlan p = dqq::plan_newton_jac(kind, N, B, p_layout);
        out[0] = p.err; out[1] = (int)p.family; out[2] = p.scratch; out[3] = p.inf_bounds;
    } else if (entry == 3 || entry == 4 || entry == 5) {
        int err = dqq::check_call(kind, B, N, p_layout);   // (capi.hip: the forwards and backwards check the call, then plan)
        dqq::Plan p;
        if (err == 0) p = entry == 3 ? dqq::plan_fwd(kind, N, B, p_layout, k) : entry == 4 ? dqq::plan_fwd_warm(kind, N, B, p_layout, k)
                                                                                           : dqq::plan_bwd(kind, N, B, p_layout, k);
        out[0] = err != 0 ? err : p.err; out[1] = (int)p.first.family; out[2] = p.scratch;
    } else if (entry == 6) {
        const dqq::CheckPlan p = dqq::plan_check(kind, N, B, p_layout);
        out[0] = p.err; out[1] = (int)p.family; out[2] = 0;
    } else {
        const dqq::JvpPlan p = dqq::plan_jvp(kind, N, B, p_layout);
        out[0] = p.err; out[1] = (int)p.family; out[2] = p.scratch;
    }
}

// route.h's ordinals of the nine families of the Newton entries: polish, newton, jacobians x (diag, team, any)
__attribute__((visibility("default"))) void newton_family_ids(int* out)
{
    const dqq::Family f[9] = {dqq::Family::PolishDiag, dqq::Family::PolishTeam, dqq::Family::PolishAny,
                              dqq::Family::NewtonDiag, dqq::Family::NewtonTeam, dqq::Family::NewtonAny,
                              dqq::Family::NewtonJacDiag, dqq::Family::NewtonJacTeam, dqq::Family::NewtonJacAny};
    for (int i = 0; i < 9; ++i) out[i] = (int)f[i];
}

} // extern "C"
