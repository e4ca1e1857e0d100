// polish_ls_route_check.cpp -- TEST ARTEFACT.  route.cpp compiled for the host behind the plan of dqq_polish_ls_f64 and of its
// parent dqq_polish_reg_f64 (tests/test_polish_ls_routes.py).
#include "../../diffqcqp_amd/csrc/route.cpp"

extern "C" {

// parent != 0: plan_polish_reg (max_halvings is not looked at).  out: err, family (route.h: Family), scratch, inf_bounds, reg
__attribute__((visibility("default"))) void polish_ls_plan(int parent, int kind, int N, long long B, int p_layout, double reg,
                                                           int max_halvings, int* out)
{
    const dqq::PolishPlan p = parent ? dqq::plan_polish_reg(kind, N, B, p_layout, reg)
                                     : dqq::plan_polish_ls(kind, N, B, p_layout, reg, max_halvings);
    out[0] = p.err;
    out[1] = (int)p.family;
    out[2] = p.scratch ? 1 : 0;
    out[3] = p.inf_bounds ? 1 : 0;
    out[4] = p.reg ? 1 : 0;
}

// route.h's ordinals of the parent's families and of the damped polish's, in the order diagonal, team, any
__attribute__((visibility("default"))) void polish_ls_families(int* out)
{
    out[0] = (int)dqq::Family::PolishDiag;
    out[1] = (int)dqq::Family::PolishTeam;
    out[2] = (int)dqq::Family::PolishAny;
    out[3] = (int)dqq::Family::PolishLsDiag;
    out[4] = (int)dqq::Family::PolishLsTeam;
    out[5] = (int)dqq::Family::PolishLsAny;
    out[6] = (int)dqq::Family::ActiveAny;   // the last family before them: the earlier ordinals stay what they were
}

} // extern "C"
