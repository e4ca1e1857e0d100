// path_route_check.cpp -- TEST ARTEFACT.  route.cpp compiled for the host behind the plan of dqq_polish_path_f64 and of the
// smoothed polish it chains, dqq_polish_smooth_f64 (tests/test_path_routes.py).
#include "../../diffqcqp_amd/csrc/route.cpp"

extern "C" {

// smooth != 0: plan_polish_smooth with kappa = kappas[0] (the schedule is not looked at otherwise).  kappas / stage_steps may
// be NULL for the path.  out: err, family (route.h: Family), scratch, inf_bounds, reg, smooth
__attribute__((visibility("default"))) void path_plan(int smooth, int kind, int N, long long B, int p_layout, double reg,
                                                      const double* kappas, const int* stage_steps, int n_stages, int max_halvings,
                                                      int* out)
{
    const dqq::PolishPlan p = smooth ? dqq::plan_polish_smooth(kind, N, B, p_layout, reg, max_halvings, kappas[0])
                                     : dqq::plan_polish_path(kind, N, B, p_layout, reg, kappas, stage_steps, n_stages, max_halvings);
    out[0] = p.err;
    out[1] = (int)p.family;
    out[2] = p.scratch ? 1 : 0;
    out[3] = p.inf_bounds ? 1 : 0;
    out[4] = p.reg ? 1 : 0;
    out[5] = p.smooth ? 1 : 0;
}

// route.h's ordinals of the smoothed polish's families and of the path's, in the order diagonal, team, any; then the last family
// before the path's, and the stage limit
__attribute__((visibility("default"))) void path_families(int* out)
{
    out[0] = (int)dqq::Family::PolishSmoothDiag;
    out[1] = (int)dqq::Family::PolishSmoothTeam;
    out[2] = (int)dqq::Family::PolishSmoothAny;
    out[3] = (int)dqq::Family::PolishPathDiag;
    out[4] = (int)dqq::Family::PolishPathTeam;
    out[5] = (int)dqq::Family::PolishPathAny;
    out[6] = (int)dqq::Family::NewtonSmoothAny;   // the last family before them: the earlier ordinals stay what they were
    out[7] = dqq::kPolishPathMaxStages;
}

} // extern "C"
