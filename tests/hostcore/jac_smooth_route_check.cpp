// jac_smooth_route_check.cpp -- TEST ARTEFACT.  route.cpp compiled for the host behind plan_newton_jac_smooth and, beside it,
// plan_newton_jac_reg (tests/test_jac_smooth_routes.py, tests/test_jac_smooth_cases.py), as a shared library through ctypes.
#include "../../diffqcqp_amd/csrc/route.cpp"

extern "C" {

static void put(const dqq::NewtonJacPlan& p, int* out)
{
    out[0] = p.err;
    out[1] = (int)p.family;
    out[2] = (int)p.route;
    out[3] = p.scratch ? 1 : 0;
    out[4] = p.reg ? 1 : 0;
    out[5] = p.smooth ? 1 : 0;
    out[6] = p.inf_bounds ? 1 : 0;
}

// out: err, family (route.h: Family), route (NewtonRoute: 1 diagonal, 2 team, 3 any-N), scratch, reg, smooth, inf_bounds
__attribute__((visibility("default"))) void jac_smooth_plan(int kind, int N, long long B, int p_layout, double reg, double kappa, int* out)
{
    put(dqq::plan_newton_jac_smooth(kind, N, B, p_layout, reg, kappa), out);
}
__attribute__((visibility("default"))) void jac_reg_plan(int kind, int N, long long B, int p_layout, double reg, int* out)
{
    put(dqq::plan_newton_jac_reg(kind, N, B, p_layout, reg), out);
}

// route.h's ordinals: every family that was there before these three, by name, then the three
__attribute__((visibility("default"))) int jac_smooth_family_ids(int* out)
{
    using F = dqq::Family;
    const F all[] = {F::None, F::FwdDiag, F::FwdLane, F::FwdSmall, F::FwdWave64, F::FwdLds, F::FwdAny, F::BwdDiag, F::BwdLane, F::BwdSmall,
                     F::BwdChol, F::BwdQcqp, F::BwdQcqpBig, F::BwdTeam, F::BwdAny, F::Check, F::CheckDiag, F::JvpDiag, F::JvpTeam, F::JvpAny,
                     F::PolishDiag, F::PolishTeam, F::PolishAny, F::NewtonDiag, F::NewtonTeam, F::NewtonAny, F::NewtonJacDiag,
                     F::NewtonJacTeam, F::NewtonJacAny, F::ActiveDiag, F::ActiveTeam, F::ActiveAny, F::PolishLsDiag, F::PolishLsTeam,
                     F::PolishLsAny, F::PolishSmoothDiag, F::PolishSmoothTeam, F::PolishSmoothAny, F::NewtonSmoothDiag,
                     F::NewtonSmoothTeam, F::NewtonSmoothAny, F::PolishPathDiag, F::PolishPathTeam, F::PolishPathAny,
                     F::NewtonJacSmoothDiag, F::NewtonJacSmoothTeam, F::NewtonJacSmoothAny};
    const int n = (int)(sizeof(all) / sizeof(all[0]));
    for (int i = 0; i < n; ++i) out[i] = (int)all[i];
    return n;
}

} // extern "C"
