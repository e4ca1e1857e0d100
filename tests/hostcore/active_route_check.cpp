// active_route_check.cpp -- TEST ARTEFACT.  route.cpp compiled for the host behind plan_newton_active
// (tests/test_active_routes.py).
#include "../../diffqcqp_amd/csrc/route.cpp"

extern "C" {

// out: err, family (route.h: Family), inf_bounds
__attribute__((visibility("default"))) void active_plan(int kind, int N, long long B, int p_layout, int* out)
{
    const dqq::NewtonActivePlan p = dqq::plan_newton_active(kind, N, B, p_layout);
    out[0] = p.err;
    out[1] = (int)p.family;
    out[2] = p.inf_bounds ? 1 : 0;
}

// route.h's ordinals of Family::NewtonJacAny (the last family before these) and ActiveDiag, ActiveTeam, ActiveAny
__attribute__((visibility("default"))) void active_family_ids(int* out)
{
    out[0] = (int)dqq::Family::NewtonJacAny;
    out[1] = (int)dqq::Family::ActiveDiag;
    out[2] = (int)dqq::Family::ActiveTeam;
    out[3] = (int)dqq::Family::ActiveAny;
}

} // extern "C"
