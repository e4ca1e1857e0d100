// newton_route_check.cpp -- TEST ARTEFACT.  route.cpp compiled for the host behind plan_newton (tests/test_newton_routes.py).
#include "../../diffqcqp_amd/csrc/route.cpp"

extern "C" {

// out: err, family (route.h: Family), scratch
__attribute__((visibility("default"))) void newton_plan(int kind, int N, long long B, int p_layout, int* out)
{
    const dqq::NewtonPlan p = dqq::plan_newton(kind, N, B, p_layout);
    out[0] = p.err;
    out[1] = (int)p.family;
    out[2] = p.scratch ? 1 : 0;
}

// route.h's ordinals of Family::PolishAny (the last family before these) and NewtonDiag, NewtonTeam, NewtonAny
__attribute__((visibility("default"))) void newton_family_ids(int* out)
{
    out[0] = (int)dqq::Family::PolishAny;
    out[1] = (int)dqq::Family::NewtonDiag;
    out[2] = (int)dqq::Family::NewtonTeam;
    out[3] = (int)dqq::Family::NewtonAny;
}

} // extern "C"
