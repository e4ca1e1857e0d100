// polish_route_check.cpp -- TEST ARTEFACT.  route.cpp compiled for the host behind plan_polish (tests/test_polish_routes.py).
#include "../../diffqcqp_amd/csrc/route.cpp"

extern "C" {

// out: err, family (route.h: Family), scratch
__attribute__((visibility("default"))) void polish_plan(int kind, int N, long long B, int p_layout, int* out)
{
    const dqq::PolishPlan p = dqq::plan_polish(kind, N, B, p_layout);
    out[0] = p.err;
    out[1] = (int)p.family;
    out[2] = p.scratch ? 1 : 0;
}

// route.h's ordinals of Family::JvpAny (the last family before the polish's) and PolishDiag, PolishTeam, PolishAny
__attribute__((visibility("default"))) void polish_family_ids(int* out)
{
    out[0] = (int)dqq::Family::JvpAny;
    out[1] = (int)dqq::Family::PolishDiag;
    out[2] = (int)dqq::Family::PolishTeam;
    out[3] = (int)dqq::Family::PolishAny;
}

} // extern "C"
