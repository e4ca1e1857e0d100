// jvp_route_check.cpp -- TEST ARTEFACT.  route.cpp compiled for the host behind plan_jvp (tests/test_jvp_routes.py).
#include "../../diffqcqp_amd/csrc/route.cpp"

extern "C" {

// out: err, family (route.h: Family), scratch
__attribute__((visibility("default"))) void jvp_plan(int kind, int N, long long B, int p_layout, int* out)
{
    const dqq::JvpPlan p = dqq::plan_jvp(kind, N, B, p_layout);
    out[0] = p.err;
    out[1] = (int)p.family;
    out[2] = p.scratch ? 1 : 0;
}

// route.h's ordinals of Family::JvpDiag, JvpTeam, JvpAny
__attribute__((visibility("default"))) void jvp_family_ids(int* out)
{
    out[0] = (int)dqq::Family::JvpDiag;
    out[1] = (int)dqq::Family::JvpTeam;
    out[2] = (int)dqq::Family::JvpAny;
}

// dqq_scratch_bytes is not 0 for these arguments
__attribute__((visibility("default"))) int jvp_scratch_applies(int kind, int pass, int N, long long B, int p_layout)
{
    return dqq::scratch_applies(kind, pass, N, B, p_layout) ? 1 : 0;
}

} // extern "C"
