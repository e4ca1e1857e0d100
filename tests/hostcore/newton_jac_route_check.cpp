// newton_jac_route_check.cpp -- TEST ARTEFACT.  route.cpp compiled for the host behind plan_newton_jac
// (tests/test_jac_routes.py): as a shared library through ctypes, and with -DNEWTON_JAC_ROUTE_MAIN as a stand-alone program.
#include "../../diffqcqp_amd/csrc/route.cpp"

extern "C" {

// out: err, family (route.h: Family), scratch
__attribute__((visibility("default"))) void newton_jac_plan(int kind, int N, long long B, int p_layout, int* out)
{
    const dqq::NewtonJacPlan p = dqq::plan_newton_jac(kind, N, B, p_layout);
    out[0] = p.err;
    out[1] = (int)p.family;
    out[2] = p.scratch ? 1 : 0;
}

// route.h's ordinals of Family::NewtonAny (the last family before these) and NewtonJacDiag, NewtonJacTeam, NewtonJacAny
__attribute__((visibility("default"))) void newton_jac_family_ids(int* out)
{
    out[0] = (int)dqq::Family::NewtonAny;
    out[1] = (int)dqq::Family::NewtonJacDiag;
    out[2] = (int)dqq::Family::NewtonJacTeam;
    out[3] = (int)dqq::Family::NewtonJacAny;
}

} // extern "C"

#if defined(NEWTON_JAC_ROUTE_MAIN)
#include <cstdio>
#include <initializer_list>
// The table once, on the host alone: the plan is plan_newton's on its own families, whatever the flags and B.
int main()
{
    int fails = 0;
    const int ns[] = {1, 2, 3, 6, 8, 20, 64, 65, 66, 200};
    for (int kind = 0; kind < 4; ++kind)
        for (int N : ns)
            for (int layout = 0; layout < 3; ++layout)
                for (long long B : {0LL, 1LL, 67LL, 1000000LL}) {
                    const dqq::NewtonJacPlan j = dqq::plan_newton_jac(kind, N, B, layout | 0x100);
                    const dqq::NewtonPlan p = dqq::plan_newton(kind, N, B, layout);
                    const int shift = (int)dqq::Family::NewtonJacDiag - (int)dqq::Family::NewtonDiag;
                    const bool same = j.err == p.err && j.scratch == p.scratch &&
                                      (p.family == dqq::Family::None ? j.family == dqq::Family::None
                                                                     : (int)j.family == (int)p.family + shift);
                    if (!same) { printf("kind %d N %d layout %d B %lld: the plans differ\n", kind, N, layout, B); ++fails; }
                }
    if (dqq::plan_newton_jac(4, 8, 1, 0).err != DQQ_E_BAD_KIND || dqq::plan_newton_jac(0, 6, 5, DQQ_P_DIAG).err != DQQ_E_UNSUPPORTED_N) ++fails;
    printf("newton_jac_route_check: %d failures\n", fails);
    return fails == 0 ? 0 : 1;
}
#endif
