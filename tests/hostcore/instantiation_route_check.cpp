// instantiation_route_check.cpp -- TEST ARTEFACT.  route.cpp compiled for the host behind the plan of every entry of the Newton
// family, one function for all of them (tests/test_instantiation_cases.py).
#include "../../diffqcqp_amd/csrc/route.cpp"

extern "C" {

// entry: 0 dqq_polish_f64, 1 dqq_polish_reg_f64, 2 dqq_polish_ls_f64, 3 dqq_polish_smooth_f64, 4 dqq_polish_path_f64 (one stage
// of kappa), 5 dqq_newton_{bwd,jvp}_f64, 6 dqq_newton_{bwd,jvp}_reg_f64, 7 dqq_newton_{bwd,jvp}_smooth_f64, 8 dqq_newton_jac_f64,
// 9 dqq_newton_jac_reg_f64, 10 dqq_newton_active_f64.  reg, kappa: not looked at by the entries that take none.
// out: err, family (route.h: Family), route (NewtonRoute: 1 diagonal, 2 team, 3 any-N), reg, smooth
__attribute__((visibility("default"))) void family_plan(int entry, int kind, int N, long long B, int p_layout, double reg, double kappa,
                                                        int* out)
{
    const int steps = 1;
    dqq::NewtonFamilyPlan p;
    switch (entry) {
    case 0: p = dqq::plan_polish(kind, N, B, p_layout); break;
    case 1: p = dqq::plan_polish_reg(kind, N, B, p_layout, reg); break;
    case 2: p = dqq::plan_polish_ls(kind, N, B, p_layout, reg, 8); break;
    case 3: p = dqq::plan_polish_smooth(kind, N, B, p_layout, reg, 8, kappa); break;
    case 4: p = dqq::plan_polish_path(kind, N, B, p_layout, reg, &kappa, &steps, 1, 8); break;
    case 5: p = dqq::plan_newton(kind, N, B, p_layout); break;
    case 6: p = dqq::plan_newton_reg(kind, N, B, p_layout, reg); break;
    case 7: p = dqq::plan_newton_smooth(kind, N, B, p_layout, reg, kappa); break;
    case 8: p = dqq::plan_newton_jac(kind, N, B, p_layout); break;
    case 9: p = dqq::plan_newton_jac_reg(kind, N, B, p_layout, reg); break;
    case 10: p = dqq::plan_newton_active(kind, N, B, p_layout); break;
    default: p.err = -1; break;
    }
    out[0] = p.err;
    out[1] = (int)p.family;
    out[2] = (int)p.route;
    out[3] = p.reg ? 1 : 0;
    out[4] = p.smooth ? 1 : 0;
}

// route.h's ordinals of the first family of each group of three (diagonal, team, any-N), in the order Polish, Newton, NewtonJac,
// Active, PolishLs, PolishSmooth, NewtonSmooth, PolishPath
__attribute__((visibility("default"))) void family_group_ids(int* out)
{
    out[0] = (int)dqq::Family::PolishDiag;
    out[1] = (int)dqq::Family::NewtonDiag;
    out[2] = (int)dqq::Family::NewtonJacDiag;
    out[3] = (int)dqq::Family::ActiveDiag;
    out[4] = (int)dqq::Family::PolishLsDiag;
    out[5] = (int)dqq::Family::PolishSmoothDiag;
    out[6] = (int)dqq::Family::NewtonSmoothDiag;
    out[7] = (int)dqq::Family::PolishPathDiag;
}

} // extern "C"
