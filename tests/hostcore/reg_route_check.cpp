// reg_route_check.cpp -- TEST ARTEFACT.  route.cpp compiled for the host behind the plans of the *_reg_f64 entries and of their
// parents (tests/test_reg_routes.py).
#include "../../diffqcqp_amd/csrc/route.cpp"

namespace {

template <typename PlanT>
void put(const PlanT& p, int* out)
{
    out[0] = p.err;
    out[1] = (int)p.family;
    out[2] = p.scratch ? 1 : 0;
    out[3] = p.inf_bounds ? 1 : 0;
    out[4] = p.reg ? 1 : 0;
}

} // namespace

extern "C" {

// entry: 0 polish, 1 Newton backward / JVP, 2 Newton Jacobians.  parent != 0: the parent's plan (reg is not looked at).
// out: err, family (route.h: Family), scratch, inf_bounds, reg
__attribute__((visibility("default"))) void reg_plan(int entry, int parent, int kind, int N, long long B, int p_layout, double reg,
                                                     int* out)
{
    if (entry == 0) put(parent ? dqq::plan_polish(kind, N, B, p_layout) : dqq::plan_polish_reg(kind, N, B, p_layout, reg), out);
    else if (entry == 1) put(parent ? dqq::plan_newton(kind, N, B, p_layout) : dqq::plan_newton_reg(kind, N, B, p_layout, reg), out);
    else put(parent ? dqq::plan_newton_jac(kind, N, B, p_layout) : dqq::plan_newton_jac_reg(kind, N, B, p_layout, reg), out);
}

} // extern "C"
