// newton_diag_reg.hip -- dqq_newton_bwd_reg_f64 / dqq_newton_jvp_reg_f64 with DQQ_P_DIAG, reg != 0: the REG = true instantiations of newton_diag.hip's
// kernels and their launcher (launch_newton_diag_reg).  One source, two translation units: the parents' instantiations stay the
// code they were, and these differ from them by one add per diagonal entry of P where M is formed (polish_core.h).
#define DQQ_REG_UNIT 1
#include "newton_diag.hip"
