// warm_start.h -- the state in which a warm-started forward (dqq_fwd_warm_f64) enters the ADMM loop, for a kernel that holds a
// problem's whole P in one lane (fwd_lane_dense.hip).  Plain host/device code: tests/hostcore/warm_check.cpp checks it on the
// CPU.  The diagonal path's form is in admm_diag_prologue.inc, the team / wave kernels' in their own prologues.
#pragma once

#include "common.h"

namespace dqq {

// l_2 = x0 (as given, not projected), u = -(P x0 + q) with the full P and the row sums in index order -- the mat-vec of the
// kernel's power iteration --, q_prox = q - mu x0.  A NaN or infinite entry of x0 sets `bad` (NaN out, this problem alone).
template <int N>
DQQ_HD void lane_warm_state(const double (&Pm)[N][N], const double (&q)[N], const double (&x0)[N], double mu,
                            double (&qp)[N], double (&l2)[N], double (&u)[N], bool& bad)
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) t += Pm[i][j] * x0[j];
        l2[i] = x0[i];
        u[i] = -(t + q[i]);
        qp[i] = q[i] - mu * x0[i];
        bad = bad || !(x0[i] - x0[i] == 0.0);
    }
}

} // namespace dqq
