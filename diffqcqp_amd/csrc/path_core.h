// path_core.h -- the polish path (dqq_polish_path_f64), host/device and without a lane notion, on top of smooth_core.h.
//
// dqq_polish_path_f64 with stages (kappa_s, steps_s), s = 0 .. S-1, is bit for bit the chain of S calls of dqq_polish_smooth_f64:
// call s has kappa = kappa_s and max_steps = steps_s, all calls share reg and max_halvings, and each call starts from the previous
// call's x_out.  polish_problem_path below IS that chain on one thread -- a loop over the stages around polish_problem_smooth,
// which takes polish_problem_ls's functions where kappa_s == 0 (the run-time branch, not the smoothed formulas at 0) --, so the bits
// of a stage are the parents' by construction.  polish_diag_path.hip and polish_dense_path.hip run the same stages with their own
// thread mappings in one launch -- P loaded once, x kept in registers / the slice between stages -- and must reproduce it bit for
// bit; tests/path_reference.py is the same definition in numpy.
//
// What the path reports besides the stages' own resid and steps (path_status, and the sums below):
//   resid  = (stage 0's r before, stage S-1's r after), each in its own stage's kappa
//   steps  = accepted steps summed over the stages;  halvings = the stages' halvings summed
//   status = 2 if an input entry is not finite or stage 0's r before is not finite; else 0 if any stage accepted a step; else 1
// An input entry that is not finite stops every stage (x_out = x).  A stage whose own r before is not finite accepts nothing, as
// in the chain -- stage 0 included: status stays 2 then, whatever a later stage does from the same x.  kappa_s need not be
// monotone; a stage with steps_s = 0 evaluates its r and moves nothing.
#pragma once

#include "smooth_core.h"

namespace dqq {

// the path's status from stage 0's (polish_status: 2 covers the inputs and stage 0's r before) and the summed steps
DQQ_HD int path_status(int status0, int steps_total) { return status0 == 2 ? 2 : (steps_total > 0 ? 0 : 1); }

// The polish path of one problem.  work: n*n + polish_vec_doubles(n) doubles.  x_out may be x.  stage_resid (2 per stage) and
// stage_steps_out (1 per stage), resid, steps_out and halvings_out are optional.  -> status
template <int KIND>
DQQ_HD int polish_problem_path(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                               const double* x, double* x_out, int n, const double* kappas, const int* stage_steps, int n_stages,
                               int max_halvings, double* resid, int* steps_out, int* halvings_out, double* stage_resid,
                               int* stage_steps_out, double* work, double reg)
{
    const double* from = x;
    double first = 0.0, last = 0.0;
    int steps = 0, halvings = 0, status0 = 1;
    for (int s = 0; s < n_stages; ++s) {
        double rs[2];
        int st = 0, hv = 0;
        const int status = polish_problem_smooth<KIND>(P, diag, q, a, b, c, from, x_out, n, stage_steps[s], max_halvings, rs, &st, &hv,
                                                       work, reg, kappas[s]);
        from = x_out;   // the next call starts from this call's x_out
        if (s == 0) { first = rs[0]; status0 = status; }
        last = rs[1];
        steps += st;
        halvings += hv;
        if (stage_resid != nullptr) { stage_resid[2 * s] = rs[0]; stage_resid[2 * s + 1] = rs[1]; }
        if (stage_steps_out != nullptr) stage_steps_out[s] = st;
    }
    if (resid != nullptr) { resid[0] = first; resid[1] = last; }
    if (steps_out != nullptr) *steps_out = steps;
    if (halvings_out != nullptr) *halvings_out = halvings;
    return path_status(status0, steps);
}

} // namespace dqq
