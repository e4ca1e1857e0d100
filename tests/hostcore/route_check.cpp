// route_check.cpp -- TEST ARTEFACT.  The route plan (diffqcqp_amd/csrc/route.cpp) compiled for the host behind a flat
// extern "C" face, so that tests/test_routes.py can check every route without a GPU.  Nothing in the product links or
// loads this file.
#include "../../diffqcqp_amd/csrc/route.cpp"

extern "C" {

// As capi.hip: check_call, then the plan of a call it accepted.  knobs: the 8 ints of dqq::Knobs in order; out: err, keep,
// worklist, scratch, then per launch (first, drain): family, lpp, fuse, lane_mode, counter -- 14 ints
__attribute__((visibility("default"))) void route_plan(int pass, int kind, int N, long long B, int p_layout,
                                                       const int* knobs, int* out)
{
    const dqq::Knobs k{knobs[0], knobs[1], knobs[2], knobs[3], knobs[4], knobs[5], knobs[6], knobs[7]};
    dqq::Plan p;
    if ((p.err = dqq::check_call(kind, B, N, p_layout)) == 0)
        p = pass == 0 ? dqq::plan_fwd(kind, N, B, p_layout, k) : dqq::plan_bwd(kind, N, B, p_layout, k);
    int* o = out;
    *o++ = p.err;
    *o++ = p.keep;
    *o++ = p.worklist;
    *o++ = p.scratch;
    const dqq::Launch* launches[] = {&p.first, &p.drain};
    for (const dqq::Launch* l : launches) {
        *o++ = (int)l->family;
        *o++ = l->lpp;
        *o++ = l->fuse;
        *o++ = l->lane_mode;
        *o++ = (int)l->counter;
    }
}

// the pure queries behind dqq_hint_flags and dqq_workspace_bytes (capi.hip forwards to the same functions)
__attribute__((visibility("default"))) int route_hint_flags(int kind, int pass, int N, long long B,
                                                            unsigned long long last_report)
{
    return dqq::hint_flags(kind, pass, N, B, last_report);
}

__attribute__((visibility("default"))) unsigned long long route_workspace_bytes(long long B)
{
    return dqq::workspace_bytes(B);
}

__attribute__((visibility("default"))) int route_tuning(void) { return dqq::kTuning ? 1 : 0; }

} // extern "C"
