// fwd_diag_warm.hip -- the diagonal-P fast path of the warm forward (dqq_fwd_warm_f64): the WARM = true instantiations of
// fwd_diag_kernel.h, every lane layout and both the fused and the work-list form.  A translation unit of its own: the cold
// kernels of fwd_diag.hip are compiled, and guarded (tests/test_isa_guard.py), exactly as before.
#include "fwd_diag_kernel.h"

namespace dqq {

hipError_t launch_fwd_diag_warm(int kind, const FwdArgs& a, int lpp, bool fuse, hipStream_t s)
{
    if (a.x0 == nullptr) return hipErrorInvalidValue;
    return launch_fwd_diag_any<true>(kind, a, lpp, fuse, s);
}

} // namespace dqq
