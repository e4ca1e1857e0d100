// fwd_diag.hip -- the diagonal-P fast path of the cold forwards: the WARM = false instantiations of fwd_diag_kernel.h.
#include "fwd_diag_kernel.h"

namespace dqq {

hipError_t launch_fwd_diag(int kind, const FwdArgs& a, int lpp, bool fuse, hipStream_t s)
{
    return launch_fwd_diag_any<false>(kind, a, lpp, fuse, s);
}

} // namespace dqq
