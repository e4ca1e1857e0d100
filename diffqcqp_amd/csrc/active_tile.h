// active_tile.h -- what active_diag.hip and active_dense.hip share on the device: the butterfly of the margin's (value, index)
// pairs over aligned groups of lanes of one wave.  Device only; the definition is active_core.h.
#pragma once

#include "launch.h"
#include "active_core.h"

namespace dqq {

// partner<STEP> (common.h) for an int
template <int STEP>
static DQQ_D int partner_int(int v)
{
    if constexpr (STEP == 1) return __builtin_amdgcn_update_dpp(0, v, kDppXor1, 0xf, 0xf, true);
    else if constexpr (STEP == 2) return __builtin_amdgcn_update_dpp(0, v, kDppXor2, 0xf, 0xf, true);
    else if constexpr (STEP == 4) return __builtin_amdgcn_update_dpp(0, v, kDppHalfMirror, 0xf, 0xf, true);
    else if constexpr (STEP == 8) return __builtin_amdgcn_update_dpp(0, v, kDppRor8, 0xf, 0xf, true);
    else return __shfl_xor(v, STEP, 64);
}

template <int STEP>
static DQQ_D ActiveMin active_min_step(ActiveMin m)
{
    return active_min(m, ActiveMin{partner<STEP>(m.v), partner_int<STEP>(m.i)});
}

// active_min over LANES adjacent lanes (a power of two, aligned): every lane of the group ends with the group's pair.  After a
// step the pair is uniform over the aligned group of 2 STEP lanes -- active_min is symmetric but for which of two equal pairs
// it returns, and equal pairs are the same pair --, which is what partner<> asks for.
template <int LANES>
static DQQ_D ActiveMin active_min_over(ActiveMin m)
{
    if constexpr (LANES >= 2) m = active_min_step<1>(m);
    if constexpr (LANES >= 4) m = active_min_step<2>(m);
    if constexpr (LANES >= 8) m = active_min_step<4>(m);
    if constexpr (LANES >= 16) m = active_min_step<8>(m);
    if constexpr (LANES >= 32) m = active_min_step<16>(m);
    if constexpr (LANES >= 64) m = active_min_step<32>(m);
    return m;
}

} // namespace dqq
