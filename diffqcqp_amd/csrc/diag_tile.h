// diag_tile.h -- the diagonal tile of the Newton family (polish_diag[_ls].hip, newton_diag.hip, newton_jac_diag.hip,
// active_diag.hip; P is the compact diagonal (B,N), N a power of two up to 64), stated once.  jvp_diag.hip's tile: a wave64 owns
// 128/N consecutive problems, a workgroup of kDiagWPB waves as many tiles.  Lane l of the wave belongs to problem l / (N/2) of
// the tile and owns that problem's coordinate pair -- or contact -- l % (N/2): every (B,N) vector is one 16-byte access per lane at
// an even element offset, so a batch slice is a valid argument.  The lanes of a tile past the end of the batch load nothing and
// store nothing; a wave whose whole tile lies past the end leaves at once (no workgroup barrier is used in these kernels).
// What the lanes of a problem share is decided by a ballot masked with the problem's lanes (diag_lane_mask): ballots and
// fences are wave-wide, so the problems of a tile never wait for one another.
#pragma once

#include "launch.h"

namespace dqq {

constexpr int kDiagWPB = 4;   // waves, and tiles, per workgroup

// the lanes of problem pl of the tile, HL = N/2 lanes each
template <int HL>
static DQQ_D unsigned long long diag_lane_mask(int pl)
{
    return (HL == 64 ? ~0ull : ((1ull << HL) - 1ull)) << (pl * HL);
}

static DQQ_D bool fin2(double2 v) { return __builtin_isfinite(v.x) && __builtin_isfinite(v.y); }

// workgroups of WPB tiles of 128/N problems for a batch of B
template <int N, int WPB>
static inline unsigned diag_tile_grid(long B)
{
    constexpr int T = 128 / N;
    const long ntiles = (B + T - 1) / T;
    const long nblocks = (ntiles + WPB - 1) / WPB;
    return (unsigned)nblocks;
}

// The instantiated N: f(std::integral_constant<int, N>) for N = 2 .. 64, a power of two.
template <typename F>
static inline hipError_t dispatch_diag_n(int N, F&& f)
{
    switch (N) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    default: return hipErrorInvalidValue;
    }
}

} // namespace dqq
