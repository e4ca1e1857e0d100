// diag_tile.h -- the diagonal tile of the Newton family (polish_diag[_ls|_smooth|_path].hip on polish_tile.h, newton_diag[_smooth].hip,
// newton_jac_diag.hip, active_diag.hip; P is the compact diagonal (B,N), N a power of two up to 64), stated once: who owns which
// lane (DiagTile), what a lane reads of its problem and which problems are not admitted (DiagInputs), and the launch
// (launch_diag).  The tile is jvp_diag.hip's: a wave64 owns 128/N consecutive problems, a workgroup of kDiagWPB waves as many
// tiles.  Lane l of the wave belongs to problem l / (N/2) of the tile and owns that problem's coordinate pair -- or contact --
// l % (N/2): every (B,N) vector is one 16-byte access per lane at an even element offset, so a batch slice is a valid argument.
// The lanes of a tile past the end of the batch load nothing and store nothing; a wave whose whole tile lies past the end leaves
// at once (no workgroup barrier is used in these kernels) -- that `if (t.first >= a.B) return;` is a statement of the kernel's
// body, where the compiler keeps it apart from the control flow that follows.  What the lanes of a problem share is decided by a
// ballot masked with the problem's lanes (diag_lane_mask, DiagTile::any): ballots and fences are wave-wide, so the problems of a
// tile never wait for one another.
#pragma once

#include "launch.h"
#include "polish_core.h"

namespace dqq {

constexpr int kDiagWPB = 4;   // waves, and tiles, per workgroup

// the lanes of problem pl of the tile, HL = N/2 lanes each
template <int HL>
static DQQ_D unsigned long long diag_lane_mask(int pl)
{
    return (HL == 64 ? ~0ull : ((1ull << HL) - 1ull)) << (pl * HL);
}

static DQQ_D bool fin2(double2 v) { return __builtin_isfinite(v.x) && __builtin_isfinite(v.y); }

// A lane's place in the tile and in the batch of B.
template <int N, int WPB>
struct DiagTile {
    static_assert(N >= 2 && (N & (N - 1)) == 0 && N <= 64, "N must be a power of two up to 64");
    static constexpr int HL = N / 2;    // lanes per problem
    static constexpr int T = 64 / HL;   // problems per wave tile (T*N == 128)
    int wave, lane;
    long first;                // the tile's first problem
    int pl, j;                 // the lane's problem of the tile, and its coordinate pair / contact of that problem
    bool valid;                // the problem lies inside the batch
    unsigned long long mine;   // the lanes of this problem
    long co, cc;               // element offsets: (B,N), a coordinate pair; (B,N/2), a contact

    DQQ_D explicit DiagTile(long B)
    {
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        lane = threadIdx.x & 63;
        first = ((long)blockIdx.x * WPB + wave) * T;
        const int nvalid = (B - first) < T ? (int)(B - first) : T;
        pl = lane / HL;
        j = lane % HL;
        valid = (unsigned)pl < (unsigned)nvalid;   // a wave that stays has nvalid >= 1: the comparison it had after its early return
        mine = diag_lane_mask<HL>(pl);
        co = first * N + 2 * lane;
        cc = first * HL + lane;
    }
    // a lane's pair of a (B,N) vector / entry of a (B,N/2) one; `other` in the slots past the end of the batch
    DQQ_D double2 load2(const double* p, double2 other) const { return valid ? *reinterpret_cast<const double2*>(p + co) : other; }
    DQQ_D double2 load2(const double* p, double other) const
    {
        return valid ? *reinterpret_cast<const double2*>(p + co) : make_double2(other, other);
    }
    DQQ_D double load1(const double* p, double other) const { return valid ? p[cc] : other; }
    // an optional input: NULL reads as zeros
    DQQ_D double2 load2_opt(const double* p) const
    {
        const double2 zero2 = make_double2(0.0, 0.0);
        return valid && p != nullptr ? *reinterpret_cast<const double2*>(p + co) : zero2;
    }
    DQQ_D double load1_opt(const double* p) const { return valid && p != nullptr ? p[cc] : 0.0; }
    // true on every lane of the problem if f is on one of them
    DQQ_D bool any(bool f) const { return (__ballot(f) & mine) != 0ull; }
};

// What a lane reads of its problem: P's diagonal, q and x of its coordinate pair and the kind's a / b / c (a contact: l_n and
// mu, 1.0 past the end of the batch; the box kinds: l_min, l_max and v, zeros where the kind has none or past the end), and
// `bad`: THIS LANE read an entry that is not admitted -- anything not finite, but for the infinite side of a one-sided box
// where the unit admits them (inf_ok: polish_core.h's polish_lo_bad / polish_hi_bad; false is plain finiteness).  A unit ORs
// its own tests into `bad` (tangents, a cotangent, z) and then makes it the problem's with t.any(bad).  pfill stands for P in
// the slots past the end.  opt: every load takes the NULL-reads-as-zeros form, as the units with optional tangents have it
// for all their inputs.
template <int KIND>
struct DiagInputs {
    double2 pv, qv, xv, av, bv, cv;
    double ln, mc;
    bool bad;

    // (the members are initialised, not assigned: double2's assignment copies by element and splits the 16-byte load)
    template <typename Tile, typename Args>
    DQQ_D DiagInputs(const Tile& t, const Args& a, bool inf_ok, double pfill, bool opt)
        : pv(pfill != 0.0 ? t.load2(a.P, pfill) : get2(t, a.P, false)), qv(get2(t, a.q, opt)), xv(get2(t, a.x, opt)),
          av(KIND >= 2 ? get2(t, a.a, opt) : make_double2(0.0, 0.0)), bv(KIND >= 2 ? get2(t, a.b, opt) : make_double2(0.0, 0.0)),
          cv(KIND == 3 ? get2(t, a.c, opt) : make_double2(0.0, 0.0)), ln(KIND == 1 ? t.load1(a.a, 1.0) : 1.0),
          mc(KIND == 1 ? t.load1(a.b, 1.0) : 1.0)
    {
        bad = !fin2(pv) || !fin2(qv) || !fin2(xv);
        if constexpr (KIND == 1) bad = bad || !__builtin_isfinite(ln) || !__builtin_isfinite(mc);
        if constexpr (KIND >= 2)
            bad = bad || polish_lo_bad(av.x, inf_ok) || polish_lo_bad(av.y, inf_ok) || polish_hi_bad(bv.x, inf_ok) ||
                  polish_hi_bad(bv.y, inf_ok);
        if constexpr (KIND == 3) bad = bad || !fin2(cv);
    }
    template <typename Tile>
    static DQQ_D double2 get2(const Tile& t, const double* p, bool opt)
    {
        return opt ? t.load2_opt(p) : t.load2(p, make_double2(0.0, 0.0));
    }
    // z of the lane's two coordinates at x
    DQQ_D double z0() const { return polish_z(xv.x, polish_acc(0.0, pv.x, xv.x), qv.x); }
    DQQ_D double z1() const { return polish_z(xv.y, polish_acc(0.0, pv.y, xv.y), qv.y); }
};

// The diagonal of P' (polish_core.h: the proximal weight) for the blocks of M.  The *_reg.hip units know at compile time
// that they add (REG; the REG = false units never read `reg`), the others look at reg at run time (polish_reg: 0 adds nothing).
template <bool REG>
static DQQ_D double2 diag_pm_unit(double2 pv, double reg)
{
    if constexpr (REG) return make_double2(polish_reg_add(pv.x, reg), polish_reg_add(pv.y, reg));
    return pv;
}
static DQQ_D double2 diag_pm(double2 pv, double reg) { return make_double2(polish_reg(pv.x, reg), polish_reg(pv.y, reg)); }

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

// The launch of a diagonal unit: kind -> KIND, N -> the instantiated N, one tile per wave.  kernel(k, n) names the
// instantiation for the two integral constants: [](auto k, auto n) { return x_kernel<decltype(k)::value, decltype(n)::value,
// kDiagWPB>; }; args are the kernel's.
template <typename K, typename... Args>
static inline hipError_t launch_diag(int kind, int N, long B, hipStream_t s, K&& kernel, const Args&... args)
{
    return dispatch_kind(kind, [&](auto k) {
        return dispatch_diag_n(N, [&](auto n) {
            return launch(kernel(k, n), dim3(diag_tile_grid<decltype(n)::value, kDiagWPB>(B)), dim3(64 * kDiagWPB), 0, s, args...);
        });
    });
}

} // namespace dqq
