// team_geometry_check.cpp -- TEST ARTEFACT.  team_dense.h and polish_team.h compiled for the host alone (hipcc
// --offload-host-only) behind team_geometry and polish_slice_doubles (tests/test_newton_trip_cases.py).  Nothing here touches a device.
#include "../../diffqcqp_amd/csrc/polish_team.h"

extern "C" {

// out: wpb, lds_bytes, grid
__attribute__((visibility("default"))) void team_geometry_of(long long slice_doubles, int T, long long B, long long* out)
{
    const dqq::TeamGeometry g = dqq::team_geometry((long)slice_doubles, T, (long)B);
    out[0] = g.wpb;
    out[1] = (long long)g.lds_bytes;
    out[2] = g.grid;
}

__attribute__((visibility("default"))) long long polish_slice_doubles_of(int n) { return dqq::polish_slice_doubles(n); }

// the team width dispatch_team picks for N (0: none, N > 64)
__attribute__((visibility("default"))) int team_width_of(int N)
{
    int T = 0;
    (void)dqq::dispatch_team(N,[&](auto t) { T = decltype(t)::value; return hipSuccess; });
    return T;
}

} // extern "C"
