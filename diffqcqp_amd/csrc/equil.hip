// equil.hip -- the power-of-two equilibration (dqq_equilibrate_f64) and its inverse on a solution (dqq_unscale_f64): streaming
// kernels that know no route.  The arithmetic is equil_core.h (host/device: tests/hostcore/equil_core_check.cpp must give the
// same bits); this file is the lane mapping and the loads.
//
// (B,N,N): check.hip's mapping -- L lanes per problem (route.h: check_lanes; 64 / L problems per wave), W = 2 adjacent columns
// per lane for even N (one 16-byte load and store per row and lane), 1 for odd N; for N > 64 W the lanes walk a row in chunks of
// 64 W columns.  A lane first takes the exponents of its own columns from the diagonal (a gather of N entries per problem, out
// of cache lines the row loop reads right after) and scales its share of q, the extras and x0 with them; then the rows: the
// exponent of row i comes from P_ii again, one address for the L lanes of the problem, inside the row that is being loaded.
// Every entry of P is read and written once by the lane that owns its column.  Nothing is exchanged between lanes: a lane
// past the end of the batch leaves at once.
// DQQ_P_DIAG and dqq_unscale_f64: elementwise over the flat arrays, a grid-stride loop.
#include "equil_core.h"
#include "launch.h"

namespace dqq {

namespace {

constexpr int kEquilBlock = 256;   // 4 waves
constexpr int kEquilRows = 4;      // rows of P in flight per lane
constexpr long kEquilMaxGrid = 1L << 20;   // the flat kernels' grid: beyond it the threads loop

template <int W>
DQQ_D void load_w(const double* p, double (&v)[W])
{
    if constexpr (W == 2) {
        const double2 t = *reinterpret_cast<const double2*>(p);
        v[0] = t.x;
        v[1] = t.y;
    } else {
        v[0] = p[0];
    }
}

template <int W>
DQQ_D void store_w(double* p, const double (&v)[W])
{
    if constexpr (W == 2) *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
    else p[0] = v[0];
}

// the W coordinates from c on (c a multiple of W, c + W <= N) of problem b: e_out, q and whatever else has an output
template <int KIND, int W>
DQQ_D void scale_coords(const EquilArgs& a, long b, int c, const int (&e)[W])
{
    const long at = b * a.N + c;
    double v[W];
#pragma unroll
    for (int w = 0; w < W; ++w) a.e_out[at + w] = e[w];
    load_w<W>(a.q + at, v);
#pragma unroll
    for (int w = 0; w < W; ++w) v[w] = equil_scale_q(v[w], e[w]);
    store_w<W>(a.q_out + at, v);
    if (a.x0_out != nullptr) {
        load_w<W>(a.x0 + at, v);
#pragma unroll
        for (int w = 0; w < W; ++w) v[w] = equil_scale_bound(v[w], e[w]);
        store_w<W>(a.x0_out + at, v);
    }
    if constexpr (KIND == 1) {   // (W = 2: the lane's columns are one contact, e[0] == e[1])
        const long ct = b * (a.N / 2) + c / 2;
        if (a.a_out != nullptr) a.a_out[ct] = equil_scale_bound(a.a[ct], e[0]);
        if (a.b_out != nullptr) a.b_out[ct] = a.b[ct];
    }
    if constexpr (KIND == 2 || KIND == 3) {
        if (a.a_out != nullptr) {
            load_w<W>(a.a + at, v);
#pragma unroll
            for (int w = 0; w < W; ++w) v[w] = equil_scale_bound(v[w], e[w]);
            store_w<W>(a.a_out + at, v);
        }
        if (a.b_out != nullptr) {
            load_w<W>(a.b + at, v);
#pragma unroll
            for (int w = 0; w < W; ++w) v[w] = equil_scale_bound(v[w], e[w]);
            store_w<W>(a.b_out + at, v);
        }
    }
    if constexpr (KIND == 3) {
        if (a.c_out != nullptr) {
            load_w<W>(a.c + at, v);
            store_w<W>(a.c_out + at, v);
        }
    }
}

template <int KIND, int W>
__global__ void __launch_bounds__(kEquilBlock) equil_kernel(const EquilArgs a, const int L)
{
    constexpr int R = kEquilRows;
    static_assert(KIND != 1 || W == 2, "a QCQP has even N: a contact per lane");
    const int lane = threadIdx.x & 63, shift = __builtin_ctz(L);
    const long first = ((long)blockIdx.x * (kEquilBlock / 64) + (threadIdx.x >> 6)) << (6 - shift);   // the wave's first problem
    const long b = first + (lane >> shift);
    const int N = a.N, j = lane & (L - 1), span = L * W, c0 = j * W;
    if (b >= a.B || c0 >= N) return;   // (c0 < N: N is a multiple of W, so c0 + W <= N)
    const double* P = a.P + b * (long)N * N;
    double* Po = a.P_out + b * (long)N * N;
    const auto diag = [P, N](int i) { return P[(long)i * N + i]; };

    int e0[W];   // the exponents of the lane's first chunk stay in registers
    for (int c = c0; c < N; c += span) {
        int e[W];
#pragma unroll
        for (int w = 0; w < W; ++w) e[w] = equil_coord_exp<KIND>(diag, c + w);
        if (c == c0) {
#pragma unroll
            for (int w = 0; w < W; ++w) e0[w] = e[w];
        }
        scale_coords<KIND, W>(a, b, c, e);
    }

    for (int i0 = 0; i0 < N; i0 += R) {
        double pr[R][W];
        int er[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            er[r] = 0;
            if (i0 + r < N) {
                load_w<W>(P + (long)(i0 + r) * N + c0, pr[r]);
                er[r] = equil_coord_exp<KIND>(diag, i0 + r);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (i0 + r < N) {
#pragma unroll
                for (int w = 0; w < W; ++w) pr[r][w] = equil_scale_p(pr[r][w], er[r], e0[w]);
                store_w<W>(Po + (long)(i0 + r) * N + c0, pr[r]);
            }
        }
        for (int c = c0 + span; c < N; c += span) {   // N > 64 W: the further chunks of these rows
            int e[W];
#pragma unroll
            for (int w = 0; w < W; ++w) e[w] = equil_coord_exp<KIND>(diag, c + w);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (i0 + r < N) {
                    double pc[W];
                    load_w<W>(P + (long)(i0 + r) * N + c, pc);
#pragma unroll
                    for (int w = 0; w < W; ++w) pc[w] = equil_scale_p(pc[w], er[r], e[w]);
                    store_w<W>(Po + (long)(i0 + r) * N + c, pc);
                }
            }
        }
    }
}

// DQQ_P_DIAG: P is the compact diagonal (B,N), N even: a thread per pair of coordinates of the flat (B N) arrays -- a pair never
// straddles two problems, and a QCQP's pair is a contact
template <int KIND>
__global__ void __launch_bounds__(kEquilBlock) equil_diag_kernel(const EquilArgs a)
{
    const long pairs = a.B * (long)(a.N / 2), step = (long)gridDim.x * kEquilBlock;
    for (long t = (long)blockIdx.x * kEquilBlock + threadIdx.x; t < pairs; t += step) {
        const long b = (2 * t) / a.N;
        const int c = (int)(2 * t - b * a.N);
        double p[2];
        load_w<2>(a.P + 2 * t, p);
        const auto diag = [&p, c](int i) { return p[i - c]; };
        const int e[2] = {equil_coord_exp<KIND>(diag, c), equil_coord_exp<KIND>(diag, c + 1)};
        p[0] = equil_scale_p(p[0], e[0], e[0]);
        p[1] = equil_scale_p(p[1], e[1], e[1]);
        store_w<2>(a.P_out + 2 * t, p);
        scale_coords<KIND, 2>(a, b, c, e);
    }
}

__global__ void __launch_bounds__(kEquilBlock) unscale_kernel(const double* y, const int* e, double* x, long n)
{
    const long step = (long)gridDim.x * kEquilBlock;
    for (long t = (long)blockIdx.x * kEquilBlock + threadIdx.x; t < n; t += step) x[t] = equil_unscale(y[t], e[t]);
}

unsigned flat_grid(long threads)
{
    const long blocks = (threads + kEquilBlock - 1) / kEquilBlock;
    return (unsigned)(blocks < kEquilMaxGrid ? blocks : kEquilMaxGrid);
}

template <int KIND, int W>
hipError_t launch_kw(const EquilArgs& a, int L, hipStream_t s)
{
    const long waves = (a.B + (64 / L) - 1) / (64 / L);
    const dim3 grid((unsigned)((waves + kEquilBlock / 64 - 1) / (kEquilBlock / 64))), block(kEquilBlock);
    return launch(equil_kernel<KIND, W>, grid, block, 0, s, a, L);
}

} // namespace

hipError_t launch_equil(int kind, const EquilArgs& a, bool diag, hipStream_t s)
{
    if (diag) {   // (N even: the entry admits N in {2, 4, 8, 16, 32, 64} only)
        const dim3 grid(flat_grid(a.B * (long)(a.N / 2))), block(kEquilBlock);
        return dispatch_kind(kind, [&](auto k) { return launch(equil_diag_kernel<decltype(k)::value>, grid, block, 0, s, a); });
    }
    const int L = check_lanes(a.N);
    const bool even = check_cols_per_lane(a.N) == 2;
    switch (kind) {
    case kKindQP: return even ? launch_kw<0, 2>(a, L, s) : launch_kw<0, 1>(a, L, s);
    case kKindQCQP: return even ? launch_kw<1, 2>(a, L, s) : hipErrorInvalidValue;
    case kKindBox: return even ? launch_kw<2, 2>(a, L, s) : launch_kw<2, 1>(a, L, s);
    case kKindSignedBox: return even ? launch_kw<3, 2>(a, L, s) : launch_kw<3, 1>(a, L, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_unscale(const double* y, const int* e, double* x, long n, hipStream_t s)
{
    const dim3 grid(flat_grid(n)), block(kEquilBlock);
    return launch(unscale_kernel, grid, block, 0, s, y, e, x, n);
}

} // namespace dqq
