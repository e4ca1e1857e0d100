// check.hip -- the solution check (dqq_check_f64): one streaming pass over a batch's inputs and its x that leaves, per problem,
// a status word and four residual scalars.  It does not know which route solved the problem.  The arithmetic and its order are
// check_core.h (host/device: tests/hostcore/check_core_check.cpp must give the same bits); this file is the lane mapping, the
// loads and the DPP between the lanes of a problem.
//
// L lanes per problem (route.cpp: plan_check; 64 / L problems per wave), W = 2 adjacent columns per lane for even N (one
// 16-byte load per row and lane: DESIGN.md section 2 on why a batch slice keeps that aligned), 1 for odd N (element loads).
// A row of P is read by the L lanes of its problem side by side; for N > 64 W the wave walks the row in chunks of 64 W columns.
// The lane's share of x, q and the kind's extras for the first chunk stays in registers; beyond it (N > 64 W) they are read
// again from global memory (cache hits), so no N needs scratch.  No lane leaves before the last DPP exchange: a DPP read from a
// lane that has left returns 0 (common.h dpp_f64); problems past the end of the batch run on zeros and store nothing.
#include "check_core.h"
#include "launch.h"

namespace dqq {

namespace {

constexpr int kCheckBlock = 256;   // 4 waves
constexpr int kCheckRows = 4;      // rows of P in flight per lane

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

// a lane's view of one problem's coordinate inputs
template <int KIND, int W>
struct CheckIn {
    double x[W], q[W], lo[W], hi[W], sg[W];
    double rad;   // KIND 1, W = 2: the lane's columns are one contact

    DQQ_D void zero()
    {
#pragma unroll
        for (int w = 0; w < W; ++w) x[w] = q[w] = lo[w] = hi[w] = sg[w] = 0.0;
        rad = 0.0;
    }
    // the W coordinates from c on (c a multiple of W, c + W <= N) of problem b
    DQQ_D void load(const CheckArgs& a, long b, int c)
    {
        const long at = b * a.N + c;
        load_w<W>(a.x + at, x);
        load_w<W>(a.q + at, q);
        if constexpr (KIND == 1) {
            const long ct = b * (a.N / 2) + c / 2;   // (B,N/2): element by element
            rad = a.a[ct] * a.b[ct];
        }
        if constexpr (KIND == 2 || KIND == 3) {
            load_w<W>(a.a + at, lo);
            load_w<W>(a.b + at, hi);
        }
        if constexpr (KIND == 3) {
            load_w<W>(a.c + at, sg);
#pragma unroll
            for (int w = 0; w < W; ++w) sg[w] = check_sign(sg[w]);
        }
    }
};

template <int STEP>
DQQ_D void merge_step(CheckAcc& c)
{
    CheckAcc o;
    o.nat = partner<STEP>(c.nat);
    o.inf = partner<STEP>(c.inf);
    o.obj = partner<STEP>(c.obj);
    o.scl = partner<STEP>(c.scl);
    o.xmx = partner<STEP>(c.xmx);
    check_merge(c, o);
}

// the tree over the L lanes of a problem (L wave-uniform: the branches are scalar)
DQQ_D void group_merge(CheckAcc& c, int L)
{
    if (L >= 2) merge_step<1>(c);
    if (L >= 4) merge_step<2>(c);
    if (L >= 8) merge_step<4>(c);
    if (L >= 16) merge_step<8>(c);
    if (L >= 32) merge_step<16>(c);
    if (L >= 64) merge_step<32>(c);
}

template <int STEP, int R>
DQQ_D void sum_step(double (&s)[R], double (&ab)[R])
{
#pragma clang fp contract(off)
    double ps[R], pa[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { ps[r] = partner<STEP>(s[r]); pa[r] = partner<STEP>(ab[r]); }
#pragma unroll
    for (int r = 0; r < R; ++r) { s[r] = s[r] + ps[r]; ab[r] = ab[r] + pa[r]; }
}

template <int R>
DQQ_D void group_sum(double (&s)[R], double (&ab)[R], int L)
{
    if (L >= 2) sum_step<1>(s, ab);
    if (L >= 4) sum_step<2>(s, ab);
    if (L >= 8) sum_step<4>(s, ab);
    if (L >= 16) sum_step<8>(s, ab);
    if (L >= 32) sum_step<16>(s, ab);
    if (L >= 64) sum_step<32>(s, ab);
}

// the lane that leads its problem stores the results; one atomic per wave and status class for the histogram
DQQ_D void check_store(const CheckArgs& a, const CheckAcc& c, long b, bool leader)
{
    int st = 0;
    if (leader) {
        st = check_status(c, a.iters != nullptr, a.iters != nullptr ? a.iters[b] : 0, a.max_iter);
        if (a.resid != nullptr) {
            double* r = a.resid + 4 * b;
            r[0] = c.nat;
            r[1] = c.inf;
            r[2] = c.obj;
            r[3] = c.scl;
        }
        if (a.status != nullptr) a.status[b] = st;
    }
    if (a.counts != nullptr) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned long long m = __ballot(leader && st == k);
            if ((threadIdx.x & 63) == 0 && m != 0ull) atomicAdd(a.counts + k, (unsigned long long)__popcll(m));
        }
    }
}

template <int KIND, int W>
__global__ void __launch_bounds__(kCheckBlock) check_kernel(const CheckArgs a, const int L)
{
    constexpr int R = kCheckRows;
    static_assert(KIND != 1 || W == 2, "a QCQP has even N: a contact per lane");
    const int lane = threadIdx.x & 63, shift = __builtin_ctz(L);
    const long first = ((long)blockIdx.x * (kCheckBlock / 64) + (threadIdx.x >> 6)) << (6 - shift);   // the wave's first problem
    if (first >= a.B) return;   // (the whole wave)
    const long b = first + (lane >> shift);
    const bool valid = b < a.B;
    const int N = a.N, j = lane & (L - 1), span = L * W, c0 = j * W;
    const bool own0 = valid && c0 < N;
    const double* P = a.P + (valid ? b : 0) * (long)N * N;

    CheckIn<KIND, W> in;
    in.zero();
    if (own0) in.load(a, b, c0);
    CheckAcc acc;
    acc.init();

    for (int i0 = 0; i0 < N; i0 += R) {
        double pr[R][W], s[R], ab[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int w = 0; w < W; ++w) pr[r][w] = 0.0;
            if (own0 && i0 + r < N) load_w<W>(P + (long)(i0 + r) * N + c0, pr[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            s[r] = ab[r] = 0.0;
            check_row_terms<W>(pr[r], in.x, s[r], ab[r]);
        }
        for (int cc = span; cc < N; cc += span) {   // N > 64 W: the further chunks of these rows (a uniform loop)
            const int c = cc + c0;
            if (valid && c < N) {
                double xc[W], pc[W];
                load_w<W>(a.x + b * N + c, xc);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (i0 + r < N) {
                        load_w<W>(P + (long)(i0 + r) * N + c, pc);
                        check_row_terms<W>(pc, xc, s[r], ab[r]);
                    }
                }
            }
        }
        group_sum<R>(s, ab, L);
        // the owner of column i takes row i (i0 is a multiple of R, R of W: column i0 + r is the owner's column r mod W)
#pragma unroll
        for (int r = 0; r < R; r += (KIND == 1 ? 2 : 1)) {
            const int i = i0 + r;
            if (valid && i < N && ((i & (span - 1)) >> (W - 1)) == j) {
                if constexpr (KIND == 1) {
                    const double ss[2] = {s[r], s[r + 1]}, aa[2] = {ab[r], ab[r + 1]};
                    if (i < span) {
                        check_contact(acc, in.x, ss, aa, in.q, in.rad);
                    } else {
                        CheckIn<KIND, W> far;
                        far.load(a, b, i);
                        check_contact(acc, far.x, ss, aa, far.q, far.rad);
                    }
                } else if (i < span) {
                    const int w = r & (W - 1);
                    check_coord<KIND>(acc, in.x[w], s[r], ab[r], in.q[w], in.lo[w], in.hi[w], in.sg[w]);
                } else {
                    CheckIn<KIND, 1> far;
                    far.zero();
                    far.load(a, b, i);
                    check_coord<KIND>(acc, far.x[0], s[r], ab[r], far.q[0], far.lo[0], far.hi[0], far.sg[0]);
                }
            }
        }
    }
    group_merge(acc, L);
    check_store(a, acc, b, valid && j == 0);
}

// DQQ_P_DIAG: P is the compact diagonal (B,N); no row tree
template <int KIND, int W>
__global__ void __launch_bounds__(kCheckBlock) check_diag_kernel(const CheckArgs a, const int L)
{
    static_assert(KIND != 1 || W == 2, "a QCQP has even N: a contact per lane");
    const int lane = threadIdx.x & 63, shift = __builtin_ctz(L);
    const long first = ((long)blockIdx.x * (kCheckBlock / 64) + (threadIdx.x >> 6)) << (6 - shift);
    if (first >= a.B) return;
    const long b = first + (lane >> shift);
    const bool valid = b < a.B;
    const int N = a.N, j = lane & (L - 1), span = L * W;
    CheckAcc acc;
    acc.init();
    for (int c = j * W; valid && c < N; c += span) {   // (no DPP inside: lanes may leave this loop one by one)
        CheckIn<KIND, W> in;
        in.zero();
        in.load(a, b, c);
        double p[W], s[W], ab[W];
        load_w<W>(a.P + b * N + c, p);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            s[w] = ab[w] = 0.0;
            const double p1[1] = {p[w]}, x1[1] = {in.x[w]};
            check_row_terms<1>(p1, x1, s[w], ab[w]);
        }
        if constexpr (KIND == 1) {
            check_contact(acc, in.x, s, ab, in.q, in.rad);
        } else {
#pragma unroll
            for (int w = 0; w < W; ++w) check_coord<KIND>(acc, in.x[w], s[w], ab[w], in.q[w], in.lo[w], in.hi[w], in.sg[w]);
        }
    }
    group_merge(acc, L);
    check_store(a, acc, b, valid && j == 0);
}

template <int KIND, int W>
hipError_t launch_kw(const CheckArgs& a, bool diag, int L, hipStream_t s)
{
    const long waves = (a.B + (64 / L) - 1) / (64 / L);
    const dim3 grid((unsigned)((waves + kCheckBlock / 64 - 1) / (kCheckBlock / 64))), block(kCheckBlock);
    return diag ? launch(check_diag_kernel<KIND, W>, grid, block, 0, s, a, L)
                : launch(check_kernel<KIND, W>, grid, block, 0, s, a, L);
}

} // namespace

hipError_t launch_check(int kind, const CheckArgs& a, bool diag, int lanes, hipStream_t s)
{
    const bool even = check_cols_per_lane(a.N) == 2;
    switch (kind) {
    case kKindQP: return even ? launch_kw<0, 2>(a, diag, lanes, s) : launch_kw<0, 1>(a, diag, lanes, s);
    case kKindQCQP: return even ? launch_kw<1, 2>(a, diag, lanes, s) : hipErrorInvalidValue;
    case kKindBox: return even ? launch_kw<2, 2>(a, diag, lanes, s) : launch_kw<2, 1>(a, diag, lanes, s);
    case kKindSignedBox: return even ? launch_kw<3, 2>(a, diag, lanes, s) : launch_kw<3, 1>(a, diag, lanes, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace dqq
