// newton_core_check.cpp -- TEST ARTEFACT.  newton_core.h's newton_jvp_problem / newton_bwd_problem on one CPU thread over a
// batch.  tests/newton_cases.py builds it as a shared library (loaded through ctypes) and, with -DNEWTON_CHECK_MAIN and the
// address and undefined-behaviour sanitizers, as a stand-alone program that tests/test_newton_hostcore.py runs once.
// tests/test_newton_hostcore.py holds it to the numpy restatement bit for bit, tests/test_gpu_newton.py holds the kernels to
// it.  Nothing in the product links or loads this file.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../diffqcqp_amd/csrc/newton_core.h"

using namespace dqq;

namespace {

size_t extras_of(int kind, int n) { return kind == 0 ? 0 : (kind == 1 ? (size_t)n / 2 : (size_t)n); }

const double* at(const double* p, size_t off) { return p != nullptr ? p + off : nullptr; }
double* at(double* p, size_t off) { return p != nullptr ? p + off : nullptr; }

} // namespace

extern "C" {

// P (B n n; diag: B n), q, x (B n), a, b, c: the kind's extras (B ne; c (B n)); tangents as their inputs or NULL; dx (B n)
__attribute__((visibility("default"))) int newton_jvp_batch(int kind, int B, int n, int diag, const double* P, const double* q,
                                                            const double* a, const double* b, const double* c, const double* x,
                                                            const double* dP, const double* dq, const double* da, const double* db,
                                                            double* dx, int* status)
{
    if (kind < 0 || kind > 3 || B < 0 || n < 1) return 2;
    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = extras_of(kind, n);
    std::vector<double> work((size_t)n * n + newton_vec_doubles(n));
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
#define NEWTON_JVP(K) newton_jvp_problem<K>(P + p * np, diag != 0, q + v, at(a, p * ne), at(b, p * ne), at(c, v), x + v, at(dP, p * np), \
                                            at(dq, v), at(da, p * ne), at(db, p * ne), dx + v, n, work.data())
        const int s = kind == 0 ? NEWTON_JVP(0) : kind == 1 ? NEWTON_JVP(1) : kind == 2 ? NEWTON_JVP(2) : NEWTON_JVP(3);
#undef NEWTON_JVP
        if (status != nullptr) status[p] = s;
    }
    return 0;
}

// gx (B n); gP (as P), gq (B n), ga, gb (B ne): each may be NULL
__attribute__((visibility("default"))) int newton_bwd_batch(int kind, int B, int n, int diag, const double* P, const double* q,
                                                            const double* a, const double* b, const double* c, const double* x,
                                                            const double* gx, double* gP, double* gq, double* ga, double* gb,
                                                            int* status)
{
    if (kind < 0 || kind > 3 || B < 0 || n < 1) return 2;
    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = extras_of(kind, n);
    std::vector<double> work((size_t)n * n + newton_vec_doubles(n));
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
#define NEWTON_BWD(K) newton_bwd_problem<K>(P + p * np, diag != 0, q + v, at(a, p * ne), at(b, p * ne), at(c, v), x + v, gx + v, \
                                            at(gP, p * np), at(gq, v), at(ga, p * ne), at(gb, p * ne), n, work.data())
        const int s = kind == 0 ? NEWTON_BWD(0) : kind == 1 ? NEWTON_BWD(1) : kind == 2 ? NEWTON_BWD(2) : NEWTON_BWD(3);
#undef NEWTON_BWD
        if (status != nullptr) status[p] = s;
    }
    return 0;
}

} // extern "C"

#if defined(NEWTON_CHECK_MAIN)
// Every kind, both layouts and both modes on a small fixed batch with active and free coordinates, a NaN problem and a singular
// one; NULL tangents and NULL outputs.  Checks the adjoint identity and the statuses; what it is run for is the sanitizers.
int main()
{
    const int B = 5, n = 6;
    int fails = 0;
    for (int kind = 0; kind < 4; ++kind)
        for (int diag = 0; diag < 2; ++diag) {
            const size_t np = diag ? (size_t)n : (size_t)n * n, ne = extras_of(kind, n);
            std::vector<double> P(B * np), q((size_t)B * n), a(B * ne), b(B * ne), c((size_t)B * n), x((size_t)B * n);
            std::vector<double> dP(B * np), dq((size_t)B * n), da(B * ne), db(B * ne), gx((size_t)B * n);
            unsigned long long r = 12345 + 17 * kind + diag;
            auto rnd = [&]() { r = r * 6364136223846793005ull + 1442695040888963407ull; return (double)(r >> 11) / 9007199254740992.0 - 0.5; };
            for (int p = 0; p < B; ++p) {
                for (int i = 0; i < n; ++i) {
                    if (diag) P[p * np + i] = 1.0 + rnd();
                    else for (int j = 0; j < n; ++j) P[p * np + i * n + j] = (i == j ? 2.0 : 0.0) + 0.2 * rnd();
                    q[p * n + i] = 2.0 * rnd();
                    x[p * n + i] = rnd();
                    c[p * n + i] = rnd();
                    dq[p * n + i] = rnd();
                    gx[p * n + i] = rnd();
                }
                for (size_t i = 0; i < np; ++i) dP[p * np + i] = rnd();
                for (size_t i = 0; i < ne; ++i) {
                    a[p * ne + i] = kind == 1 ? 0.5 + rnd() : -0.3 + 0.2 * rnd();
                    b[p * ne + i] = kind == 1 ? 0.6 : 0.3 + 0.2 * rnd();
                    da[p * ne + i] = rnd();
                    db[p * ne + i] = rnd();
                }
            }
            q[1 * n + 2] = std::nan("");                                       // problem 1: not finite
            for (size_t j = 0; j < (diag ? 1 : (size_t)n); ++j) P[3 * np + (diag ? 0 : j)] = 0.0;   // problem 3: a zero row
            q[3 * n] = -0.01; x[3 * n] = 0.01;                                // ... at a free coordinate (z_0 = 0.02 for every kind)
            if (kind == 1) { a[3 * ne] = 1.0; b[3 * ne] = 1.0; x[3 * n + 1] = 0.0; q[3 * n + 1] = 0.0; if (diag) P[3 * np + 1] = 1.0; }
            if (kind >= 2) { a[3 * ne] = -1.0; b[3 * ne] = 1.0; c[3 * n] = -1.0; }
            const double* pa = ne ? a.data() : nullptr;
            const double* pb = ne ? b.data() : nullptr;
            const double* pc = kind == 3 ? c.data() : nullptr;
            std::vector<double> dx((size_t)B * n), gP(B * np), gq((size_t)B * n), ga(B * ne), gb(B * ne), dx0((size_t)B * n);
            std::vector<int> sj(B), sb(B);
            newton_jvp_batch(kind, B, n, diag, P.data(), q.data(), pa, pb, pc, x.data(), dP.data(), dq.data(), ne ? da.data() : nullptr,
                             ne ? db.data() : nullptr, dx.data(), sj.data());
            newton_bwd_batch(kind, B, n, diag, P.data(), q.data(), pa, pb, pc, x.data(), gx.data(), gP.data(), gq.data(),
                             ne ? ga.data() : nullptr, ne ? gb.data() : nullptr, sb.data());
            newton_jvp_batch(kind, B, n, diag, P.data(), q.data(), pa, pb, pc, x.data(), nullptr, nullptr, nullptr, nullptr, dx0.data(),
                             nullptr);
            newton_bwd_batch(kind, B, n, diag, P.data(), q.data(), pa, pb, pc, x.data(), gx.data(), nullptr, nullptr, nullptr, nullptr,
                             nullptr);
            for (int p = 0; p < B; ++p) {
                const int want = p == 1 ? 2 : (p == 3 ? 1 : 0);
                if (sj[p] != want || sb[p] != want) { printf("kind %d diag %d problem %d: status %d / %d, expected %d\n", kind, diag, p, sj[p], sb[p], want); ++fails; }
                if (want != 0) { if (!std::isnan(dx[p * n]) || !std::isnan(gq[p * n])) { printf("kind %d: outputs of a bad problem are not NaN\n", kind); ++fails; } continue; }
                double lhs = 0.0, rhs = 0.0, mag = 0.0;
                for (int i = 0; i < n; ++i) {
                    lhs += gx[p * n + i] * dx[p * n + i];
                    rhs += gq[p * n + i] * dq[p * n + i];
                    mag += std::fabs(gx[p * n + i] * dx[p * n + i]) + std::fabs(gq[p * n + i] * dq[p * n + i]);
                    if (dx0[p * n + i] != 0.0) { printf("kind %d: a zero tangent moved x\n", kind); ++fails; }
                }
                for (size_t i = 0; i < np; ++i) { rhs += gP[p * np + i] * dP[p * np + i]; mag += std::fabs(gP[p * np + i] * dP[p * np + i]); }
                for (size_t i = 0; i < ne; ++i) {
                    rhs += ga[p * ne + i] * da[p * ne + i] + gb[p * ne + i] * db[p * ne + i];
                    mag += std::fabs(ga[p * ne + i] * da[p * ne + i]) + std::fabs(gb[p * ne + i] * db[p * ne + i]);
                }
                if (!(std::fabs(lhs - rhs) <= 1e-12 * mag)) { printf("kind %d diag %d problem %d: adjoint gap %g\n", kind, diag, p, std::fabs(lhs - rhs) / mag); ++fails; }
            }
        }
    printf("newton_core_check: %d failures\n", fails);
    return fails == 0 ? 0 : 1;
}
#endif
