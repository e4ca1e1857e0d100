// reg_core_check.cpp -- TEST ARTEFACT.  The one-thread cores of polish_core.h / newton_core.h with the proximal weight `reg`
// (polish_problem, newton_jvp_problem, newton_bwd_problem, newton_jac_problem) over a batch.  tests/reg_cases.py builds it as a
// shared library (loaded through ctypes) and, with -DREG_CHECK_MAIN and the address and undefined-behaviour sanitizers, as a
// stand-alone program that tests/test_reg_hostcore.py runs once.  tests/test_reg_hostcore.py holds it to the numpy restatement
// tests/reg_reference.py bit for bit, tests/test_gpu_reg.py holds the kernels to it.  Nothing in the product links or loads this
// file.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../diffqcqp_amd/csrc/newton_core.h"

using namespace dqq;

namespace {

size_t extras_of(int kind, int n) { return kind == 0 ? 0 : (kind == 1 ? (size_t)n / 2 : (size_t)n); }

const double* at(const double* p, size_t off) { return p != nullptr ? p + off : nullptr; }
double* at(double* p, size_t off) { return p != nullptr ? p + off : nullptr; }
int* at(int* p, size_t off) { return p != nullptr ? p + off : nullptr; }

#define REG_KIND(CALL) (kind == 0 ? CALL(0) : kind == 1 ? CALL(1) : kind == 2 ? CALL(2) : CALL(3))

} // namespace

extern "C" {

// P (B n n; diag: B n), q, x (B n), a, b, c: the kind's extras (B ne; c (B n)); x_out (B n), resid (B 2), steps, status (B)
__attribute__((visibility("default"))) int reg_polish_batch(int kind, int B, int n, int diag, int inf_ok, double reg, int max_steps,
                                                            const double* P, const double* q, const double* a, const double* b,
                                                            const double* c, const double* x, double* x_out, double* resid,
                                                            int* steps, int* status)
{
    if (kind < 0 || kind > 3 || B < 0 || n < 1) return 2;
    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = extras_of(kind, n);
    std::vector<double> work((size_t)n * n + polish_vec_doubles(n));
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
#define REG_POLISH(K) polish_problem<K>(P + p * np, diag != 0, q + v, at(a, p * ne), at(b, p * ne), at(c, v), x + v, x_out + v, n, \
                                        max_steps, at(resid, 2 * (size_t)p), at(steps, p), work.data(), inf_ok != 0, reg)
        const int s = REG_KIND(REG_POLISH);
#undef REG_POLISH
        if (status != nullptr) status[p] = s;
    }
    return 0;
}

// tangents as their inputs or NULL; dx (B n)
__attribute__((visibility("default"))) int reg_jvp_batch(int kind, int B, int n, int diag, int inf_ok, double reg, const double* P,
                                                         const double* q, const double* a, const double* b, const double* c,
                                                         const double* x, const double* dP, const double* dq, const double* da,
                                                         const double* db, double* dx, int* status)
{
    if (kind < 0 || kind > 3 || B < 0 || n < 1) return 2;
    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = extras_of(kind, n);
    std::vector<double> work((size_t)n * n + newton_vec_doubles(n));
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
#define REG_JVP(K) newton_jvp_problem<K>(P + p * np, diag != 0, q + v, at(a, p * ne), at(b, p * ne), at(c, v), x + v, at(dP, p * np), \
                                         at(dq, v), at(da, p * ne), at(db, p * ne), dx + v, n, work.data(), inf_ok != 0, reg)
        const int s = REG_KIND(REG_JVP);
#undef REG_JVP
        if (status != nullptr) status[p] = s;
    }
    return 0;
}

// gx (B n); gP (as P), gq (B n), ga, gb (B ne): each may be NULL
__attribute__((visibility("default"))) int reg_bwd_batch(int kind, int B, int n, int diag, int inf_ok, double reg, const double* P,
                                                         const double* q, const double* a, const double* b, const double* c,
                                                         const double* x, const double* gx, double* gP, double* gq, double* ga,
                                                         double* gb, int* status)
{
    if (kind < 0 || kind > 3 || B < 0 || n < 1) return 2;
    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = extras_of(kind, n);
    std::vector<double> work((size_t)n * n + newton_vec_doubles(n));
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
#define REG_BWD(K) newton_bwd_problem<K>(P + p * np, diag != 0, q + v, at(a, p * ne), at(b, p * ne), at(c, v), x + v, gx + v, \
                                         at(gP, p * np), at(gq, v), at(ga, p * ne), at(gb, p * ne), n, work.data(), inf_ok != 0, reg)
        const int s = REG_KIND(REG_BWD);
#undef REG_BWD
        if (status != nullptr) status[p] = s;
    }
    return 0;
}

// Jq (B n n; diag: B n, QCQP B n 2), Ja, Jb (B n ne; diag: B n): each may be NULL
__attribute__((visibility("default"))) int reg_jac_batch(int kind, int B, int n, int diag, int inf_ok, double reg, const double* P,
                                                         const double* q, const double* a, const double* b, const double* c,
                                                         const double* x, double* Jq, double* Ja, double* Jb, int* status)
{
    if (kind < 0 || kind > 3 || B < 0 || n < 1) return 2;
    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = extras_of(kind, n);
    const size_t nq = diag ? (kind == 1 ? 2 * (size_t)n : (size_t)n) : (size_t)n * n, nx = diag ? (size_t)n : (size_t)n * ne;
    std::vector<double> work(newton_jac_work_doubles(kind, n));
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
#define REG_JAC(K) newton_jac_problem<K>(P + p * np, diag != 0, q + v, at(a, p * ne), at(b, p * ne), at(c, v), x + v, at(Jq, p * nq), \
                                         at(Ja, p * nx), at(Jb, p * nx), n, work.data(), inf_ok != 0, reg)
        const int s = REG_KIND(REG_JAC);
#undef REG_JAC
        if (status != nullptr) status[p] = s;
    }
    return 0;
}

} // extern "C"

#if defined(REG_CHECK_MAIN)
// Every kind and both layouts on a small batch whose P is singular on free coordinates (a zero matrix; problem 2 a rank-one one),
// through all four cores at reg = 1e-7 and at reg = 0, NULL outputs included.  Checks what the weight is for -- status 0 and
// finite numbers with it, status 1 without -- and the adjoint identity; what it is run for is the sanitizers.
int main()
{
    const int B = 4, n = 6;
    int fails = 0;
    for (int kind = 0; kind < 4; ++kind)
        for (int diag = 0; diag < 2; ++diag) {
            const size_t np = diag ? (size_t)n : (size_t)n * n, ne = extras_of(kind, n);
            std::vector<double> P(B * np, 0.0), q((size_t)B * n), a(B * ne), b(B * ne), c((size_t)B * n), x((size_t)B * n);
            std::vector<double> dq((size_t)B * n), gx((size_t)B * n);
            unsigned long long r = 4711 + 17 * kind + diag;
            auto rnd = [&]() { r = r * 6364136223846793005ull + 1442695040888963407ull; return (double)(r >> 11) / 9007199254740992.0 - 0.5; };
            for (int p = 0; p < B; ++p) {
                for (int i = 0; i < n; ++i) {
                    // x = 0.1 inside every constraint set and q = 0: with P = 0, z = x, every coordinate free, F = 0
                    x[p * n + i] = 0.1;
                    q[p * n + i] = p == 3 ? 0.01 * rnd() : 0.0;   // problem 3: not a solution (and none exists for every kind)
                    c[p * n + i] = -1.0;                          // v < 0: the effective box is [max(l_min, 0), l_max]
                    dq[p * n + i] = rnd();
                    gx[p * n + i] = rnd();
                }
                for (size_t i = 0; i < ne; ++i) {
                    a[p * ne + i] = kind == 1 ? 1.0 : -1.0;
                    b[p * ne + i] = 1.0;
                }
            }
            if (!diag) for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) P[2 * np + i * n + j] = 0.01;   // rank one
            const double* pa = ne ? a.data() : nullptr;
            const double* pb = ne ? b.data() : nullptr;
            const double* pc = kind == 3 ? c.data() : nullptr;
            const size_t nq = diag ? (kind == 1 ? 2 * (size_t)n : (size_t)n) : (size_t)n * n, nx = diag ? (size_t)n : (size_t)n * ne;
            for (int pass = 0; pass < 2; ++pass) {
                const double reg = pass == 0 ? 1e-7 : 0.0;
                std::vector<double> dx((size_t)B * n), gP(B * np), gq((size_t)B * n), ga(B * ne), gb(B * ne), xo((size_t)B * n),
                    resid((size_t)B * 2), Jq(B * nq), Ja(B * nx), Jb(B * nx);
                std::vector<int> sj(B), sb(B), sc(B), sp(B), steps(B);
                reg_jvp_batch(kind, B, n, diag, 0, reg, P.data(), q.data(), pa, pb, pc, x.data(), nullptr, dq.data(), nullptr, nullptr,
                              dx.data(), sj.data());
                reg_bwd_batch(kind, B, n, diag, 0, reg, P.data(), q.data(), pa, pb, pc, x.data(), gx.data(), gP.data(), gq.data(),
                              ne ? ga.data() : nullptr, ne ? gb.data() : nullptr, sb.data());
                reg_bwd_batch(kind, B, n, diag, 0, reg, P.data(), q.data(), pa, pb, pc, x.data(), gx.data(), nullptr, nullptr, nullptr,
                              nullptr, nullptr);
                reg_jac_batch(kind, B, n, diag, 0, reg, P.data(), q.data(), pa, pb, pc, x.data(), Jq.data(), ne ? Ja.data() : nullptr,
                              ne ? Jb.data() : nullptr, sc.data());
                reg_polish_batch(kind, B, n, diag, 0, reg, 4, P.data(), q.data(), pa, pb, pc, x.data(), xo.data(), resid.data(),
                                 steps.data(), sp.data());
                for (int p = 0; p < B; ++p) {
                    const int want = pass == 0 ? 0 : 1;
                    if (sj[p] != want || sb[p] != want || sc[p] != want) {
                        printf("kind %d diag %d reg %g problem %d: status %d / %d / %d, expected %d\n", kind, diag, reg, p, sj[p], sb[p], sc[p], want);
                        ++fails;
                    }
                    if (!(resid[2 * p + 1] <= resid[2 * p])) { printf("kind %d: the polish made problem %d worse\n", kind, p); ++fails; }
                    if (p == 3 && pass == 1 && sp[p] != 1) { printf("kind %d diag %d: a step on a singular M without reg\n", kind, diag); ++fails; }
                    if (pass == 1) continue;
                    double lhs = 0.0, rhs = 0.0, mag = 0.0;
                    for (int i = 0; i < n; ++i) {
                        if (!std::isfinite(dx[p * n + i]) || !std::isfinite(gq[p * n + i])) { printf("kind %d: not finite with reg\n", kind); ++fails; }
                        lhs += gx[p * n + i] * dx[p * n + i];
                        rhs += gq[p * n + i] * dq[p * n + i];
                        mag += std::fabs(gx[p * n + i] * dx[p * n + i]) + std::fabs(gq[p * n + i] * dq[p * n + i]);
                    }
                    if (!(std::fabs(lhs - rhs) <= 1e-12 * mag)) { printf("kind %d diag %d problem %d: adjoint gap %g\n", kind, diag, p, std::fabs(lhs - rhs) / mag); ++fails; }
                }
            }
        }
    printf("reg_core_check: %d failures\n", fails);
    return fails == 0 ? 0 : 1;
}
#endif
