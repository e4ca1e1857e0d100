// newton_jac_check.cpp -- TEST ARTEFACT.  newton_core.h's newton_jac_problem on one CPU thread over a batch.  tests/jac_cases.py
// builds it as a shared library (loaded through ctypes) and, with -DNEWTON_JAC_CHECK_MAIN and the address and
// undefined-behaviour sanitizers, as a stand-alone program that tests/test_jac_hostcore.py runs once.
// tests/test_jac_hostcore.py holds it to the numpy restatement bit for bit, tests/test_gpu_jac.py holds the kernels to it.
// Nothing in the product links or loads this file.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../diffqcqp_amd/csrc/newton_core.h"

using namespace dqq;

namespace {

const double* at(const double* p, size_t off) { return p != nullptr ? p + off : nullptr; }
double* at(double* p, size_t off) { return p != nullptr ? p + off : nullptr; }

// doubles per problem of output `which` (0 Jq, 1 Ja, 2 Jb)
size_t out_size(int kind, int n, int diag, int which)
{
    if (diag) return kind == 1 && which == 0 ? 2 * (size_t)n : (size_t)n;
    return (size_t)n * (which == 0 ? n : newton_jac_extra_cols(kind, n));
}

} // namespace

extern "C" {

// P (B n n; diag: B n), q, x (B n), a, b, c: the kind's extras (B ne; c (B n)); Jq, Ja, Jb as include/diffqcqp_hip.h shapes them,
// each may be NULL
__attribute__((visibility("default"))) int newton_jac_batch(int kind, int B, int n, int diag, const double* P, const double* q,
                                                            const double* a, const double* b, const double* c, const double* x,
                                                            double* Jq, double* Ja, double* Jb, int* status)
{
    if (kind < 0 || kind > 3 || B < 0 || n < 1) return 2;
    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = newton_jac_extra_cols(kind, n);
    std::vector<double> work(newton_jac_work_doubles(kind, n));
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
#define NEWTON_JAC(K) newton_jac_problem<K>(P + p * np, diag != 0, q + v, at(a, p * ne), at(b, p * ne), at(c, v), x + v, \
                                            at(Jq, p * out_size(kind, n, diag, 0)), at(Ja, p * out_size(kind, n, diag, 1)), \
                                            at(Jb, p * out_size(kind, n, diag, 2)), n, work.data())
        const int s = kind == 0 ? NEWTON_JAC(0) : kind == 1 ? NEWTON_JAC(1) : kind == 2 ? NEWTON_JAC(2) : NEWTON_JAC(3);
#undef NEWTON_JAC
        if (status != nullptr) status[p] = s;
    }
    return 0;
}

} // extern "C"

#if defined(NEWTON_JAC_CHECK_MAIN)
int newton_jvp_for_check(int kind, int B, int n, int diag, const double* P, const double* q, const double* a, const double* b,
                         const double* c, const double* x, int which, const double* tan, double* dx, int* status);

// Every kind and both layouts on a small fixed batch with active and free coordinates, a NaN problem, an infinite bound and a
// singular problem; each output alone and all together.  Checks every column against newton_jvp_problem with the unit tangent bit
// for bit, the statuses and the NaN rows; what it is run for is the sanitizers.
int main()
{
    const int B = 6, n = 6;
    int fails = 0;
    for (int kind = 0; kind < 4; ++kind)
        for (int diag = 0; diag < 2; ++diag) {
            const size_t np = diag ? (size_t)n : (size_t)n * n, ne = newton_jac_extra_cols(kind, n);
            std::vector<double> P(B * np), q((size_t)B * n), a(B * ne), b(B * ne), c((size_t)B * n), x((size_t)B * n);
            unsigned long long r = 4321 + 17 * kind + diag;
            auto rnd = [&]() { r = r * 6364136223846793005ull + 1442695040888963407ull; return (double)(r >> 11) / 9007199254740992.0 - 0.5; };
            for (int p = 0; p < B; ++p) {
                for (int i = 0; i < n; ++i) {
                    if (diag) P[p * np + i] = 1.0 + rnd();
                    else for (int j = 0; j < n; ++j) P[p * np + i * n + j] = (i == j ? 2.0 : 0.0) + 0.2 * rnd();
                    q[p * n + i] = 2.0 * rnd();
                    x[p * n + i] = rnd();
                    c[p * n + i] = rnd();
                }
                for (size_t i = 0; i < ne; ++i) {
                    a[p * ne + i] = kind == 1 ? 0.5 + rnd() : -0.3 + 0.2 * rnd();
                    b[p * ne + i] = kind == 1 ? 0.6 : 0.3 + 0.2 * rnd();
                }
            }
            q[1 * n + 2] = std::nan("");                                       // problem 1: not finite
            for (size_t j = 0; j < (diag ? 1 : (size_t)n); ++j) P[3 * np + (diag ? 0 : j)] = 0.0;   // problem 3: a zero row
            q[3 * n] = -0.01; x[3 * n] = 0.01;                                // ... at a free coordinate (z_0 = 0.02 for every kind)
            if (kind == 1) { a[3 * ne] = 1.0; b[3 * ne] = 1.0; x[3 * n + 1] = 0.0; q[3 * n + 1] = 0.0; if (diag) P[3 * np + 1] = 1.0; }
            if (kind >= 2) { a[3 * ne] = -1.0; b[3 * ne] = 1.0; c[3 * n] = -1.0; }
            if (kind >= 1) b[4 * ne + 1] = INFINITY;                           // problem 4: an infinite bound / friction coefficient
            const double* pa = ne ? a.data() : nullptr;
            const double* pb = ne ? b.data() : nullptr;
            const double* pc = kind == 3 ? c.data() : nullptr;
            const size_t sz[3] = {out_size(kind, n, diag, 0), out_size(kind, n, diag, 1), out_size(kind, n, diag, 2)};
            std::vector<double> J[3], one[3];
            for (int w = 0; w < 3; ++w) { J[w].assign(B * sz[w], 7.0); one[w].assign(B * sz[w], 7.0); }
            std::vector<int> st(B, -1), st1(B, -1);
            const int nout = kind == 0 ? 1 : 3;
            newton_jac_batch(kind, B, n, diag, P.data(), q.data(), pa, pb, pc, x.data(), J[0].data(), nout > 1 ? J[1].data() : nullptr,
                             nout > 1 ? J[2].data() : nullptr, st.data());
            for (int w = 0; w < nout; ++w) {   // each output alone: the same bits, the same status
                newton_jac_batch(kind, B, n, diag, P.data(), q.data(), pa, pb, pc, x.data(), w == 0 ? one[0].data() : nullptr,
                                 w == 1 ? one[1].data() : nullptr, w == 2 ? one[2].data() : nullptr, st1.data());
                if (std::memcmp(one[w].data(), J[w].data(), sizeof(double) * J[w].size()) != 0 || st1 != st) {
                    printf("kind %d diag %d: output %d alone differs from the full call\n", kind, diag, w); ++fails;
                }
            }
            newton_jac_batch(kind, B, n, diag, P.data(), q.data(), pa, pb, pc, x.data(), J[0].data(), nullptr, nullptr, nullptr);
            std::vector<double> dx((size_t)B * n), tan((size_t)B * n);
            for (int p = 0; p < B; ++p) {
                const int want = p == 1 ? 2 : (p == 3 ? 1 : (p == 4 && kind >= 1 ? 2 : 0));
                if (st[p] != want) { printf("kind %d diag %d problem %d: status %d, expected %d\n", kind, diag, p, st[p], want); ++fails; }
                for (int w = 0; w < nout; ++w)
                    for (size_t i = 0; i < sz[w]; ++i)
                        if ((want != 0) != std::isnan(J[w][p * sz[w] + i])) { printf("kind %d diag %d problem %d: NaN rows are wrong\n", kind, diag, p); ++fails; i = sz[w]; }
            }
            // every column against the JVP of the unit tangent, bit for bit
            for (int w = 0; w < nout; ++w) {
                const int cols = w == 0 ? n : (int)ne;
                for (int j = 0; j < cols; ++j) {
                    std::fill(tan.begin(), tan.end(), 0.0);
                    const size_t tw = w == 0 ? (size_t)n : ne;
                    for (int p = 0; p < B; ++p) tan[p * tw + j] = 1.0;
                    std::vector<int> sj(B);
                    newton_jvp_for_check(kind, B, n, diag, P.data(), q.data(), pa, pb, pc, x.data(), w, tan.data(), dx.data(), sj.data());
                    for (int p = 0; p < B; ++p)
                        for (int i = 0; i < n; ++i) {
                            double got;
                            if (!diag) got = J[w][p * sz[w] + (size_t)i * cols + j];
                            else if (kind == 1) { if (w == 0 ? i / 2 != j / 2 : i / 2 != j) continue; got = w == 0 ? J[0][p * sz[0] + 2 * i + (j & 1)] : J[w][p * sz[w] + i]; }
                            else { if (i != j) continue; got = J[w][p * sz[w] + i]; }
                            const double ref = dx[(size_t)p * n + i];
                            if (std::memcmp(&got, &ref, sizeof(double)) != 0 && !(std::isnan(got) && std::isnan(ref))) {
                                printf("kind %d diag %d problem %d output %d (%d,%d): %a, the JVP gives %a\n", kind, diag, p, w, i, j, got, ref);
                                ++fails;
                            }
                        }
                }
            }
        }
    printf("newton_jac_check: %d failures\n", fails);
    return fails == 0 ? 0 : 1;
}

// newton_jvp_problem over the batch with one tangent (which: 0 dq, 1 da, 2 db) and every other NULL
int newton_jvp_for_check(int kind, int B, int n, int diag, const double* P, const double* q, const double* a, const double* b,
                         const double* c, const double* x, int which, const double* tan, double* dx, int* status)
{
    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = newton_jac_extra_cols(kind, n);
    std::vector<double> work((size_t)n * n + newton_vec_doubles(n));
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
        const double* dq = which == 0 ? tan + v : nullptr;
        const double* da = which == 1 ? tan + p * ne : nullptr;
        const double* db = which == 2 ? tan + p * ne : nullptr;
#define NEWTON_JVP(K) newton_jvp_problem<K>(P + p * np, diag != 0, q + v, at(a, p * ne), at(b, p * ne), at(c, v), x + v, nullptr, dq, da, db, \
                                            dx + v, n, work.data())
        status[p] = kind == 0 ? NEWTON_JVP(0) : kind == 1 ? NEWTON_JVP(1) : kind == 2 ? NEWTON_JVP(2) : NEWTON_JVP(3);
#undef NEWTON_JVP
    }
    return 0;
}
#endif
