// polish_ls_core_check.cpp -- TEST ARTEFACT.  A stand-alone program: polish_core.h's polish_problem_ls (the damped polish,
// dqq_polish_ls_f64) on one CPU thread over a batch read from a file, the results written to another.  tests/polish_ls_cases.py
// builds it (plain, and with the address and undefined-behaviour sanitizers) and runs it; tests/test_polish_ls_hostcore.py holds it
// to the numpy restatement bit for bit, tests/test_gpu_polish_ls.py holds the kernels to it.  Nothing in the product links or
// loads this file.
//
// Input:  int32 kind, B, n, diag, max_steps, in_place, max_halvings, inf_ok; float64 reg; then float64 P (B n n, or B n if
//         diag), q (B n), a, b, c (as many entries as the kind has: QCQP B n/2 each; box B n each; signed box also c), x (B n).
// Output: float64 x_out (B n), resid (B 2); int32 steps (B), status (B), halvings (B).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../diffqcqp_amd/csrc/polish_core.h"

using namespace dqq;

namespace {

bool read_all(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

struct Call {
    const double *P, *q, *a, *b, *c, *x;
    double* x_out;
    int n, max_steps, max_halvings;
    double* resid;
    int *steps, *halvings;
    double* work;
    bool diag, inf_ok;
    double reg;
};

template <int KIND>
int run(const Call& k)
{
    return polish_problem_ls<KIND>(k.P, k.diag, k.q, k.a, k.b, k.c, k.x, k.x_out, k.n, k.max_steps, k.max_halvings, k.resid, k.steps,
                                   k.halvings, k.work, k.inf_ok, k.reg);
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (f == nullptr) return 2;
    int h[8];
    double reg = 0.0;
    if (!read_all(f, h, sizeof h) || !read_all(f, &reg, sizeof reg)) return 2;
    const int kind = h[0], B = h[1], n = h[2], diag = h[3], max_steps = h[4], in_place = h[5], max_halvings = h[6], inf_ok = h[7];
    if (kind < 0 || kind > 3 || B < 0 || n < 1 || max_halvings < 0) return 2;
    const size_t np = diag ? (size_t)n : (size_t)n * n;
    const size_t ne = kind == 0 ? 0 : (kind == 1 ? (size_t)n / 2 : (size_t)n);
    std::vector<double> P(B * np), q((size_t)B * n), a(B * ne), b(B * ne), c(kind == 3 ? (size_t)B * n : 0), x((size_t)B * n);
    bool ok = read_all(f, P.data(), P.size() * 8) && read_all(f, q.data(), q.size() * 8) && read_all(f, a.data(), a.size() * 8) &&
              read_all(f, b.data(), b.size() * 8) && read_all(f, c.data(), c.size() * 8) && read_all(f, x.data(), x.size() * 8);
    fclose(f);
    if (!ok) return 2;
    std::vector<double> xo((size_t)B * n), resid((size_t)B * 2), work((size_t)n * n + polish_vec_doubles(n));
    std::vector<int> steps(B), status(B), halvings(B);
    if (in_place) xo = x;
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
        const Call k{P.data() + p * np, q.data() + v, ne ? a.data() + p * ne : nullptr, ne ? b.data() + p * ne : nullptr,
                     kind == 3 ? c.data() + v : nullptr, in_place ? xo.data() + v : x.data() + v, xo.data() + v, n, max_steps,
                     max_halvings, resid.data() + 2 * (size_t)p, &steps[p], &halvings[p], work.data(), diag != 0, inf_ok != 0, reg};
        status[p] = kind == 0 ? run<0>(k) : kind == 1 ? run<1>(k) : kind == 2 ? run<2>(k) : run<3>(k);
    }
    FILE* g = fopen(argv[2], "wb");
    if (g == nullptr) return 2;
    fwrite(xo.data(), 8, xo.size(), g);
    fwrite(resid.data(), 8, resid.size(), g);
    fwrite(steps.data(), 4, steps.size(), g);
    fwrite(status.data(), 4, status.size(), g);
    fwrite(halvings.data(), 4, halvings.size(), g);
    return fclose(g) == 0 ? 0 : 2;
}
