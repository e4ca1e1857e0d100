// path_core_check.cpp -- TEST ARTEFACT.  A stand-alone program: path_core.h's polish_problem_path (dqq_polish_path_f64) on one
// CPU thread over a batch read from a file, the results written to another.  tests/path_cases.py builds it (plain, and with the
// address and undefined-behaviour sanitizers) and runs it; tests/test_path_hostcore.py holds it to the numpy restatement
// tests/path_reference.py bit for bit, tests/test_gpu_path.py holds the kernels to it.  Nothing in the product links or loads
// this file.  smooth_core_check.cpp's file protocol, extended by the schedule.
//
// Input:  int32 kind, B, n, diag, in_place, max_halvings, n_stages; float64 reg; float64 kappas (n_stages); int32 stage_steps
//         (n_stages); then float64 P (B n n, or B n if diag), q (B n), a, b, c (as many entries as the kind has: QCQP B n/2 each;
//         box B n each; signed box also c), x (B n).
// Output: float64 x_out (B n), resid (B 2), stage_resid (B n_stages 2); int32 steps (B), status (B), halvings (B), stage_steps
//         (B n_stages).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../diffqcqp_amd/csrc/path_core.h"
#include "../../diffqcqp_amd/csrc/route.h"

using namespace dqq;

namespace {

bool read_all(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }
bool read_vec(FILE* f, std::vector<double>& v) { return read_all(f, v.data(), v.size() * 8); }

struct Call {
    const double *P, *q, *a, *b, *c, *x;
    double* x_out;
    int n, n_stages, max_halvings;
    bool diag;
    double reg;
    const double* kappas;
    const int* budgets;
    double *resid, *stage_resid, *work;
    int *steps, *halvings, *stage_steps;
};

template <int KIND>
int run(const Call& k)
{
    return polish_problem_path<KIND>(k.P, k.diag, k.q, k.a, k.b, k.c, k.x, k.x_out, k.n, k.kappas, k.budgets, k.n_stages, k.max_halvings,
                                     k.resid, k.steps, k.halvings, k.stage_resid, k.stage_steps, k.work, k.reg);
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (f == nullptr) return 2;
    int h[7];
    double reg;
    if (!read_all(f, h, sizeof h) || !read_all(f, &reg, sizeof reg)) return 2;
    const int kind = h[0], B = h[1], n = h[2], diag = h[3], in_place = h[4], max_halvings = h[5], S = h[6];
    if (kind < 0 || kind > 3 || B < 0 || n < 1 || max_halvings < 0 || S < 1 || S > kPolishPathMaxStages) return 2;
    std::vector<double> kappas(S);
    std::vector<int> budgets(S);
    if (!read_vec(f, kappas) || !read_all(f, budgets.data(), sizeof(int) * S)) return 2;
    const size_t np = diag ? (size_t)n : (size_t)n * n;
    const size_t ne = kind == 0 ? 0 : (kind == 1 ? (size_t)n / 2 : (size_t)n);
    const size_t nv = (size_t)B * n;
    std::vector<double> P(B * np), q(nv), a(B * ne), b(B * ne), c(kind == 3 ? nv : 0), x(nv);
    const bool ok = read_vec(f, P) && read_vec(f, q) && read_vec(f, a) && read_vec(f, b) && read_vec(f, c) && read_vec(f, x);
    fclose(f);
    if (!ok) return 2;
    std::vector<double> work((size_t)n * n + polish_vec_doubles(n));
    std::vector<double> xo(nv), resid((size_t)B * 2), stage_resid((size_t)B * S * 2);
    std::vector<int> steps(B), status(B), halvings(B), stage_steps((size_t)B * S);
    if (in_place) xo = x;
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
        Call k{};
        k.P = P.data() + p * np; k.q = q.data() + v;
        k.a = ne ? a.data() + p * ne : nullptr; k.b = ne ? b.data() + p * ne : nullptr; k.c = kind == 3 ? c.data() + v : nullptr;
        k.x = in_place ? xo.data() + v : x.data() + v;
        k.x_out = xo.data() + v;
        k.n = n; k.n_stages = S; k.max_halvings = max_halvings; k.diag = diag != 0; k.reg = reg;
        k.kappas = kappas.data(); k.budgets = budgets.data();
        k.resid = resid.data() + 2 * (size_t)p; k.stage_resid = stage_resid.data() + 2 * (size_t)p * S;
        k.steps = &steps[p]; k.halvings = &halvings[p]; k.stage_steps = stage_steps.data() + (size_t)p * S;
        k.work = work.data();
        status[p] = kind == 0 ? run<0>(k) : kind == 1 ? run<1>(k) : kind == 2 ? run<2>(k) : run<3>(k);
    }
    FILE* g = fopen(argv[2], "wb");
    if (g == nullptr) return 2;
    for (const std::vector<double>* d : {&xo, &resid, &stage_resid})
        if (!d->empty()) fwrite(d->data(), 8, d->size(), g);
    for (const std::vector<int>* d : {&steps, &status, &halvings, &stage_steps})
        if (!d->empty()) fwrite(d->data(), 4, d->size(), g);
    return fclose(g) == 0 ? 0 : 2;
}
