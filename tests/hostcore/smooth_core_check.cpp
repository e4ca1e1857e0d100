// smooth_core_check.cpp -- TEST ARTEFACT.  A stand-alone program: smooth_core.h's polish_problem_smooth,
// newton_bwd_problem_smooth and newton_jvp_problem_smooth (dqq_polish_smooth_f64, dqq_newton_bwd_smooth_f64,
// dqq_newton_jvp_smooth_f64) on one CPU thread over a batch read from a file, the results written to another.
// tests/smooth_cases.py builds it (plain, and with the address and undefined-behaviour sanitizers) and runs it;
// tests/test_smooth_hostcore.py holds it to the numpy restatement bit for bit, tests/test_gpu_smooth.py holds the kernels to it.
// Nothing in the product links or loads this file.
//
// Input:  int32 mode (0 polish, 1 backward, 2 JVP), kind, B, n, diag, max_steps, in_place, max_halvings, given (JVP: bit i set
//         = tangent i of dP, dq, da, db follows); float64 reg, kappa; then float64 P (B n n, or B n if diag), q (B n), a, b, c (as
//         many entries as the kind has: QCQP B n/2 each; box B n each; signed box also c), x (B n); backward: grad_x (B n); JVP:
//         the given tangents, shaped as their inputs.
// Output: polish: float64 x_out (B n), resid (B 2); int32 steps (B), status (B), halvings (B).
//         backward: float64 grad_P (as P), grad_q (B n), grad_a, grad_b (as a; none for the QP); int32 status (B).
//         JVP: float64 dx (B n); int32 status (B).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../diffqcqp_amd/csrc/smooth_core.h"

using namespace dqq;

namespace {

bool read_all(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }
bool read_vec(FILE* f, std::vector<double>& v) { return read_all(f, v.data(), v.size() * 8); }

struct Call {
    const double *P, *q, *a, *b, *c, *x;
    int n, max_steps, max_halvings;
    bool diag;
    double reg, kappa;
    double* work;
    // polish
    double *x_out, *resid;
    int *steps, *halvings;
    // backward
    const double* gx;
    double *gP, *gq, *ga, *gb;
    // JVP
    const double *dP, *dq, *da, *db;
    double* dx;
};

template <int KIND>
int run(int mode, const Call& k)
{
    if (mode == 0)
        return polish_problem_smooth<KIND>(k.P, k.diag, k.q, k.a, k.b, k.c, k.x, k.x_out, k.n, k.max_steps, k.max_halvings, k.resid,
                                           k.steps, k.halvings, k.work, k.reg, k.kappa);
    if (mode == 1)
        return newton_bwd_problem_smooth<KIND>(k.P, k.diag, k.q, k.a, k.b, k.c, k.x, k.gx, k.gP, k.gq, k.ga, k.gb, k.n, k.work, k.reg,
                                               k.kappa);
    return newton_jvp_problem_smooth<KIND>(k.P, k.diag, k.q, k.a, k.b, k.c, k.x, k.dP, k.dq, k.da, k.db, k.dx, k.n, k.work, k.reg, k.kappa);
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (f == nullptr) return 2;
    int h[9];
    double rk[2];
    if (!read_all(f, h, sizeof h) || !read_all(f, rk, sizeof rk)) return 2;
    const int mode = h[0], kind = h[1], B = h[2], n = h[3], diag = h[4], max_steps = h[5], in_place = h[6], max_halvings = h[7], given = h[8];
    if (mode < 0 || mode > 2 || kind < 0 || kind > 3 || B < 0 || n < 1 || max_halvings < 0) return 2;
    const size_t np = diag ? (size_t)n : (size_t)n * n;
    const size_t ne = kind == 0 ? 0 : (kind == 1 ? (size_t)n / 2 : (size_t)n);
    const size_t nv = (size_t)B * n;
    std::vector<double> P(B * np), q(nv), a(B * ne), b(B * ne), c(kind == 3 ? nv : 0), x(nv), gx(mode == 1 ? nv : 0);
    std::vector<double> dP(mode == 2 && (given & 1) ? B * np : 0), dq(mode == 2 && (given & 2) ? nv : 0),
        da(mode == 2 && (given & 4) ? B * ne : 0), db(mode == 2 && (given & 8) ? B * ne : 0);
    bool ok = read_vec(f, P) && read_vec(f, q) && read_vec(f, a) && read_vec(f, b) && read_vec(f, c) && read_vec(f, x) && read_vec(f, gx) &&
              read_vec(f, dP) && read_vec(f, dq) && read_vec(f, da) && read_vec(f, db);
    fclose(f);
    if (!ok) return 2;
    std::vector<double> work((size_t)n * n + polish_vec_doubles(n));
    std::vector<double> xo(mode == 0 ? nv : 0), resid(mode == 0 ? (size_t)B * 2 : 0), gP(mode == 1 ? B * np : 0), gq(mode == 1 ? nv : 0),
        ga(mode == 1 ? B * ne : 0), gb(mode == 1 ? B * ne : 0), dx(mode == 2 ? nv : 0);
    std::vector<int> steps(mode == 0 ? B : 0), halvings(mode == 0 ? B : 0), status(B);
    if (mode == 0 && in_place) xo = x;
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
        Call k{};
        k.P = P.data() + p * np; k.q = q.data() + v;
        k.a = ne ? a.data() + p * ne : nullptr; k.b = ne ? b.data() + p * ne : nullptr; k.c = kind == 3 ? c.data() + v : nullptr;
        k.x = mode == 0 && in_place ? xo.data() + v : x.data() + v;
        k.n = n; k.max_steps = max_steps; k.max_halvings = max_halvings; k.diag = diag != 0; k.reg = rk[0]; k.kappa = rk[1];
        k.work = work.data();
        if (mode == 0) { k.x_out = xo.data() + v; k.resid = resid.data() + 2 * (size_t)p; k.steps = &steps[p]; k.halvings = &halvings[p]; }
        if (mode == 1) {
            k.gx = gx.data() + v; k.gP = gP.data() + p * np; k.gq = gq.data() + v;
            k.ga = ne ? ga.data() + p * ne : nullptr; k.gb = ne ? gb.data() + p * ne : nullptr;
        }
        if (mode == 2) {
            k.dP = dP.empty() ? nullptr : dP.data() + p * np; k.dq = dq.empty() ? nullptr : dq.data() + v;
            k.da = da.empty() ? nullptr : da.data() + p * ne; k.db = db.empty() ? nullptr : db.data() + p * ne;
            k.dx = dx.data() + v;
        }
        status[p] = kind == 0 ? run<0>(mode, k) : kind == 1 ? run<1>(mode, k) : kind == 2 ? run<2>(mode, k) : run<3>(mode, k);
    }
    FILE* g = fopen(argv[2], "wb");
    if (g == nullptr) return 2;
    for (const std::vector<double>* d : {&xo, &resid, &gP, &gq, &ga, &gb, &dx})
        if (!d->empty()) fwrite(d->data(), 8, d->size(), g);
    for (const std::vector<int>* d : {&steps, &status, &halvings})
        if (!d->empty()) fwrite(d->data(), 4, d->size(), g);
    return fclose(g) == 0 ? 0 : 2;
}
