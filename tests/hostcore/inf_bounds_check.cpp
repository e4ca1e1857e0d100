// inf_bounds_check.cpp -- TEST ARTEFACT.  The four host cores of the Newton family (csrc/polish_core.h: polish_problem;
// csrc/newton_core.h: newton_jvp_problem, newton_bwd_problem, newton_jac_problem) on one CPU thread over a batch, with the
// one-sided-box flag (inf_ok: DQQ_F_INFINITE_BOUNDS) as an argument.  A stand-alone program: tests/inf_bounds_cases.py builds it
// plain (the yardstick of tests/test_gpu_inf_bounds.py) and with the address and undefined-behaviour sanitizers (run by
// tests/test_inf_bounds_hostcore.py over its mixed-bounds batches), and talks to it through two files.  Nothing in the product
// links or loads this file.
//
// usage: inf_bounds_check IN OUT
// IN:  int32 kind, B, n, diag, max_steps, inf_ok, has_c, has_tan (dP, dq, da, db present), then doubles: P (B n n; diag: B n),
//      q (B n), a, b (B ne), [c (B n)], x (B n), gx (B n), [dP (as P), dq (B n), da, db (B ne)]
// OUT: doubles x_out (B n), resid (B 2), dx (B n), gP (as P), gq (B n), ga, gb (B ne), Jq, Ja, Jb (as include/diffqcqp_hip.h shapes
//      them); then int32 steps (B) and the statuses of the polish, the JVP, the backward and the Jacobians (B each)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../diffqcqp_amd/csrc/newton_core.h"

using namespace dqq;

namespace {

const double* at(const std::vector<double>& v, size_t off) { return v.empty() ? nullptr : v.data() + off; }
double* at(std::vector<double>& v, size_t off) { return v.empty() ? nullptr : v.data() + off; }

bool read_into(FILE* f, std::vector<double>& v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(double), n, f) == n;
}

template <int KIND>
void run(int B, int n, bool diag, int max_steps, bool inf_ok, const std::vector<double>& P, const std::vector<double>& q,
         const std::vector<double>& a, const std::vector<double>& b, const std::vector<double>& c, const std::vector<double>& x,
         const std::vector<double>& gx, const std::vector<double>& dP, const std::vector<double>& dq, const std::vector<double>& da,
         const std::vector<double>& db, FILE* out)
{
    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = newton_jac_extra_cols(KIND, n);
    const size_t jq = diag ? (KIND == 1 ? 2 * (size_t)n : (size_t)n) : (size_t)n * n, je = diag ? (size_t)n : (size_t)n * ne;
    std::vector<double> xo((size_t)B * n), resid((size_t)B * 2), dx((size_t)B * n), gP(B * np), gq((size_t)B * n), ga(B * ne),
        gb(B * ne), Jq(B * jq), Ja(ne ? B * je : 0), Jb(ne ? B * je : 0);
    std::vector<int> ints((size_t)5 * B);
    std::vector<double> work(newton_jac_work_doubles(KIND, n));
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
        ints[p] = -1;
        ints[B + p] = polish_problem<KIND>(P.data() + p * np, diag, q.data() + v, at(a, p * ne), at(b, p * ne), at(c, v), x.data() + v,
                                           xo.data() + v, n, max_steps, resid.data() + 2 * (size_t)p, &ints[p], work.data(), inf_ok);
        ints[2 * B + p] = newton_jvp_problem<KIND>(P.data() + p * np, diag, q.data() + v, at(a, p * ne), at(b, p * ne), at(c, v),
                                                   x.data() + v, at(dP, p * np), at(dq, v), at(da, p * ne), at(db, p * ne),
                                                   dx.data() + v, n, work.data(), inf_ok);
        ints[3 * B + p] = newton_bwd_problem<KIND>(P.data() + p * np, diag, q.data() + v, at(a, p * ne), at(b, p * ne), at(c, v),
                                                   x.data() + v, gx.data() + v, gP.data() + p * np, gq.data() + v, at(ga, p * ne),
                                                   at(gb, p * ne), n, work.data(), inf_ok);
        ints[4 * B + p] = newton_jac_problem<KIND>(P.data() + p * np, diag, q.data() + v, at(a, p * ne), at(b, p * ne), at(c, v),
                                                   x.data() + v, Jq.data() + p * jq, at(Ja, p * je), at(Jb, p * je), n, work.data(),
                                                   inf_ok);
    }
    for (const std::vector<double>* w : {&xo, &resid, &dx, &gP, &gq, &ga, &gb, &Jq, &Ja, &Jb})
        if (!w->empty()) fwrite(w->data(), sizeof(double), w->size(), out);
    fwrite(ints.data(), sizeof(int), ints.size(), out);
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int h[8];
    if (f == nullptr || fread(h, sizeof(int), 8, f) != 8) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const int kind = h[0], B = h[1], n = h[2], max_steps = h[4];
    const bool diag = h[3] != 0, inf_ok = h[5] != 0, has_c = h[6] != 0, has_tan = h[7] != 0;
    if (kind < 0 || kind > 3 || B < 0 || n < 1 || (kind == 1 && n % 2)) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = newton_jac_extra_cols(kind, n), bn = (size_t)B * n;
    std::vector<double> P, q, a, b, c, x, gx, dP, dq, da, db;
    bool ok = read_into(f, P, B * np) && read_into(f, q, bn) && read_into(f, a, B * ne) && read_into(f, b, B * ne) &&
              read_into(f, c, has_c ? bn : 0) && read_into(f, x, bn) && read_into(f, gx, bn);
    if (has_tan) ok = ok && read_into(f, dP, B * np) && read_into(f, dq, bn) && read_into(f, da, B * ne) && read_into(f, db, B * ne);
    fclose(f);
    if (!ok) { fprintf(stderr, "%s is too short\n", argv[1]); return 2; }
    FILE* out = fopen(argv[2], "wb");
    if (out == nullptr) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    switch (kind) {
    case 0: run<0>(B, n, diag, max_steps, inf_ok, P, q, a, b, c, x, gx, dP, dq, da, db, out); break;
    case 1: run<1>(B, n, diag, max_steps, inf_ok, P, q, a, b, c, x, gx, dP, dq, da, db, out); break;
    case 2: run<2>(B, n, diag, max_steps, inf_ok, P, q, a, b, c, x, gx, dP, dq, da, db, out); break;
    default: run<3>(B, n, diag, max_steps, inf_ok, P, q, a, b, c, x, gx, dP, dq, da, db, out); break;
    }
    return fclose(out) == 0 ? 0 : 2;
}
