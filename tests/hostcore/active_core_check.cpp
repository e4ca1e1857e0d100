// active_core_check.cpp -- TEST ARTEFACT.  csrc/active_core.h's active_problem on one CPU thread over a batch, with the
// one-sided-box flag (inf_ok: DQQ_F_INFINITE_BOUNDS) as an argument.  A stand-alone program: tests/active_cases.py builds it
// plain (the yardstick of tests/test_gpu_active.py) and with the address and undefined-behaviour sanitizers (run by
// tests/test_active_hostcore.py over the same batches), and talks to it through two files.  Nothing in the product links or
// loads this file.
//
// usage: active_core_check IN OUT
// IN:  int32 kind, B, n, diag, inf_ok, has_c, mask (bit i: output i of state, mult, margin, where is requested; the others are
//      passed as NULL and come back as the fill -7 / 7.0), 0; then doubles: P (B n n; diag: B n), q (B n), a, b (B ne), [c (B n)],
//      x (B n)
// OUT: int32 state (B ne), where (B), status (B); then doubles mult (B ne), margin (B)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../diffqcqp_amd/csrc/active_core.h"

using namespace dqq;

namespace {

const double* at(const std::vector<double>& v, size_t off) { return v.empty() ? nullptr : v.data() + off; }

bool read_into(FILE* f, std::vector<double>& v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(double), n, f) == n;
}

template <int KIND>
void run(int B, int n, bool diag, bool inf_ok, int mask, const std::vector<double>& P, const std::vector<double>& q,
         const std::vector<double>& a, const std::vector<double>& b, const std::vector<double>& c, const std::vector<double>& x,
         FILE* out)
{
    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = (size_t)active_elements(KIND, n), nx = KIND == 0 ? 0 : ne;
    std::vector<int> state(B * ne, -7), where((size_t)B, -7), status((size_t)B, -7);
    std::vector<double> mult(B * ne, 7.0), margin((size_t)B, 7.0), z((size_t)n);
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
        status[p] = active_problem<KIND>(P.data() + p * np, diag, q.data() + v, at(a, p * nx), at(b, p * nx), at(c, v), x.data() + v, n,
                                         (mask & 1) ? state.data() + p * ne : nullptr, (mask & 2) ? mult.data() + p * ne : nullptr,
                                         (mask & 4) ? margin.data() + p : nullptr, (mask & 8) ? where.data() + p : nullptr, z.data(),
                                         inf_ok);
    }
    for (const std::vector<int>* w : {&state, &where, &status})
        if (!w->empty()) fwrite(w->data(), sizeof(int), w->size(), out);
    for (const std::vector<double>* w : {&mult, &margin})
        if (!w->empty()) fwrite(w->data(), sizeof(double), w->size(), out);
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int h[8];
    if (f == nullptr || fread(h, sizeof(int), 8, f) != 8) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const int kind = h[0], B = h[1], n = h[2], mask = h[6];
    const bool diag = h[3] != 0, inf_ok = h[4] != 0, has_c = h[5] != 0;
    if (kind < 0 || kind > 3 || B < 0 || n < 1 || (kind == 1 && n % 2)) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t np = diag ? (size_t)n : (size_t)n * n, nx = kind == 0 ? 0 : (size_t)active_elements(kind, n), bn = (size_t)B * n;
    std::vector<double> P, q, a, b, c, x;
    const bool ok = read_into(f, P, B * np) && read_into(f, q, bn) && read_into(f, a, B * nx) && read_into(f, b, B * nx) &&
                    read_into(f, c, has_c ? bn : 0) && read_into(f, x, bn);
    fclose(f);
    if (!ok) { fprintf(stderr, "%s is too short\n", argv[1]); return 2; }
    FILE* out = fopen(argv[2], "wb");
    if (out == nullptr) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    switch (kind) {
    case 0: run<0>(B, n, diag, inf_ok, mask, P, q, a, b, c, x, out); break;
    case 1: run<1>(B, n, diag, inf_ok, mask, P, q, a, b, c, x, out); break;
    case 2: run<2>(B, n, diag, inf_ok, mask, P, q, a, b, c, x, out); break;
    default: run<3>(B, n, diag, inf_ok, mask, P, q, a, b, c, x, out); break;
    }
    return fclose(out) == 0 ? 0 : 2;
}
