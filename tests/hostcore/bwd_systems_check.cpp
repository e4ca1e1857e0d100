// bwd_systems_check.cpp -- TEST ARTEFACT.  The general-P backward on one CPU thread: P l + q with index-order sums, the
// duals, active sets and every entry of the systems through diffqcqp_amd/csrc/bwd_systems.h, then the loops of
// dense_core.h: chol_inverse_wave / ir_wave run sequentially (IrControl from kkt_core.h) and the kernels' scatter and
// gradient assembly.  tests/test_bwd_systems_hostcore.py holds the result bit-equal to the oracle.  Nothing in the
// product links or loads this file.
#include <vector>

#include "../../diffqcqp_amd/csrc/kkt_core.h"
#include "../../diffqcqp_amd/csrc/sbox_bounds.h"

using namespace dqq;
typedef std::vector<double> vec;

// dense_core.h: chol_inverse_wave, lane by lane
static void chol_inverse(vec& A, vec& Ainv, int n)
{
    for (int k = 0; k < n; ++k) {
        double s = 0.0;
        for (int j = 0; j < k; ++j) { const double t = A[k * n + j]; s += t * t; }
        const double xk = sqrt(A[k * n + k] - s);
        for (int i = k + 1; i < n; ++i) {
            double t = 0.0;
            for (int j = 0; j < k; ++j) t += A[i * n + j] * A[k * n + j];
            A[i * n + k] = (A[i * n + k] - t) / xk;
        }
        A[k * n + k] = xk;
    }
    for (int c = 0; c < n; ++c) {
        for (int i = 0; i < n; ++i) {
            double t = (i == c) ? 1.0 : 0.0;
            for (int j = 0; j < i; ++j) t -= A[i * n + j] * Ainv[j * n + c];
            Ainv[i * n + c] = t / A[i * n + i];
        }
        for (int i = n - 1; i >= 0; --i) {
            double t = Ainv[i * n + c];
            for (int j = i + 1; j < n; ++j) t -= A[j * n + i] * Ainv[j * n + c];
            Ainv[i * n + c] = t / A[i * n + i];
        }
    }
}

static double row_dot(const vec& M, int ld, int row, const vec& v, int n)
{
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += M[row * ld + j] * v[j];
    return s;
}

// dense_core.h: ir_wave for the rows x m system whose transpose is At (row stride m); -> xs, steps
static int refine(const vec& At, int rows, int m, const vec& dd, vec& xs)
{
    vec Ab(m), K(m * m), W(m * m), Kinv(m * m), KinvAb(m), d(m), t(m);
    for (int i = 0; i < m; ++i) {
        double s = 0.0;
        for (int k = 0; k < rows; ++k) s += At[k * m + i] * dd[k];
        Ab[i] = s;
        for (int j = 0; j < m; ++j) {
            double u = 0.0;
            for (int k = 0; k < rows; ++k) u += At[k * m + i] * At[k * m + j];
            K[i * m + j] = u;
        }
        K[i * m + i] += kMuIr;
    }
    W = K;
    chol_inverse(W, Kinv, m);
    for (int i = 0; i < m; ++i) KinvAb[i] = row_dot(Kinv, m, i, Ab, m);
    xs.assign(m, 0.0);
    IrControl ctl;
    ctl.init();
    int steps = 0;
    for (int it = 0; it < kIrMaxIter; ++it) {
        steps = it + 1;
        for (int i = 0; i < m; ++i) t[i] = row_dot(Kinv, m, i, xs, m);
        for (int i = 0; i < m; ++i) xs[i] = kMuIr * t[i] + KinvAb[i];
        double ss = 0.0;
        for (int i = 0; i < m; ++i) d[i] = row_dot(K, m, i, xs, m) - Ab[i];
        for (int i = 0; i < m; ++i) ss += d[i] * d[i];
        if (ctl.update(sqrt(ss))) break;
    }
    return steps;
}

extern "C" {

// One problem.  kind 0 QP, 1 QCQP (aux0 = l_n, aux1 = mu), 2 box QP (aux0 = l_min, aux1 = l_max), 3 signed box QP (+ v).
// Outputs as the kernels write them: grad_P (n,n), grad_q (n), gout0 / gout1 (grad_l_n, grad_mu (n/2) or grad_l_min,
// grad_l_max (n)), gamma / dgamma (n/2, or 2n as [lower | upper]), steps (1, box kinds 2).
// stats: how often each test of the header came out true / false -- [0,1] dual test (QP: x > eps; QCQP: gamma != 0; box: aL),
// [2,3] active test (QP, QCQP; box: aU), [4] box: nn == 0, [5] box: coordinates with both multipliers.
__attribute__((visibility("default"))) void bwd_systems_check(int kind, int n, const double* P, const double* q,
                                                              const double* aux0, const double* aux1, const double* v,
                                                              const double* x, const double* g, double eps,
                                                              double* grad_P, double* grad_q, double* gout0, double* gout1,
                                                              double* gamma_out, double* dgamma_out, int* steps, int* stats)
{
    const int nc = n / 2;
    vec xv(x, x + n), dl(n), xs, At, dd;
    for (int i = 0; i < 6; ++i) stats[i] = 0;
    if (kind == 0) {
        vec gam(n);
        std::vector<int> perm(n);
        for (int i = 0; i < n; ++i) {
            double s = 0.0;
            for (int j = 0; j < n; ++j) s += P[i * n + j] * x[j];
            gam[i] = qp_dual(s + q[i], x[i], eps);
            stats[x[i] > eps ? 0 : 1]++;
            stats[qp_active(gam[i]) ? 2 : 3]++;
        }
        int na = 0;
        for (int i = 0; i < n; ++i) if (qp_active(gam[i])) perm[na++] = i;
        int p = na;
        for (int i = 0; i < n; ++i) if (!qp_active(gam[i])) perm[p++] = i;
        const int m = n;
        At.resize(m * m);
        dd.resize(m);
        for (int rr = 0; rr < m; ++rr)
            for (int cc = 0; cc < m; ++cc) At[rr * m + cc] = qp_system_At(rr, cc, na, perm.data(), x, P, n);
        for (int i = 0; i < m; ++i) dd[i] = qp_system_rhs(i, na, perm.data(), g);
        steps[0] = refine(At, m, m, dd, xs);
        for (int i = 0; i < m; ++i) dl[perm[i]] = (i < na) ? 0.0 : xs[i];
    } else if (kind == 1) {
        vec plq(n), gam(nc), S(nc), dg(nc, 0.0);
        std::vector<int> perm(nc);
        for (int i = 0; i < n; ++i) {
            double s = 0.0;
            for (int j = 0; j < n; ++j) s += P[i * n + j] * x[j];
            plq[i] = s + q[i];
        }
        int na = 0;
        for (int c = 0; c < nc; ++c) {
            const QcqpDual ct = qcqp_contact(x[2 * c], x[2 * c + 1], plq[2 * c], plq[2 * c + 1], aux0[c], aux1[c], eps);
            gam[c] = ct.gamma;
            S[c] = ct.S;
            if (ct.act) perm[na++] = c;
            stats[ct.gamma != 0.0 ? 0 : 1]++;
            stats[ct.act ? 2 : 3]++;
        }
        const int m = n + na;
        At.resize(m * m);
        dd.resize(m);
        for (int rr = 0; rr < m; ++rr)
            for (int cc = 0; cc < m; ++cc)
                At[rr * m + cc] = qcqp_system_At(rr, cc, na, perm.data(), S.data(), gam.data(), x, P, n);
        for (int i = 0; i < m; ++i) dd[i] = system_rhs(i, na, g);
        steps[0] = refine(At, m, m, dd, xs);
        for (int i = 0; i < m; ++i) {
            if (i < na) dg[perm[i]] = xs[i];
            else dl[i - na] = xs[i];
        }
        for (int c = 0; c < nc; ++c) {
            gout0[c] = QcqpContact::e2(gam[c], aux0[c], aux1[c]) * dg[c];
            gout1[c] = QcqpContact::e1(gam[c], aux0[c], aux1[c]) * dg[c];
            gamma_out[c] = gam[c];
            dgamma_out[c] = dg[c];
        }
    } else {
        vec lo(aux0, aux0 + n), hi(aux1, aux1 + n), gam(2 * n, 0.0), dg(2 * n, 0.0);
        std::vector<char> keep_lo(n, 1), keep_hi(n, 1);
        std::vector<int> nnl(2 * n);
        int nn = 0;
        for (int i = 0; i < n; ++i) {
            if (kind == 3) {
                const SBoxBounds eb = sbox_bounds(lo[i], hi[i], v[i]);
                lo[i] = eb.lo; hi[i] = eb.hi; keep_lo[i] = eb.keep_lo; keep_hi[i] = eb.keep_hi;
            }
            const BoxNotNull b = box_not_null(x[i], lo[i], hi[i], eps);
            if (b.aL) nnl[nn++] = i;
            if (b.aU) nnl[nn++] = n + i;
            stats[b.aL ? 0 : 1]++;
            stats[b.aU ? 2 : 3]++;
            if (b.aL && b.aU) stats[5]++;
        }
        stats[4] = nn == 0;
        steps[0] = 1; // nn == 0: the reference runs one loop body on empty vectors
        if (nn > 0) {
            At.assign(n * nn, 0.0);
            dd.resize(n);
            for (int i = 0; i < n; ++i) {
                for (int p = 0; p < nn; ++p) At[i * nn + p] = box_dual_At(i, p, nnl.data(), n);
                dd[i] = box_dual_rhs(P + i * n, x, n, q[i]);
            }
            steps[0] = refine(At, n, nn, dd, xs);
            for (int p = 0; p < nn; ++p) gam[nnl[p]] = xs[p];
        }
        const int m = nn + n;
        At.resize(m * m);
        dd.resize(m);
        for (int rr = 0; rr < m; ++rr)
            for (int cc = 0; cc < m; ++cc) At[rr * m + cc] = box_system_At(rr, cc, nn, nnl.data(), gam.data(), P, n, n);
        for (int i = 0; i < m; ++i) dd[i] = system_rhs(i, nn, g);
        steps[1] = refine(At, m, m, dd, xs);
        for (int i = 0; i < m; ++i) {
            if (i < nn) dg[nnl[i]] = xs[i];
            else dl[i - nn] = xs[i];
        }
        for (int i = 0; i < n; ++i) {
            gout0[i] = keep_lo[i] ? -(dg[i] * gam[i]) : 0.0;
            gout1[i] = keep_hi[i] ? dg[n + i] * gam[n + i] : 0.0;
        }
        for (int i = 0; i < 2 * n; ++i) { gamma_out[i] = gam[i]; dgamma_out[i] = dg[i]; }
    }
    for (int i = 0; i < n; ++i) {
        grad_q[i] = -dl[i];
        for (int j = 0; j < n; ++j) grad_P[i * n + j] = -(dl[i] * x[j]);
    }
}

} // extern "C"
