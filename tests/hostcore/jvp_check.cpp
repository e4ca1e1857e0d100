// jvp_check.cpp -- TEST ARTEFACT.  dqq_jvp_f64 on one CPU thread: the duals, active sets, the transposed matrix, s = R^T(tangents)
// and dx = rhs^T(w) through the forward-mode helpers of diffqcqp_amd/csrc/bwd_systems.h, the refinement through the loops of
// bwd_systems_check.cpp (dense_core.h: chol_inverse_wave / ir_wave run sequentially).  tests/test_jvp_hostcore.py holds the result
// against the numpy restatement (tests/jvp_reference.py); the GPU tests hold the kernels against this.  Nothing in the product
// links or loads this file.
#include "bwd_systems_check.cpp"

extern "C" {

// One problem.  kind, aux0, aux1, v: as bwd_systems_check.  dP (n,n), dq (n), da, db: the tangents, NULL = zero.
// Outputs: dx (n), steps (1, box kinds 2).
__attribute__((visibility("default"))) void jvp_check(int kind, int n, const double* P, const double* q, const double* aux0,
                                                      const double* aux1, const double* v, const double* x, const double* dP,
                                                      const double* dq, const double* da, const double* db, double eps,
                                                      double* dx, int* steps)
{
    const int nc = n / 2;
    vec t(n), xs, A, s;
    for (int i = 0; i < n; ++i) {
        double dpx = 0.0;
        if (dP != nullptr)
            for (int j = 0; j < n; ++j) dpx += dP[i * n + j] * x[j];
        t[i] = jvp_coord(dpx, dq != nullptr ? dq[i] : 0.0);
    }
    if (kind == 0) {
        vec gam(n);
        std::vector<int> perm(n);
        for (int i = 0; i < n; ++i) {
            double r = 0.0;
            for (int j = 0; j < n; ++j) r += P[i * n + j] * x[j];
            gam[i] = qp_dual(r + q[i], x[i], eps);
        }
        int na = 0;
        for (int i = 0; i < n; ++i) if (qp_active(gam[i])) perm[na++] = i;
        int p = na;
        for (int i = 0; i < n; ++i) if (!qp_active(gam[i])) perm[p++] = i;
        const int m = n;
        A.resize(m * m);
        s.resize(m);
        for (int rr = 0; rr < m; ++rr)
            for (int cc = 0; cc < m; ++cc) A[rr * m + cc] = qp_system_A(rr, cc, na, perm.data(), x, P, n);
        for (int i = 0; i < m; ++i) s[i] = qp_jvp_s(i, na, perm.data(), t.data());
        steps[0] = refine(A, m, m, s, xs);
        for (int i = 0; i < m; ++i) dx[perm[i]] = jvp_dx_qp(i, na, xs[i]);
    } else if (kind == 1) {
        vec plq(n), gam(nc), S(nc), sm(nc);
        std::vector<int> perm(nc);
        for (int i = 0; i < n; ++i) {
            double r = 0.0;
            for (int j = 0; j < n; ++j) r += P[i * n + j] * x[j];
            plq[i] = r + q[i];
        }
        int na = 0;
        for (int c = 0; c < nc; ++c) {
            const QcqpDual ct = qcqp_contact(x[2 * c], x[2 * c + 1], plq[2 * c], plq[2 * c + 1], aux0[c], aux1[c], eps);
            gam[c] = ct.gamma;
            S[c] = ct.S;
            if (ct.act) {
                sm[na] = qcqp_jvp_mult(QcqpContact::e2(ct.gamma, aux0[c], aux1[c]), da != nullptr ? da[c] : 0.0,
                                       QcqpContact::e1(ct.gamma, aux0[c], aux1[c]), db != nullptr ? db[c] : 0.0);
                perm[na++] = c;
            }
        }
        const int m = n + na;
        A.resize(m * m);
        s.resize(m);
        for (int rr = 0; rr < m; ++rr)
            for (int cc = 0; cc < m; ++cc)
                A[rr * m + cc] = qcqp_system_A(rr, cc, na, perm.data(), S.data(), gam.data(), x, P, n);
        for (int i = 0; i < m; ++i) s[i] = system_jvp_s(i, na, sm.data(), t.data());
        steps[0] = refine(A, m, m, s, xs);
        for (int i = 0; i < n; ++i) dx[i] = xs[na + i];
    } else {
        vec lo(aux0, aux0 + n), hi(aux1, aux1 + n), gam(2 * n, 0.0), dlo(n), dhi(n), sm(2 * n), dd;
        std::vector<int> nnl(2 * n);
        int nn = 0;
        for (int i = 0; i < n; ++i) {
            dlo[i] = da != nullptr ? da[i] : 0.0;
            dhi[i] = db != nullptr ? db[i] : 0.0;
            if (kind == 3) {
                const SBoxBounds eb = sbox_bounds(lo[i], hi[i], v[i]);
                lo[i] = eb.lo; hi[i] = eb.hi;
                dlo[i] = eb.keep_lo ? dlo[i] : 0.0;
                dhi[i] = eb.keep_hi ? dhi[i] : 0.0;
            }
            const BoxNotNull b = box_not_null(x[i], lo[i], hi[i], eps);
            if (b.aL) nnl[nn++] = i;
            if (b.aU) nnl[nn++] = n + i;
        }
        steps[0] = 1;
        if (nn > 0) { // the dual recovery: the backward's, unchanged
            A.assign(n * nn, 0.0);
            dd.resize(n);
            for (int i = 0; i < n; ++i) {
                for (int p = 0; p < nn; ++p) A[i * nn + p] = box_dual_At(i, p, nnl.data(), n);
                dd[i] = box_dual_rhs(P + i * n, x, n, q[i]);
            }
            steps[0] = refine(A, n, nn, dd, xs);
            for (int p = 0; p < nn; ++p) gam[nnl[p]] = xs[p];
        }
        const int m = nn + n;
        A.resize(m * m);
        s.resize(m);
        for (int p = 0; p < nn; ++p) {
            const int i = nnl[p] < n ? nnl[p] : nnl[p] - n;
            sm[p] = box_jvp_mult(nnl[p], n, gam.data(), dlo[i], dhi[i]);
        }
        for (int rr = 0; rr < m; ++rr)
            for (int cc = 0; cc < m; ++cc) A[rr * m + cc] = box_system_A(rr, cc, nn, nnl.data(), gam.data(), P, n, n);
        for (int i = 0; i < m; ++i) s[i] = system_jvp_s(i, nn, sm.data(), t.data());
        steps[1] = refine(A, m, m, s, xs);
        for (int i = 0; i < n; ++i) dx[i] = xs[nn + i];
    }
}

} // extern "C"
