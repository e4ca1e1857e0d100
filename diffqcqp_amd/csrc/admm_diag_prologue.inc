// admm_diag_prologue.inc -- state set-up of the diagonal-P ADMM solve (power iteration in closed form, rho / tau
// start values, shifted diagonal and its reciprocals; Solver.cpp:46-59, 71-77 / 530-536), textually included by
// the solvers of admm_core.h.  Expects in scope: KIND, E, G, QP_LIKE, p, q, mu, and WARM with x0v (the lane's E coordinates
// of the caller's start point, read only if WARM); declares M, Minv, qp, l2, u, rho, inv_rho, tau_inc, tau_dec, Mmin, bad.
    double M[E], Minv[E], qp[E], l2[E], u[E];

    // ---- power_iteration, Solver.cpp:46-59 (K = 10 steps for QP :71, 100 for QCQP :530).
    // For a diagonal P the K normalised steps from the uniform start vector give v ~ p^K, so the
    // Rayleigh quotient the reference returns is  L = sum p^(2K+1) / sum p^(2K)  (the per-step
    // normalisations only rescale v).  Evaluated by repeated squaring on p scaled by an exact power
    // of two so that nothing overflows; ~1e-15 relative to the iterated value.
    double L;
    {
        // (round 4) The two sums are taken over a perfect binary tree in coordinate order -- within the lane here, across the
        // lanes in G::sum -- and nothing is contracted: L, and with it every iterate, is the same bits on one, two or four
        // lanes per problem (the forward picks the layout by batch size and by the caller's hint flag -- what the batch held
        // last time: a result must not depend on that).
#pragma clang fp contract(off)
        static_assert((E & (E - 1)) == 0, "coordinates per lane: a power of two");
        double m = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) m = fmax(m, fabs(p[e]));
        m = G::max(m);
        if (m > 0.0 && m < 1.79e308) {
            int k;
            (void)frexp(m, &k);
            double nv[E], dv[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double s1 = ldexp(p[e], -k); // |s1| < 1, the largest is >= 0.5
                const double s2 = s1 * s1, s4 = s2 * s2, s8 = s4 * s4, s16 = s8 * s8;
                double a; // s1^(2K)
                if (QP_LIKE) {
                    a = s16 * s4;                                   // ^20
                } else {
                    const double s32 = s16 * s16, s64 = s32 * s32, s128 = s64 * s64;
                    a = (s128 * s64) * s8;                          // ^200
                }
                dv[e] = a;
                nv[e] = a * s1;
            }
#pragma unroll
            for (int w = 1; w < E; w *= 2)
#pragma unroll
                for (int e = 0; e < E; e += 2 * w) {
                    dv[e] = dv[e] + dv[e + w];
                    nv[e] = nv[e] + nv[e + w];
                }
            const double num = G::sum(nv[0]);
            const double den = G::sum(dv[0]);
            L = ldexp(num / den, k);
        } else {
            L = (m > 0.0) ? NAN : 0.0; // P == 0 -> L = 0 (rho = 0 -> NaN, as in the reference); inf/NaN -> NaN
        }
    }

    // ---- Solver.cpp:72-77 / 531-536
    double p40, p15;
    G::pow_pair(L / mu, p40, p15);
    double rho = sqrt(mu * L) * p40;
    double tau_inc = p15, tau_dec = tau_inc;
    double itau_inc = fast_rcp(tau_inc), itau_dec = itau_inc;   // (admm_diag_body.inc: the reciprocals are state)
    double inv_rho = fast_rcp(rho);
    bool bad = !(rho > 0.0) || !(rho < 1.79e308);
    // Every M[e] receives the same sequence of additions and rounding is monotone, so the smallest M[e] is always
    // the one of the smallest p[e]: positivity of the shifted diagonal after a rho update is ONE comparison.
    // The smallest over the PROBLEM (not the lane): `bad` is then the same on every lane of a problem, which the loop's
    // exit on it (admm_diag_body.inc) and the hand-over of the re-spread (lane 0 of a problem speaks for it) rely on.
    double Mmin = p[0];
#pragma unroll
    for (int e = 1; e < E; ++e) Mmin = fmin(Mmin, p[e]);
    Mmin = -G::max(-Mmin);
    Mmin = Mmin + (rho + mu);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        M[e] = p[e] + (rho + mu);
        bad = bad || !(M[e] > 0.0);   // (also catches a NaN entry, which fmin above would drop)
        if constexpr (WARM) {
            // the warm start (dqq_fwd_warm_f64): l_2 = l_2_pred = x0 as given, u = -(P x0 + q), q_prox = q - mu x0 -- the state
            // in which the first x-update returns x0.  Elementwise, every product rounded on its own (no contraction): the
            // bits do not depend on how a problem's coordinates are spread over lanes, as everywhere in this file.
#pragma clang fp contract(off)
            const double px = p[e] * x0v[e];
            l2[e] = x0v[e];
            u[e] = -(px + q[e]);
            qp[e] = __builtin_fma(-mu, x0v[e], q[e]);
            bad = bad || !(x0v[e] - x0v[e] == 0.0);   // a NaN / infinite start point: NaN out, for this problem alone
        } else {
            qp[e] = q[e];
            l2[e] = 0.0;
            u[e] = 0.0;
        }
    }
    bad = G::max(bad ? 1.0 : 0.0) > 0.0;
    rcp_all<E>(M, Minv);
    if (QP_LIKE && bad) rho = 0.0;   // the lean body's exit on `bad` (admm_diag_body.inc): stop in the first iteration
