// admm_diag_body.inc -- ONE ADMM iteration of the diagonal-P solve (Solver.cpp:80-120 / 539-580), textually included
// into the loops of admm_core.h (admm_fwd_diag: wave-private tiles; admm_fwd_diag_compact: tiles repacked across
// the waves of a workgroup).  Expects in scope: KIND, E, G, QP_LIKE, the per-lane state M, Minv, q, qp, l2, u,
// rad / lo / hi / sg, rho, inv_rho, tau_inc, tau_dec, Mmin, rho_up, cpt, bad, iters, the loop counter `it`, and
// eps, mu, adaptive; DQQ_ADMM_ON_STOP is the statement that leaves the loop when the stopping test passes.
// With DQQ_ADMM_LEAN defined (admm_core.h: the loops of the diagonal forward, round 6) the caller also provides `adaptive_on`
// (bool: adaptive != 0) and `badi` (int: the `bad` flag kept in a vector register) and the body avoids what costs scalar
// instructions at every divergent join: `adaptive` is folded into the firing test, `bad` is not a bool, and the QCQP's second
// stopping test sits behind a wave-uniform branch with scalar mask arithmetic.  Same arithmetic, same bits.
// With DQQ_ADMM_GENERAL_P defined (group_dense.h: a general P, rows spread over the lanes of the group) the
// diagonal scale and the E reciprocals are replaced by DQQ_ADMM_SOLVE(l) and DQQ_ADMM_REFACTOR(delta).
// Every fused multiply-add of the iteration is written out and the compiler may not form others: the bits of an
// iterate must not depend on the instantiation (E, the lane layout) the code is compiled into -- admm_fwd_diag_respread
// moves problems between two of them in mid-solve.
#pragma clang fp contract(off)
#ifdef DQQ_CHECK_GROUPS
            // debug builds (DQQ_EXTRA_FLAGS=-DDQQ_CHECK_GROUPS): the lanes of a problem must leave the loop together --
            // a DPP read from a lane that has left returns 0.0 (common.h dpp_f64), so every group reduction below
            // rests on it.  Trap if the execution mask ever holds part of a group.
            {
                const unsigned long long live = __ballot(true);
                unsigned long long heads = 0;
                for (int g0 = 0; g0 < 64; g0 += G::kLanes) heads |= 1ull << g0;
                const unsigned long long full = (G::kLanes == 64) ? ~0ull : ((1ull << G::kLanes) - 1);
                if (live != (live & heads) * full) __builtin_trap();
            }
#endif
#if defined(DQQ_SALU_PROBE_DIAG) && defined(__HIPCC__)
            // measurement only (tools/ab_salu_probe.sh diag): extra scalar instructions per ADMM iteration of the diagonal path
#pragma unroll
            for (int sp = 0; sp < DQQ_SALU_PROBE_DIAG; ++sp) { int sd; asm volatile("s_mov_b32 %0, 0" : "=s"(sd)); }
#endif
            double rd = 0.0, rp = 0.0;
            double w[E], z[E], lv[(KIND == 1) ? E : 1];
#ifdef DQQ_ADMM_GENERAL_P
            double lsol[E];
            DQQ_ADMM_SOLVE(lsol);                                             // (P + (rho+mu) I)^-1 (rho l2 - u - qp)
#endif
#pragma unroll
            for (int e = 0; e < E; ++e) {
#ifdef DQQ_ADMM_GENERAL_P
                const double l = lsol[e];                                     // :80 / :539
#else
                const double l = Minv[e] * (__builtin_fma(rho, l2[e], -u[e]) - qp[e]); // :80 / :539
#endif
                qp[e] = __builtin_fma(-mu, l, q[e]);                          // :81 / :540
                w[e] = __builtin_fma(kAlpha, l, (1 - kAlpha) * l2[e]);        // alpha*l + (1-alpha)*l2_pred
                z[e] = __builtin_fma(u[e], inv_rho, w[e]);                    // :82 / :541
                if (KIND == 1) lv[e] = l;
            }
            if (KIND == 0) {
#pragma unroll
                for (int e = 0; e < E; ++e) z[e] = fmax(z[e], 0.0);           // cwiseMax(0), :82
            } else if (KIND == 2 || KIND == 3) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    double t = z[e];
                    t = t < lo[e] ? lo[e] : t;                                // cwiseMax(l_min), :219 / :396
                    t = hi[e] < t ? hi[e] : t;                                // cwiseMin(l_max), :220 / :397
                    if (KIND == 3) {                                          // v o min(v o l_2, 0), :398
                        double m = sg[e] * t;
                        m = 0 < m ? 0 : m;
                        t = sg[e] * m;
                    }
                    z[e] = t;
                }
            }
            double dw[E], dz[E];
            if (KIND == 1) {
#if defined(__HIPCC__)
                if constexpr (E == 1) {
                    // one coordinate per lane (the last survivors of a tile on eight lanes each, admm_core.h): the
                    // contact's other coordinate is the neighbour's; both lanes form the same a, b and the same scale
                    const bool odd = (threadIdx.x & 1) != 0;
                    const double own = z[0], oth = partner<1>(own);
                    const double a = odd ? oth : own, b = odd ? own : oth;
                    const double n2 = __builtin_fma(b, b, a * a);
                    const double rn = fast_rsqrt(n2);
                    const double sc = (n2 > rad[0] * fabs(rad[0])) ? rad[0] * rn : 1.0;   // (see below)
                    z[0] = own * sc;
                } else
#endif
                {
#pragma unroll
                    for (int c = 0; c < E / 2; ++c) {                         // prox_circle, :505-519
                        const double a = z[2 * c], b = z[2 * c + 1];
                        const double n2 = __builtin_fma(b, b, a * a);
                        const double rn = fast_rsqrt(n2);      // n2 == 0: inf, and no scaling (0 > r|r| is false for r >= 0)
                        // |l_(c)| > r (:513-514) tested on the squares: |l|^2 > r |r| -- the right-hand side is loop-invariant
                        // (the compiler hoists it), so the norm itself is never formed (round 5: one multiplication per
                        // contact and iteration less; a negative radius still scales every iterate, as in the reference)
                        const double sc = (n2 > rad[c] * fabs(rad[c])) ? rad[c] * rn : 1.0; // one select; * 1.0 is exact
                        z[2 * c] = a * sc;
                        z[2 * c + 1] = b * sc;
                    }
                }
            }
            // differences of the ROUNDED iterates, as the reference takes them (:84-86 / :544-546): an iterate that
            // has stopped moving gives res_dual == 0 exactly (fma(a, sc, -l2) would leave the product's rounding
            // error, which at eps = 1e-10 and |x| ~ 1e3 is another iteration: tests/golden ref_m2_qcqp)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                dw[e] = w[e] - z[e];
                dz[e] = z[e] - l2[e];
            }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                u[e] = __builtin_fma(rho, dw[e], u[e]);                       // :83 / :543
                l2[e] = z[e];                                                 // :87 / :547
            }
            if constexpr (E == 1) {
                rd = max_abs2(dz[0], dz[0]);
                rp = max_abs2(dw[0], dw[0]);
            } else {
                rd = max_abs2(dz[E > 1 ? 0 : 0], dz[E > 1 ? 1 : 0]);          // :84-85 / :544-545
                rp = max_abs2(dw[E > 1 ? 0 : 0], dw[E > 1 ? 1 : 0]);          // :86 / :546
#pragma unroll
                for (int e = 2; e < E; ++e) {
                    rd = max_abs1(rd, dz[e]);
                    rp = max_abs1(rp, dw[e]);
                }
            }
            G::max2(rd, rp);   // (both residual maxima, their butterflies interleaved)
            const double res_dual = rho * rd;   // max|rho*d| == rho*max|d| for rho > 0
            const double res_prim = rp;
            iters = it + 1;
            // :88.  A problem whose shifted diagonal lost positivity (`bad`) stops too: the reference's llt() gives NaN
            // there, its residual max skips the NaN (res_dual = 0) and the loop ends in the iteration after the update.  Not
            // the QCQP: its second test compares with eps + 1e-4 |NaN|, fails, and the reference runs to max_iter.
            // (The lean body takes that exit through rho = 0 -- res_dual = 0 * rd -- set where `bad` arises: no instruction
            // in the loop's common path.)
#if defined(DQQ_ADMM_LEAN)
            bool stop = res_dual < eps;
#else
            bool stop = res_dual < eps || (QP_LIKE && bad);
#endif
#if defined(DQQ_ADMM_LEAN)
            [[maybe_unused]] unsigned long long stop_mask = 0;   // QCQP: the lanes that pass BOTH tests (a scalar)
#endif
            if (KIND == 1) {
#if defined(DQQ_ADMM_LEAN) && defined(__HIPCC__)
                // a WAVE-UNIFORM branch (any lane passed the dual test), the second test evaluated by every lane: an
                // instruction costs the wave the same whatever the number of lanes under it, and `stop` stays a scalar lane
                // mask across a uniform join (across a divergent one it took a round trip through a vector register)
                stop_mask = __ballot(stop);
                if (stop_mask != 0ull) {
#else
                if (stop) {
#endif
                    // res_prim < eps + 1e-4 |l|_2 (:548), only evaluated once the dual test passes, and without
                    // the square root: t = res_prim - eps < 0, or t^2 < 1e-8 |l|^2
                    // (summed contact by contact: the same association whichever way a problem is spread over lanes)
                    double nl = 0.0;
#if defined(__HIPCC__)
                    if constexpr (E == 1) {
                        const bool odd = (threadIdx.x & 1) != 0;
                        const double own = lv[0], oth = partner<1>(own);
                        const double a = odd ? oth : own, b = odd ? own : oth;
                        nl += __builtin_fma(b, b, a * a);
                        // both lanes of a contact hold its term: the tree over the CONTACTS, as with a contact per lane
                        if constexpr (G::kLanes >= 4) nl = nl + partner<2>(nl);
                        if constexpr (G::kLanes >= 8) nl = nl + partner<4>(nl);
                    } else
#endif
                    {
                        // a binary tree over the contacts in index order, continued across the lanes by G::sum: the same
                        // association on one, two or four lanes per problem
                        double cs[E / 2];
#pragma unroll
                        for (int c = 0; c < E / 2; ++c) cs[c] = __builtin_fma(lv[2 * c + 1], lv[2 * c + 1], lv[2 * c] * lv[2 * c]);
#pragma unroll
                        for (int w = 1; w < E / 2; w *= 2)
#pragma unroll
                            for (int c = 0; c + w < E / 2; c += 2 * w) cs[c] = cs[c] + cs[c + w];
                        nl = G::sum(cs[0]);
                    }
                    const double t = res_prim - eps;
#if defined(DQQ_ADMM_LEAN) && defined(__HIPCC__)
                    stop_mask &= __ballot(t < 0.0) | __ballot(t * t < (kEpsRel * kEpsRel) * nl);   // scalar mask arithmetic
                    stop = ((stop_mask >> (threadIdx.x & 63)) & 1ull) != 0;
#else
                    stop = t < 0.0 || t * t < (kEpsRel * kEpsRel) * nl;
#endif
                }
            }
            if (stop) DQQ_ADMM_ON_STOP;
#if defined(DQQ_ADMM_LEAN)
            {   // (`adaptive` is folded into `fire` below: one scalar AND instead of a branch and a join of its own)
#else
            if (adaptive) {
#endif
                // rho adaptation, Solver.cpp:90-120 / 550-580: increase when the primal residual dominates,
                // decrease when the dual one does, at most once every 5 imbalanced iterations.  Same state
                // machine as common.h RhoSchedule (used by the general kernels), kept inline here: through the
                // struct this kernel measured 0.7 us (2 %) slower at the bench shape.
                const bool inc = res_prim > kMuThresh * res_dual;             // :92 / :552
                const bool dec = !inc && (res_dual > kMuThresh * res_prim);   // :106 / :566
                const bool imb = inc || dec;
#if defined(DQQ_ADMM_LEAN)
                const bool fire = imb && (cpt == 0) && adaptive_on;           // cpt % 5 == 0 (and the caller wants adaptation)
#else
                const bool fire = imb && (cpt == 0);                          // cpt % 5 == 0
#endif
                cpt = imb ? (cpt == 4 ? 0 : cpt + 1) : cpt;                   // cpt++ (kept mod 5)
                if (fire) {
                    if (rho_up == (inc ? -1 : 1)) {                           // direction flipped: damp tau
                        const double ti = __builtin_fma(.8, tau_inc - 1, 1.0), td = __builtin_fma(.8, tau_dec - 1, 1.0);
                        // QCQP: 1/tau is state (round 4).  A tau changes only here, on a change of direction, while the update
                        // below runs -- for the whole wave -- on every trip in which ANY lane fires; the reciprocal of an
                        // unchanged tau is the same bits every time (QCQP forward 29.9 -> 29.4 us).  The QP-like kinds damp
                        // BOTH taus here: two reciprocals per change of direction cost them more than the one per firing
                        // they save (QP forward 25.1 -> 26.3 us, A/B of the builds), so they keep the reciprocal below.
                        if (QP_LIKE) { tau_inc = ti; tau_dec = td; }          // :94-97, :108-111 (QP damps both)
                        else if (inc) { tau_inc = ti; itau_inc = fast_rcp(ti); }  // :554-556
                        else { tau_dec = td; itau_dec = fast_rcp(td); }           // :568-570
                    }
                    // one reciprocal per update, of the factor in use: rho and 1/rho move by reciprocal factors
                    const double tau = inc ? tau_inc : tau_dec;
                    const double inv_tau = QP_LIKE ? fast_rcp(tau) : (inc ? itau_inc : itau_dec);
                    const double f = inc ? tau : inv_tau;                     // rho *= tau_inc | rho /= tau_dec
                    const double delta = rho * (f - 1);                       // :98 / :112
                    rho = rho * f;                                            // :99 / :113
                    rho_up = inc ? 1 : -1;
                    inv_rho = inv_rho * (inc ? inv_tau : tau);
#ifdef DQQ_ADMM_GENERAL_P
                    DQQ_ADMM_REFACTOR(delta);                                 // llt() + solveInPlace(Identity), :100-101
#else
                    // llt() + solveInPlace(Identity) of the shifted matrix, diagonal case (:100-101)
                    Mmin += delta;
#if defined(DQQ_ADMM_LEAN)
                    if (QP_LIKE) rho = (Mmin > 0.0) ? rho : 0.0;   // `bad`: rho = 0 ends the problem next iteration (above)
                    else badi |= (Mmin > 0.0) ? 0 : 1;   // (an int in a VGPR: a bool live across the region costs three
                                                         // scalar instructions at every join it crosses)
#else
                    bad = bad || !(Mmin > 0.0);
#endif
#pragma unroll
                    for (int e = 0; e < E; ++e) M[e] += delta;
                    rcp_all<E>(M, Minv);
#endif
                }
            }
