// exact_divisor_check.cpp -- TEST ARTEFACT (a program of its own, driven by tests/test_exact_divisor_hostcore.py).
//
// 1. csrc/common.h: ExactDivisorT -- the device's text, compiled for the host with a MODEL of the hardware's reciprocal
//    estimate as its seed -- against the host's `/`, bit for bit.  Seed models: the correctly rounded reciprocal moved by
//    -1, 0, +1 ulp (modes 0..2), and, wider than anything the instruction returns, the reciprocal rounded to float
//    precision moved by -1, 0, +1 float ulp (modes 3..5: a relative error of 2^-24, the figure common.h quotes for the
//    hardware's estimate).
// 2. csrc/kkt_core.h: QcqpContact as it is now -- with the host's plain divider and with the device's divider on every
//    seed model -- against the struct as it was before the divider existed (OldQcqpContact below, verbatim), member by
//    member after setup and after each of three steps.
// Prints one line per check: "<name> <cases> <certified-fast cases> <mismatches>"; exit status 1 if anything mismatched.
#include "../../diffqcqp_amd/csrc/kkt_core.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace dqq;

static uint64_t bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }
static double from_bits(uint64_t b) { double v; memcpy(&v, &b, 8); return v; }
static bool same(double a, double b) { return bits(a) == bits(b); }

struct Rng {   // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * 0x1p-53; }                 // [0, 1)
    double uni(double a, double b) { return a + (b - a) * uni(); }
    // sign and mantissa uniform, biased exponent uniform in [elo, ehi] (0 = subnormals): log-uniform magnitudes
    double logu(int elo, int ehi) { const uint64_t r = next(); const uint64_t e = (uint64_t)elo + next() % (uint64_t)(ehi - elo + 1); return from_bits((r & 0x800fffffffffffffull) | (e << 52)); }
};

// ---- models of the reciprocal estimate
template <int MODE>
struct ModelSeed {
    static double rcp(double d)
    {
        double y = 1.0 / d;
        if (!(fabs(y) > 0x1p-1000 && fabs(y) < 0x1p1000)) return y;          // 0, inf, NaN, near the ends: as they are
        if (MODE < 3) {
            const int k = MODE - 1;
            return k < 0 ? nextafter(y, 0.0) : (k > 0 ? nextafter(y, y * 2) : y);
        }
        if (!(fabs(y) > 0x1p-100 && fabs(y) < 0x1p100)) return y;            // outside float's range: the exact one
        float f = (float)y;
        const int k = MODE - 4;
        f = k < 0 ? nextafterf(f, 0.0f) : (k > 0 ? nextafterf(f, f * 2) : f);
        return (double)f;
    }
};

static long g_cases, g_fast, g_bad;
static int g_shown;

template <int MODE>
static void check_pair(double n, double d)
{
    ModerateRange rg;
    const ExactDivisorT<ModelSeed<MODE>> dv(d, rg);
    const double got = div(n, dv), want = n / d;
    dv.quotient(n, rg);
    g_cases++;
    if (rg.moderate()) g_fast++;
    if (!same(got, want)) {
        g_bad++;
        if (g_shown++ < 10) printf("# mode %d: %a / %a = %a, got %a\n", MODE, n, d, want, got);
    }
}
static void check_pair_all(double n, double d)
{
    check_pair<0>(n, d); check_pair<1>(n, d); check_pair<2>(n, d);
    check_pair<3>(n, d); check_pair<4>(n, d); check_pair<5>(n, d);
}
static int report(const char* name)
{
    printf("%s %ld %ld %ld\n", name, g_cases, g_fast, g_bad);
    const int bad = g_bad != 0;
    g_cases = g_fast = g_bad = 0;
    return bad;
}

static std::vector<double> edge_values()
{
    const double ulp1 = 0x1p-52;
    std::vector<double> v = {0.0, 0x1p-1074, from_bits(0x000fffffffffffffull), 0x1p-1022, 1.0 - ulp1 / 2, 1.0, 1.0 + ulp1,
                             from_bits(0x7fefffffffffffffull), INFINITY, 3.0, 1.0 / 3.0, 0.1, from_bits(0x3fffffffffffffffull)};
    for (int e = -1074; e <= 1023; e += 37) v.push_back(ldexp(1.0, e));
    // around the limits of ModerateRange and of the numerators it admits
    for (int e : {-602, -601, -600, -301, -300, -299, -1, 1, 299, 300, 301, 600, 601, 602, 1023})
        for (double m : {1.0, 1.5, from_bits(0x3fffffffffffffffull) / 2 * 1.0}) v.push_back(ldexp(m, e));
    // just below and above a power of two: where the reciprocal lies closest to a rounding boundary
    for (int k = 1; k < 32; k += 2) { v.push_back(2.0 - k * ulp1); v.push_back(1.0 + k * ulp1); }
    const size_t n = v.size();
    for (size_t i = 0; i < n; ++i) v.push_back(-v[i]);
    v.push_back(NAN);
    v.push_back(-NAN);
    return v;
}

// ---- the struct before ExactDivisor: verbatim
struct OldQcqpContact {
    bool act;          // in the derivative system's active set (Solver.cpp:639)
    double gamma;      // dual of the contact (0 when inactive), dualFromPrimalQCQP
    double K[3][3], Kinv[3][3], Ab[3], KinvAb[3], xs[3]; // order: gamma, a, b

    DQQ_HD void setup(double pa, double pb, double qa, double qb, double xa, double xb, double ga, double gb,
                      double l_n, double mu, double eps = kActiveEps)
    {
        // bwd_systems.h: qcqp_contact for a diagonal P, written out (a call reorders bwd_diag_kernel<1, ..>)
        const double r = l_n * mu;                             // pybindings.cpp:65
        // ---- dualFromPrimalQCQP, Solver.cpp:584-617 (epsilon: pybindings.cpp:62, default 1e-10)
        {
            const double slack = r + -sqrt(xa * xa + xb * xb); // :594-597
            gamma = 0.0;
            if (!(slack > eps || r < eps)) {                   // :598-604
                const double ca = 2 * xa, cb = 2 * xb;         // A(2i,i), A(2i+1,i), :589-592
                const double G = ca * ca + cb * cb;            // A~^T A~ (diagonal)
                const double pla = pa * xa + qa, plb = pb * xb + qb; // P l + q
                const double rhs = ca * pla + cb * plb;        // A~^T (P l + q)
                const double L = sqrt(G);                      // llt().solve, :611
                gamma = -((rhs / L) / L);
            }
        }
        // ---- solveDerivativesQCQP, Solver.cpp:619-681
        double S = -(r * r);                                   // :622
        S = S + (xa * xa + xb * xb);                           // :628-629
        act = S > -kActiveEps && r > kActiveEps;               // :637-641
        const double ca = 2 * xa, cb = 2 * xb;                 // C, :630-631
        const double Da = 2 * gamma + pa, Db = 2 * gamma + pb; // D_tild + P, :632-633, :651
        xs[0] = xs[1] = xs[2] = 0.0;
        if (act) {
            const double Ba = gamma * ca, Bb = gamma * cb;     // diag(gamma) C^T, :644
            // A (before transposeInPlace) = [[S,Ba,Bb],[ca,Da,0],[cb,0,Db]]; b = [0,ga,gb]
            Ab[0] = Ba * ga + Bb * gb;                         // A^T_t b = A b, :19
            Ab[1] = Da * ga;
            Ab[2] = Db * gb;
            K[0][0] = (S * S + Ba * Ba) + Bb * Bb + kMuIr;     // A_t^T A_t + mu_ir I, :20-21
            K[0][1] = K[1][0] = S * ca + Ba * Da;
            K[0][2] = K[2][0] = S * cb + Bb * Db;
            K[1][1] = ca * ca + Da * Da + kMuIr;
            K[1][2] = K[2][1] = ca * cb;
            K[2][2] = cb * cb + Db * Db + kMuIr;
            // lower Cholesky, :23
            const double L00 = sqrt(K[0][0]);
            const double L10 = K[1][0] / L00, L20 = K[2][0] / L00;
            const double L11 = sqrt(K[1][1] - L10 * L10);
            const double L21 = (K[2][1] - L20 * L10) / L11;
            const double L22 = sqrt(K[2][2] - (L20 * L20 + L21 * L21));
            // solveInPlace(Identity): L y = e_c then L^T x = y, column by column
            {   // column 0
                const double y0 = 1.0 / L00, y1 = (0.0 - L10 * y0) / L11, y2 = ((0.0 - L20 * y0) - L21 * y1) / L22;
                const double x2 = y2 / L22, x1 = (y1 - L21 * x2) / L11, x0 = ((y0 - L10 * x1) - L20 * x2) / L00;
                Kinv[0][0] = x0; Kinv[1][0] = x1; Kinv[2][0] = x2;
            }
            {   // column 1
                const double y1 = 1.0 / L11, y2 = (0.0 - L21 * y1) / L22;
                const double x2 = y2 / L22, x1 = (y1 - L21 * x2) / L11, x0 = ((0.0 - L10 * x1) - L20 * x2) / L00;
                Kinv[0][1] = x0; Kinv[1][1] = x1; Kinv[2][1] = x2;
            }
            {   // column 2
                const double y2 = 1.0 / L22;
                const double x2 = y2 / L22, x1 = (0.0 - L21 * x2) / L11, x0 = ((0.0 - L10 * x1) - L20 * x2) / L00;
                Kinv[0][2] = x0; Kinv[1][2] = x1; Kinv[2][2] = x2;
            }
            for (int i = 0; i < 3; ++i)
                KinvAb[i] = (Kinv[i][0] * Ab[0] + Kinv[i][1] * Ab[1]) + Kinv[i][2] * Ab[2]; // :27
        } else {
            // the contact's two coordinates are 1x1 blocks of D_tild + P
            const double D[2] = {Da, Db}, g[2] = {ga, gb};
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) K[i][j] = Kinv[i][j] = 0.0;
            Ab[0] = KinvAb[0] = 0.0;
            for (int i = 0; i < 2; ++i) {
                Ab[i + 1] = D[i] * g[i];
                K[i + 1][i + 1] = D[i] * D[i] + kMuIr;
                const double L = sqrt(K[i + 1][i + 1]);
                Kinv[i + 1][i + 1] = (1.0 / L) / L;
                KinvAb[i + 1] = Kinv[i + 1][i + 1] * Ab[i + 1];
            }
        }
    }

    // one refinement step (:29-31); dsq = squared residual entries (gamma, a, b)
    DQQ_HD void step(double (&dsq)[3])
    {
        if (act) {
            double t[3];
            for (int i = 0; i < 3; ++i) t[i] = (Kinv[i][0] * xs[0] + Kinv[i][1] * xs[1]) + Kinv[i][2] * xs[2];
            for (int i = 0; i < 3; ++i) xs[i] = kMuIr * t[i] + KinvAb[i];
            for (int i = 0; i < 3; ++i) {
                const double d = ((K[i][0] * xs[0] + K[i][1] * xs[1]) + K[i][2] * xs[2]) - Ab[i];
                dsq[i] = d * d;
            }
        } else {
            dsq[0] = 0.0;
            for (int i = 1; i < 3; ++i) {
                const double t = Kinv[i][i] * xs[i];
                xs[i] = kMuIr * t + KinvAb[i];
                const double d = K[i][i] * xs[i] - Ab[i];
                dsq[i] = d * d;
            }
        }
    }
    DQQ_HD double dgamma() const { return act ? xs[0] : 0.0; }  // :671-674
    DQQ_HD double dla() const { return xs[1]; }
    DQQ_HD double dlb() const { return xs[2]; }
};

// ---- contacts of the benchmark's distribution: p ~ U(0.1, 1.1), l_n, mu ~ U(0, 1); x a solution of the contact's problem
// for some q -- on the cone's boundary with a positive multiplier (active) or strictly inside (inactive)
struct Contact { double pa, pb, qa, qb, xa, xb, ga, gb, ln, mu; };

static Contact bench_contact(Rng& r, bool active)
{
    Contact c;
    c.pa = r.uni(0.1, 1.1); c.pb = r.uni(0.1, 1.1);
    c.ln = r.uni(); c.mu = r.uni();
    const double rad = c.ln * c.mu, th = r.uni(0.0, 6.283185307179586), rho = active ? 1.0 : r.uni(0.0, 0.9);
    c.xa = rho * rad * cos(th); c.xb = rho * rad * sin(th);
    const double gam = active ? r.uni(0.0, 2.0) : 0.0;
    c.qa = -(c.pa * c.xa) - 2 * gam * c.xa;   // stationarity: P x + q + 2 gamma x = 0
    c.qb = -(c.pb * c.xb) - 2 * gam * c.xb;
    c.ga = r.uni(-1.0, 1.0); c.gb = r.uni(-1.0, 1.0);
    return c;
}
// the same with what the fast division must hand back to the plain one: zeros, huge and tiny scales, NaN
static Contact odd_contact(Rng& r, long i)
{
    Contact c = bench_contact(r, (i & 1) != 0);
    switch ((i >> 1) % 8) {
    case 0: c.xa = 0.0; c.qa = 0.0; break;                       // zero numerators (K[2][1] = ca cb = 0)
    case 1: c.xb = -0.0; c.qb = 0.0; break;
    case 2: c.ga = 0.0; c.gb = -0.0; break;
    case 3: c.pa *= 0x1p400; c.qa *= 0x1p400; break;              // denominators beyond 2^300
    case 4: c.pa *= 0x1p-400; c.pb *= 0x1p-400; c.qa *= 0x1p-400; c.qb *= 0x1p-400; break;
    case 5: c.ga *= 0x1p-700; c.gb *= 0x1p700; break;
    case 6: c.qa = NAN; break;
    default: c.ln *= 1e-6; c.xa *= 1e-6; c.xb *= 1e-6; break;     // a cone radius near the active-set thresholds
    }
    return c;
}

// a divider for QcqpContact::setup that checks every (numerator, denominator) pair it is given, on every seed model
struct PairCheckingDen {
    double den;
    PairCheckingDen(double d, ModerateRange&) : den(d) {}
    double operator()(double n, ModerateRange&) const { check_pair_all(n, den); return n / den; }
};

template <class A, class B>
static bool members_equal(const A& a, const B& b)
{
    if (a.act != b.act || !same(a.gamma, b.gamma)) return false;
    bool eq = true;
    for (int i = 0; i < 3; ++i) eq = eq && same(a.xs[i], b.xs[i]);
    for (int i = a.act ? 0 : 1; i < 3; ++i) {                     // an inactive contact carries entries [1][1], [2][2] only
        eq = eq && same(a.Ab[i], b.Ab[i]) && same(a.KinvAb[i], b.KinvAb[i]);
        for (int j = a.act ? 0 : i; j < (a.act ? 3 : i + 1); ++j) eq = eq && same(a.K[i][j], b.K[i][j]) && same(a.Kinv[i][j], b.Kinv[i][j]);
    }
    return eq && same(a.dgamma(), b.dgamma()) && same(a.dla(), b.dla()) && same(a.dlb(), b.dlb());
}

template <class Shared>
static void compare_contact(const Contact& c, long& n_act)
{
    OldQcqpContact o;
    QcqpContact n;
    o.setup(c.pa, c.pb, c.qa, c.qb, c.xa, c.xb, c.ga, c.gb, c.ln, c.mu);
    n.template setup<Shared>(c.pa, c.pb, c.qa, c.qb, c.xa, c.xb, c.ga, c.gb, c.ln, c.mu);
    bool eq = members_equal(o, n);
    for (int it = 0; it < 3; ++it) {
        double d0[3], d1[3];
        o.step(d0);
        n.step(d1);
        eq = eq && members_equal(o, n) && same(d0[0], d1[0]) && same(d0[1], d1[1]) && same(d0[2], d1[2]);
    }
    g_cases++;
    if (o.act) n_act++;
    if (!eq) {
        g_bad++;
        if (g_shown++ < 10) printf("# contact differs: p %a %a q %a %a x %a %a g %a %a l_n %a mu %a\n", c.pa, c.pb, c.qa, c.qb, c.xa, c.xb, c.ga, c.gb, c.ln, c.mu);
    }
}
template <int MODE>
using ModelDen = SharedDen<ExactDivisorT<ModelSeed<MODE>>>;

static void compare_contact_all(const Contact& c, long& n_act)
{
    compare_contact<SharedDen<ExactDivisor>>(c, n_act);           // the host's own build of the struct
    compare_contact<ModelDen<0>>(c, n_act); compare_contact<ModelDen<1>>(c, n_act); compare_contact<ModelDen<2>>(c, n_act);
    compare_contact<ModelDen<3>>(c, n_act); compare_contact<ModelDen<4>>(c, n_act); compare_contact<ModelDen<5>>(c, n_act);
}

int main(int argc, char** argv)
{
    const std::string what = argc > 1 ? argv[1] : "all";
    const long scale = argc > 2 ? atol(argv[2]) : 1;             // divides the random counts (quick local runs)
    int bad = 0;
    Rng r{20261019};
    if (what == "all" || what == "divisor") {
        for (long i = 0; i < 10000000 / scale; ++i) check_pair_all(r.logu(0, 2046), r.logu(0, 2046));
        bad |= report("random_full_range");
        for (long i = 0; i < 10000000 / scale; ++i) check_pair_all(r.logu(1023 - 640, 1023 + 640), r.logu(1023 - 320, 1023 + 320));
        bad |= report("random_around_the_certified_range");
        const std::vector<double> e = edge_values();
        for (double n : e) for (double d : e) check_pair_all(n, d);
        bad |= report("edge_values");
        long pairs = 0;
        for (long i = 0; pairs < 1000000 / scale; ++i) {
            const Contact c = bench_contact(r, (i & 1) != 0);
            QcqpContact ct;
            ct.setup<PairCheckingDen>(c.pa, c.pb, c.qa, c.qb, c.xa, c.xb, c.ga, c.gb, c.ln, c.mu);
            pairs = g_cases / 6;
        }
        bad |= report("bench_kkt_pairs");
    }
    if (what == "all" || what == "contact") {
        long n_act = 0;
        for (long i = 0; i < 100000 / scale; ++i) compare_contact_all(bench_contact(r, (i & 1) != 0), n_act);
        printf("contact_active_share %ld\n", n_act);
        bad |= report("bench_contacts");
        n_act = 0;
        for (long i = 0; i < 100000 / scale; ++i) compare_contact_all(odd_contact(r, i), n_act);
        printf("odd_contact_active_share %ld\n", n_act);
        bad |= report("odd_contacts");
    }
    return bad;
}
