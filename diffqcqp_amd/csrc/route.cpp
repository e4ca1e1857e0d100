// route.cpp -- the route plan of every call (route.h).  Routing is a function of (kind, N, B, p_layout) only -- p_layout
// including the caller's hint flags --: two calls with the same arguments launch the same kernels, whatever ran before them,
// on whatever thread or stream.  The library keeps no state.  (The developer build, -DDQQ_TUNING, adds the knobs of tuning.h.)
#include "route.h"

#include "report.h"
#include "tuning.h"
#include "worklist.h"

namespace dqq {

namespace {

constexpr int kAllFlags = DQQ_F_REFERENCE_ORDER | DQQ_F_EXPECT_DENSE | DQQ_F_EXPECT_LONG_LIST;

bool diag_n(int N) { return N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64; }

// Built-in lanes per problem of the diagonal forward, from sweeps on MI355X (tools/probe_lpp_sweep.py; us per forward launch,
// QP / QCQP):
//   N = 8    B = 49152: LPP 4 20.6 / 25.5, LPP 2 23.0 / 28.7;   65536: LPP 2 25.0 / 30.3, LPP 4 27.4 / 34.5;
//            131072: LPP 2 39.9 / 48.0, LPP 4 47.3 / 55.5;      262144: LPP 1 67 / 93, LPP 2 (fused kernel) 66 / 79;
//            1048576: LPP 1 238 / 326, LPP 2 (fused kernel) 222 / 264
//   N = 16   B = 32768: LPP 8 33.3 / 38.4, LPP 4 33.8 / 38.8;   65536: LPP 4 51.2 / 59.6, LPP 2 54.2 / 66.6;
//            262144: LPP 4 150.3 / 169.1, LPP 2 153.6 / 194.4, LPP 8 166.1 / 184.4
//   N = 4    LPP 2 below 131072 problems (32768: 12.6 / 15.6 against 16.4 / 22.2), LPP 1 from there on
// Fewer lanes per problem = fewer instructions per problem (the scalar rho / tau / stop logic and the pow()
// prologue are replicated on every lane of a problem), more lanes = more waves to hide the latency of a small
// batch behind; four coordinates per lane is the sweet spot of a batch that fills the chip (at N = 8 also because
// those tiles re-spread their tails, admm_fwd_diag_respread).
// N >= 32: a wave first streams 32+ KiB of P per problem, and the smaller its tile, the finer that stream
// interleaves with other waves' arithmetic -- the most lanes per problem win at every batch size measured
// (N=32 QP forward, LPP 4 / 8 / 16: B=32768 73 / 68 / 63 us, B=262144 478 / 458 / 442 us; QCQP B=32768
// 84 / 78 / 69 us; N=64 alike).
int default_lpp(int N, int64_t B)
{
    if (N >= 32) return N / 2;
    if (N == 16) return B <= 40960 ? 8 : 4;
    if (N == 8) return B < 57344 ? 4 : 2;
    if (N == 4) return B >= 131072 ? 1 : 2;   // the first of {1, 2} that puts 2048 waves on the chip
    return 1;
}

// The lane layouts fwd_diag.hip instantiates (E = N / LPP coordinates per lane, E even and <= 8): the built-in ones, the
// hint's one lane and DQQ_P_DENSE's N / 2 -- and, behind "fwd_lpp" in the developer build, the others the sweeps compared
// them with.  A requested layout that is not built falls back to the built-in one.
bool lpp_built(int N, int lpp)
{
    switch (N) {
    case 2: return lpp == 1;
    case 4: return lpp == 1 || lpp == 2;
    case 8: return lpp == 1 || lpp == 2 || lpp == 4;
    case 16: return lpp == 4 || lpp == 8 || (kTuning && lpp == 2);
    case 32: return lpp == 16 || (kTuning && (lpp == 4 || lpp == 8));
    case 64: return lpp == 32 || (kTuning && (lpp == 8 || lpp == 16));
    default: return false;
    }
}

Launch fwd_diag(int N, int64_t B, int lpp, bool fuse)
{
    Launch l;
    l.family = Family::FwdDiag;
    l.lpp = lpp_built(N, lpp) ? lpp : default_lpp(N, B);
    l.fuse = fuse;
    return l;
}

// In-kernel solve of non-diagonal tiles (fused) against queueing them for the dense kernel launched behind (work-list),
// forward, us per launch (tools/probe_fuse_n.py; diagonal batch QP / QCQP, then dense batch QP / QCQP):
//   N = 2  B = 131072: fused 14 / 19, 34 / 25, work-list 17 / 21, 53 / 46;  1048576: fused 68 / 87, 154 / 106,
//          work-list 74 / 92, 279 / 271                                      -> fused at every size
//   N = 4  B = 65536: fused 16 / 22, 38 / 38, work-list 17 / 24, 45 / 48;   1048576: fused 122 / 157, 371 / 350,
//          work-list 122 / 162, 321 / 344                                    -> fused up to 131072 problems
//   N = 8  (two lanes per problem, 128 VGPRs either way) B = 131072: fused 40 / 48, 222 / 214, work-list 43 / 50,
//          185 / 182;  1048576: fused 222 / 264, 1396 / 1338, work-list 236 / 278, 1308 / 1237
//          -> fused at every size: the diagonal batch is what DQQ_P_AUTO is for (a batch known to be dense has
//          DQQ_P_DENSE), and it saves the drain launch (2.5-5 us of a 56 us step at the bench shape)
// Only where the fallback solves a whole tile at once (group_dense.h, N <= 8): the per-problem fallback of N = 16
// makes a dense batch 3-10x slower than the work-list route (4096 x 16: 735 vs 81 us), for 3 us saved on a diagonal one.
bool fwd_fuses(int N, int64_t B, int fuse_opt)
{
    if (!fwd_diag_fuses(N)) return false;
    if (fuse_opt >= 0) return fuse_opt != 0;
    return N <= 8 && (N != 4 || B <= 131072);
}

// The backward's in-kernel general routine (dense_core.h dense_bwd_problem) takes the problems of a non-diagonal
// tile one at a time, a whole wave each: a dense batch pays 126 / 467 us (QP / QCQP, 4096 x 8) where the work-list
// route -- one more launch, ~2.5 us when the list is empty, then the team kernel -- takes 19 / 33, and ONE dense
// problem in a tile keeps its wave for the 16 problems of the tile.  A real contact problem's P is dense, so the
// work-list route is the built-in choice at EVERY batch size (round 2 fused for 32 Ki <= B <= 128 Ki -- the bench's
// shape -- and left a 10-100x cliff for a dense P exactly there: VERDICT r2 #3).  The fused form remains behind
// the option fuse_fallback = 1.  The box QP's general routine needs 3N rows of LDS: never fused.
bool bwd_fuses(int kind, int N, int fuse_opt) { return bwd_diag_fuses(N) && kind != kKindBox && fuse_opt > 0; }

// the general (non-diagonal P) path, forward: the first launch of a DQQ_P_DENSE call or the drain of a DQQ_P_AUTO one
Launch general_fwd(int kind, int N, bool ref_order, const Knobs& k)
{
    Launch l;
    if (general_needs_scratch(kind, 0, N, ref_order)) l.family = Family::FwdAny;
    else if ((N == 2 || N == 4 || N == 6 || N == 8) && k.lane_dense != 0) l.family = Family::FwdLane;
    else if ((N == 10 || N == 12 || N == 14 || N == 16) && k.small_fwd != 0) l.family = Family::FwdSmall;
    else if (N > 16 && N <= 64 && !ref_order) l.family = Family::FwdWave64;
    else l.family = Family::FwdLds;
    return l;
}

// ... backward.  list: the drain of a work-list, whose length the caller may have hinted (DQQ_F_EXPECT_LONG_LIST)
Launch general_bwd(int kind, int N, int64_t B, bool ref_order, bool list, int hints, const Knobs& k)
{
    Launch l;
    if (general_needs_scratch(kind, 1, N, ref_order)) {
        l.family = Family::BwdAny;
    } else if (k.lane_bwd != 0 && bwd_lane_fills_chip(kind, N, B) && (!list || (hints & DQQ_F_EXPECT_LONG_LIST) != 0)) {
        // a batch DECLARED dense that fills the chip: a lane per problem (the same bits as the team kernel).  Not in work-list
        // mode unless the list is known to be long: its 512-register waves need an empty SIMD each, and an empty list must
        // cost next to nothing.
        l.family = Family::BwdLane;
        l.lane_mode = list ? 1 : 0;
        if (list) l.counter = Counter::LaneListDrains;
    } else if (k.small_bwd != 0 &&
               (kind == kKindBox ? N == 2 : (kind == kKindQP || kind == kKindQCQP) && N <= 16 && N % 2 == 0)) {
        // (the box QP instantiations, M = 3N, run out of registers from N = 4 on and lose to the run-time sized kernel)
        l.family = Family::BwdSmall;
    } else if (N > 16 && N <= 64 && !ref_order && kind == kKindQP) {
        l.family = Family::BwdChol;
    } else if (N > 16 && N <= 64 && !ref_order && kind == kKindQCQP && N % 2 == 0) {
        // QCQP, 16 < N <= 64: the register-resident block-Cholesky kernels re-associate the sums of these Tikhonov systems
        // (cond(K) ~ 1e9: gradients within 5e-7 / 8e-6 of the reference-order evaluation, the evaluation-order noise of the
        // reference's own formulas); the per-call flag DQQ_F_REFERENCE_ORDER selects the reference-order
        // kernels instead (LDS team kernel up to N = 42, global-memory kernel beyond: 1e-9, 10-30x slower).
        l.family = N <= 32 ? Family::BwdQcqp : Family::BwdQcqpBig;
    } else {
        l.family = Family::BwdTeam;
    }
    return l;
}

} // namespace

int check_call(int kind, int64_t B, int N, int p_layout, int more_flags)
{
    if (B < 0 || N < 1 || B > 0x7fffffffLL) return DQQ_E_BAD_SIZE;
    if (kind == kKindQCQP && (N % 2) != 0) return DQQ_E_BAD_SIZE;
    const int layout = p_layout & 0xff;
    if ((p_layout & ~(0xff | kAllFlags | more_flags)) != 0) return DQQ_E_BAD_LAYOUT;   // unknown flag bits
    if (layout != DQQ_P_AUTO && layout != DQQ_P_DENSE && layout != DQQ_P_DIAG) return DQQ_E_BAD_LAYOUT;
    return 0;
}

Plan plan_fwd(int kind, int N, int64_t B, int p_layout, const Knobs& k)
{
    Plan p;
    const int layout = p_layout & 0xff;
    const bool ref_order = (p_layout & DQQ_F_REFERENCE_ORDER) != 0;
    p.keep = layout == DQQ_P_AUTO && diag_n(N);
    if (B == 0) return p;
    if (layout == DQQ_P_DIAG) {
        if (!diag_n(N)) p.err = DQQ_E_UNSUPPORTED_N;
        else p.first = fwd_diag(N, B, k.fwd_lpp > 0 ? k.fwd_lpp : default_lpp(N, B), false);
        return p;
    }
    if (layout == DQQ_P_DENSE || !diag_n(N)) {
        // DQQ_P_DENSE batches the fused kernel's group solve (group_dense.h) takes from the lane-per-problem kernel: N = 8
        // below 32 Ki problems, where 64 problems per wave leave most of the chip idle (4096 x 8: 44 vs 86 us).  It runs on
        // the general solve's own mapping (N/2 lanes per problem): one pass per tile.
        if (layout == DQQ_P_DENSE && kind < 2 && N == 8 && B <= 32768 && k.lane_dense != 0 && k.fuse_fallback != 0)
            p.first = fwd_diag(N, B, k.fwd_lpp > 0 ? k.fwd_lpp : N / 2, true);
        else
            p.first = general_fwd(kind, N, ref_order, k);
        p.scratch = p.first.family == Family::FwdAny;
        return p;
    }
    // DQQ_P_AUTO: fast path over every tile; non-diagonal tiles are solved inside it (small N) or queued for the general
    // kernel launched right behind it
    p.worklist = true;
    const bool fuse = fwd_fuses(N, B, k.fuse_fallback);
    int lpp = k.fwd_lpp > 0 ? k.fwd_lpp : default_lpp(N, B);
    Counter counter = Counter::None;
    // A DQQ_P_AUTO batch the caller expects to be half or more non-diagonal (DQQ_F_EXPECT_DENSE: dqq_hint_flags from the
    // report word of the last backward, report.h) runs on ONE lane per problem: the general solve with a problem's whole matrix
    // in its lane's registers instead of four lanes exchanging rows (65536 x 8 all non-diagonal, forward: QP 106 -> 65 us,
    // QCQP 116 -> 84; one problem in 10: 95 -> 68, 109 -> 82; tools/probe_sparse_dense_lpp.py).  Below that share two
    // lanes stay: since non-diagonal problems are handed to the general solve one by one (fwd_diag_kernel), a sparse
    // few cost one pass of it per affected 16-problem block -- one in 1000: 46 / 52 us, what four lanes per problem took.
    // The same bits either way: neither the diagonal arithmetic nor the general solve depends on the lane layout, and
    // which of the two a problem gets depends on the problem alone.
    if (k.fwd_lpp <= 0 && fuse && N == 8 && kind < 2 && lpp == 2 && k.fwd_feedback != 0 &&
        (p_layout & DQQ_F_EXPECT_DENSE) != 0) {
        lpp = 1;
        counter = Counter::FwdFeedbackRoutes;
    }
    p.first = fwd_diag(N, B, lpp, fuse);
    p.first.counter = counter;
    if (!fuse) p.drain = general_fwd(kind, N, ref_order, k);
    p.scratch = p.drain.family == Family::FwdAny;
    return p;
}

// Every forward family has a warm form (the kernels carry x0 as a template parameter or as a kernel-uniform branch of their
// prologue), so the warm plan is the cold one: the same families, lanes, fused / drained split, counters and
// scratch, and the hint flags and DQQ_F_REFERENCE_ORDER mean what they mean there.  A family WITHOUT a warm form would go to
// the LDS wave kernel (N <= 64: every kind, any N) or to the global-memory kernel here, never to a refusal: no (kind, N,
// layout) the cold forward accepts is refused.
bool fwd_family_warm(Family f)
{
    switch (f) {
    case Family::FwdDiag: case Family::FwdLane: case Family::FwdSmall: case Family::FwdWave64: case Family::FwdLds:
    case Family::FwdAny: return true;
    default: return false;
    }
}

Plan plan_fwd_warm(int kind, int N, int64_t B, int p_layout, const Knobs& k)
{
    Plan p = plan_fwd(kind, N, B, p_layout, k);
    const bool ref_order = (p_layout & DQQ_F_REFERENCE_ORDER) != 0;
    Launch* const both[2] = {&p.first, &p.drain};
    for (Launch* l : both) {
        if (l->family == Family::None || fwd_family_warm(l->family)) continue;
        l->family = general_needs_scratch(kind, 0, N, ref_order) ? Family::FwdAny : Family::FwdLds;   // (not reached today)
        l->lpp = 0;
        l->fuse = false;
        l->counter = Counter::None;
    }
    return p;
}

Plan plan_bwd(int kind, int N, int64_t B, int p_layout, const Knobs& k)
{
    // the signed box QP's backward is the box QP's on other bounds (sbox_bounds.h): the same families, the same drain, no
    // hints, never fused -- routed as kind 2; the launchers get the caller's kind and pick the signed instantiation
    if (kind == kKindSignedBox) kind = kKindBox;
    Plan p;
    const int layout = p_layout & 0xff;
    const bool ref_order = (p_layout & DQQ_F_REFERENCE_ORDER) != 0;
    const int hints = kind == kKindBox ? 0 : p_layout & (DQQ_F_EXPECT_DENSE | DQQ_F_EXPECT_LONG_LIST);   // (box QP: none)
    if (B == 0) return p;
    if (layout == DQQ_P_DIAG) {
        if (!diag_n(N)) p.err = DQQ_E_UNSUPPORTED_N;
        else p.first.family = Family::BwdDiag;
        return p;
    }
    if (layout == DQQ_P_DENSE || !diag_n(N)) {
        p.first = general_bwd(kind, N, B, ref_order, false, hints, k);
        p.scratch = p.first.family == Family::BwdAny;
        return p;
    }
    p.worklist = true;
    if (bwd_fuses(kind, N, k.fuse_fallback)) {
        p.first.family = Family::BwdDiag;
        p.first.fuse = true;
        return p;
    }
    // the caller expects all of it non-diagonal (DQQ_F_EXPECT_DENSE, dqq_hint_flags: three quarters of the batch or more
    // queued, twice running): one launch of the lane kernel over everything costs what its waves cost (B / 64 of them,
    // whatever their problems are) and recounts for the caller's next hint (a diagonal problem gets the same bits there);
    // classifying first costs a launch that queues the entries through one atomic per workgroup (14 us per 65536) plus the
    // same waves for the queued part
    if (k.lane_bwd != 0 && k.bwd_skip_classify != 0 && bwd_lane_fills_chip(kind, N, B) && (hints & DQQ_F_EXPECT_DENSE) != 0) {
        p.first.family = Family::BwdLane;
        p.first.lane_mode = 2;
        p.first.counter = Counter::BwdWholeBatches;
        return p;
    }
    p.first.family = Family::BwdDiag;
    p.drain = general_bwd(kind, N, B, ref_order, true, hints, k);
    p.scratch = p.drain.family == Family::BwdAny;
    return p;
}

CheckPlan plan_check(int kind, int N, int64_t B, int p_layout)
{
    CheckPlan p;
    if (kind < kKindQP || kind > kKindSignedBox) p.err = DQQ_E_BAD_KIND;
    else p.err = check_call(kind, B, N, p_layout);
    if (p.err != 0 || B == 0) return p;
    p.family = (p_layout & 0xff) == DQQ_P_DIAG ? Family::CheckDiag : Family::Check;
    p.lanes = check_lanes(N);
    return p;
}

JvpPlan plan_jvp(int kind, int N, int64_t B, int p_layout)
{
    JvpPlan p;
    if (kind < kKindQP || kind > kKindSignedBox) p.err = DQQ_E_BAD_KIND;
    else p.err = check_call(kind, B, N, p_layout);
    if (p.err != 0 || B == 0) return p;
    if ((p_layout & 0xff) == DQQ_P_DIAG) {
        if (!diag_n(N)) p.err = DQQ_E_UNSUPPORTED_N;
        else p.family = Family::JvpDiag;
        return p;
    }
    // DQQ_P_AUTO is not classified: the general kernel is correct on a diagonal P too
    p.scratch = general_needs_scratch(kind, 1, N, true);
    p.family = p.scratch ? Family::JvpAny : Family::JvpTeam;
    return p;
}

// The Newton family's table (route.h): a group's diagonal, team and any-N family, in NewtonGroup's order
static constexpr Family kNewtonFamilies[9][3] = {
    {Family::PolishDiag, Family::PolishTeam, Family::PolishAny},
    {Family::PolishLsDiag, Family::PolishLsTeam, Family::PolishLsAny},
    {Family::NewtonDiag, Family::NewtonTeam, Family::NewtonAny},
    {Family::NewtonJacDiag, Family::NewtonJacTeam, Family::NewtonJacAny},
    {Family::ActiveDiag, Family::ActiveTeam, Family::ActiveAny},
    {Family::PolishSmoothDiag, Family::PolishSmoothTeam, Family::PolishSmoothAny},
    {Family::NewtonSmoothDiag, Family::NewtonSmoothTeam, Family::NewtonSmoothAny},
    {Family::PolishPathDiag, Family::PolishPathTeam, Family::PolishPathAny},
    {Family::NewtonJacSmoothDiag, Family::NewtonJacSmoothTeam, Family::NewtonJacSmoothAny},
};
static_assert(kPolishTeamMaxN == kNewtonTeamMaxN, "one team kernel limit for the family");

NewtonFamilyPlan plan_newton_family(NewtonGroup group, int kind, int N, int64_t B, int p_layout, bool inf_flag)
{
    NewtonFamilyPlan p;
    if (kind < kKindQP || kind > kKindSignedBox) p.err = DQQ_E_BAD_KIND;
    else p.err = check_call(kind, B, N, p_layout, inf_flag ? newton_family_flags(kind) : 0);
    p.inf_bounds = p.err == 0 && inf_flag && plan_inf_bounds(kind, p_layout);
    if (p.err != 0 || B == 0) return p;
    if ((p_layout & 0xff) == DQQ_P_DIAG) {
        if (!diag_n(N)) p.err = DQQ_E_UNSUPPORTED_N;
        else p.route = NewtonRoute::Diag;
    } else {
        // DQQ_P_AUTO is not classified: the general kernel gives the diagonal kernel's bits on (the blocks of) a diagonal P
        p.route = N > kNewtonTeamMaxN ? NewtonRoute::Any : NewtonRoute::Team;
        p.scratch = p.route == NewtonRoute::Any && group != NewtonGroup::Active;
    }
    if (p.route != NewtonRoute::None) p.family = kNewtonFamilies[(int)group][(int)p.route - 1];
    return p;
}

PolishPlan plan_polish(int kind, int N, int64_t B, int p_layout) { return plan_newton_family(NewtonGroup::Polish, kind, N, B, p_layout); }
NewtonPlan plan_newton(int kind, int N, int64_t B, int p_layout) { return plan_newton_family(NewtonGroup::Derivative, kind, N, B, p_layout); }
NewtonJacPlan plan_newton_jac(int kind, int N, int64_t B, int p_layout)
{
    return plan_newton_family(NewtonGroup::Jacobian, kind, N, B, p_layout);
}
NewtonActivePlan plan_newton_active(int kind, int N, int64_t B, int p_layout)
{
    return plan_newton_family(NewtonGroup::Active, kind, N, B, p_layout);
}

// the parent's plan with the proximal weight looked at (route.h)
static NewtonFamilyPlan with_reg(NewtonFamilyPlan p, double reg)
{
    if ((p.err == 0 || p.err == DQQ_E_UNSUPPORTED_N) && !reg_ok(reg)) {
        p = NewtonFamilyPlan{};
        p.err = DQQ_E_BAD_SIZE;
        return p;
    }
    p.reg = p.err == 0 && p.family != Family::None && reg != 0.0;
    return p;
}

PolishPlan plan_polish_reg(int kind, int N, int64_t B, int p_layout, double reg) { return with_reg(plan_polish(kind, N, B, p_layout), reg); }
NewtonPlan plan_newton_reg(int kind, int N, int64_t B, int p_layout, double reg) { return with_reg(plan_newton(kind, N, B, p_layout), reg); }
NewtonJacPlan plan_newton_jac_reg(int kind, int N, int64_t B, int p_layout, double reg)
{
    return with_reg(plan_newton_jac(kind, N, B, p_layout), reg);
}

PolishPlan plan_polish_ls(int kind, int N, int64_t B, int p_layout, double reg, int max_halvings)
{
    PolishPlan p = with_reg(plan_newton_family(NewtonGroup::PolishLs, kind, N, B, p_layout), reg);
    if ((p.err == 0 || p.err == DQQ_E_UNSUPPORTED_N) && (max_halvings < 0 || max_halvings > kPolishMaxHalvings)) {
        p = PolishPlan{};
        p.err = DQQ_E_BAD_OPTION;
    }
    return p;
}

// the smoothed entries (route.h): the parent's plan, on the smoothed families where kappa is not a zero
static NewtonFamilyPlan with_kappa(NewtonFamilyPlan p, double kappa, bool option_bad)
{
    if ((p.err == 0 || p.err == DQQ_E_UNSUPPORTED_N) && (option_bad || !kappa_ok(kappa))) {
        p = NewtonFamilyPlan{};
        p.err = DQQ_E_BAD_OPTION;
        return p;
    }
    p.smooth = p.err == 0 && p.family != Family::None && kappa != 0.0;
    return p;
}

PolishPlan plan_polish_smooth(int kind, int N, int64_t B, int p_layout, double reg, int max_halvings, double kappa)
{
    const NewtonGroup g = kappa != 0.0 ? NewtonGroup::PolishSmooth : NewtonGroup::PolishLs;
    return with_kappa(with_reg(plan_newton_family(g, kind, N, B, p_layout, false), reg), kappa,
                      max_halvings < 0 || max_halvings > kPolishMaxHalvings);
}

NewtonPlan plan_newton_smooth(int kind, int N, int64_t B, int p_layout, double reg, double kappa)
{
    const NewtonGroup g = kappa != 0.0 ? NewtonGroup::DerivativeSmooth : NewtonGroup::Derivative;
    return with_kappa(with_reg(plan_newton_family(g, kind, N, B, p_layout, false), reg), kappa, false);
}

NewtonJacPlan plan_newton_jac_smooth(int kind, int N, int64_t B, int p_layout, double reg, double kappa)
{
    const NewtonGroup g = kappa != 0.0 ? NewtonGroup::JacobianSmooth : NewtonGroup::Jacobian;
    return with_kappa(with_reg(plan_newton_family(g, kind, N, B, p_layout, false), reg), kappa, false);
}

// the polish path (route.h): the smoothed polish's plan on the path's families, and the schedule's own errors
PolishPlan plan_polish_path(int kind, int N, int64_t B, int p_layout, double reg, const double* kappas, const int* stage_steps,
                            int n_stages, int max_halvings)
{
    PolishPlan p = with_reg(plan_newton_family(NewtonGroup::PolishPath, kind, N, B, p_layout, false), reg);
    if (p.err != 0 && p.err != DQQ_E_UNSUPPORTED_N) return p;
    int err = 0;
    if (n_stages < 1 || n_stages > kPolishPathMaxStages || max_halvings < 0 || max_halvings > kPolishMaxHalvings) err = DQQ_E_BAD_OPTION;
    else if (kappas == nullptr || stage_steps == nullptr) err = DQQ_E_NULLPTR;
    else
        for (int s = 0; s < n_stages; ++s)
            if (!kappa_ok(kappas[s]) || stage_steps[s] < 0) err = DQQ_E_BAD_OPTION;
    if (err != 0) {
        p = PolishPlan{};
        p.err = err;
    }
    return p;
}

// The largest N of the register / LDS kernels (64 rows): the forward's N, the QCQP backward's N + N/2 (with the reference's
// order; the register-resident kernels hold N = 64), the box QP backward's 3N.
int max_n(int which, bool ref_order)
{
    if (which == 2) return ref_order ? 42 : 64;
    if (which == 3) return 21;
    return 64;
}

// The scratch a call demands is the scratch the kernels it launches use: the plans above send a problem of the general path
// to the global-memory kernels exactly when this holds (the default route of QCQP 42 < N <= 64 once demanded
// 46 MB it never touched).
bool general_needs_scratch(int kind, int pass, int N, bool ref_order)
{
    const int which = pass == 0 ? (kind == kKindQCQP ? 1 : 0) : (kind == kKindQP ? 0 : (kind == kKindQCQP ? 2 : 3));
    return N > max_n(which, ref_order);
}

// P declared dense, QP / QCQP, N = 2, 4, 6, 8, batches that fill the chip: a lane per problem needs 64 problems per wave
// and a wave per SIMD, below that the team kernel's 4 to 8 problems per wave spread a batch better.  Backward, us, team
// / lane (tools/probe_lane_bwd.py --sweep):   QCQP N = 8: B = 16384 34 / 35, 24576 49 / 34, 32768 64 / 42, 65536 117 / 86,
// 131072 221 / 140;  QCQP N = 6: 16384 25 / 20, 65536 79 / 26, 131072 146 / 48;  QP N = 8: 16384 20 / 19, 32768 24 / 14,
// 65536 37 / 22, 131072 68 / 42;  QP N = 6: 65536 21 / 12;  N <= 4: launch-bound up to 65536, 131072: 46 / 25 (QCQP N = 4)
bool bwd_lane_fills_chip(int kind, int N, int64_t B)
{
    const int64_t min_b = (N == 8) ? 24576 : 16384;
    return (kind == kKindQP || kind == kKindQCQP) && (N == 2 || N == 4 || N == 6 || N == 8) && B >= min_b;
}

int hint_flags(int kind, int pass, int N, int64_t B, unsigned long long last_report)
{
    // pure: the flags a caller may OR into p_layout for a call of (kind, pass, N, B) when the last backward of that kind and N
    // left `last_report` in the caller's report word (report.h).  0 whenever the word says nothing about such a batch.
    if (!hint_applies(kind, N) || B <= 0 || (pass != 0 && pass != 1)) return 0;
    int flags = 0;
    if (pass == 0) {
        // forward, N = 8: half of the batch or more sat in 16-problem blocks with a non-diagonal problem
        if (N == 8 && 2 * report_count_in_blocks(last_report, (long)B) >= B) flags |= DQQ_F_EXPECT_DENSE;
        return flags;
    }
    if (!bwd_lane_fills_chip(kind, N, (long)B)) return 0;
    int streak = 0;
    const long c = report_count(last_report, (long)B, &streak);
    if (4 * c >= 3 * B && streak >= 1) flags |= DQQ_F_EXPECT_DENSE;         // all non-diagonal, twice running
    if (bwd_lane_fills_chip(kind, N, c)) flags |= DQQ_F_EXPECT_LONG_LIST; // a list that fills the chip
    return flags;
}

size_t workspace_bytes(int64_t B)
{
    if (B < 0) B = 0;
    // header + the entry area: B slots of the plain list, or the 32 segments of the N >= 32 list (worklist.h)
    size_t n = (size_t)kWsEntries + (size_t)kWsEntryInts((long)B);
    n = (n + 63) & ~(size_t)63;
    return n * sizeof(int);
}

bool scratch_applies(int kind, int pass, int N, int64_t B, int p_layout)
{
    if (B <= 0 || N < 1 || kind < 0 || kind > 3 || (pass != 0 && pass != 1)) return false;
    // dqq_signedboxqp_bwd_f64 came after this query: it takes the box QP's scratch, dqq_scratch_bytes(2, 1, ...), and
    // (3, 1, ...) keeps answering 0 as it did when the kind had no backward
    if (pass == 1 && kind == kKindSignedBox) return false;
    return general_needs_scratch(kind, pass, N, (p_layout & DQQ_F_REFERENCE_ORDER) != 0);
}

} // namespace dqq
