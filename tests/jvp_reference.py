"""numpy restatement of the implicit-function derivatives in BOTH modes, built on the backward's systems (not a test file).

`derivative(kind, ..., mode="bwd")` is the backward of include/diffqcqp_hip.h: duals and active sets from x, the matrix At and
right-hand side rhs(g) of diffqcqp_amd/csrc/bwd_systems.h, b = iterative_refinement(At, rhs(g)), the gradients R(b).
`mode="jvp"` is dqq_jvp_f64: s = R^T(tangents), w = iterative_refinement(At^T, s), dx = rhs^T(w) -- the same matrix, the same
refinement routine, the same placements read the other way round.  tests/test_jvp_reference.py pins the first mode bit-equal to
the oracle's backward, which pins the matrix, the placements and the refinement the second mode shares.

Every sum runs in index order, one rounding per operation (numpy never contracts a * b + c): the arithmetic of the oracle and
of the reference-order kernels.  One problem per call; vectors are 1-d."""
import numpy as np

MU_IR, IR_EPS, IR_MAX, ACTIVE_EPS = 1e-7, 1e-10, 10, 1e-10
KIND = {"qp": 0, "qcqp": 1, "box": 2, "sbox": 3}


def _matvec(M, v):
    """row i: sum_j M[i, j] v[j], j in index order"""
    s = np.zeros(M.shape[0])
    for j in range(M.shape[1]):
        s = s + M[:, j] * v[j]
    return s


def _chol_inverse(A):
    """Left-looking LLT of A (lower triangle read), then the explicit inverse column by column: L y = e_c, L^T x = y."""
    n = A.shape[0]
    L = A.copy()
    for k in range(n):
        s = 0.0
        for j in range(k):
            s = s + L[k, j] * L[k, j]
        xk = np.sqrt(L[k, k] - s)
        t = np.zeros(n - k - 1)
        for j in range(k):
            t = t + L[k + 1:, j] * L[k, j]
        L[k + 1:, k] = (L[k + 1:, k] - t) / xk
        L[k, k] = xk
    inv = np.zeros((n, n))
    for i in range(n):          # every column c at once
        t = np.zeros(n)
        t[i] = 1.0
        for j in range(i):
            t = t - L[i, j] * inv[j, :]
        inv[i, :] = t / L[i, i]
    for i in range(n - 1, -1, -1):
        t = inv[i, :].copy()
        for j in range(i + 1, n):
            t = t - L[j, i] * inv[j, :]
        inv[i, :] = t / L[i, i]
    return inv


def refine(M, dd):
    """Solver::iterative_refinement (Solver.cpp:15-44) handed the rows x m matrix M: the Tikhonov iterate of M x = dd.
    -> (x, steps)"""
    rows, m = M.shape
    Ab = np.zeros(m)
    K = np.zeros((m, m))
    for k in range(rows):
        Ab = Ab + M[k, :] * dd[k]
        K = K + np.outer(M[k, :], M[k, :])
    K[np.arange(m), np.arange(m)] += MU_IR
    Kinv = _chol_inverse(K)
    KinvAb = _matvec(Kinv, Ab)
    xs = np.zeros(m)
    res_pred, not_improved, steps = np.finfo(np.float64).max, 0, 0
    for it in range(IR_MAX):
        steps = it + 1
        xs = MU_IR * _matvec(Kinv, xs) + KinvAb
        d = _matvec(K, xs) - Ab
        ss = 0.0
        for i in range(m):
            ss = ss + d[i] * d[i]
        res = np.sqrt(ss)
        if res_pred - res < IR_EPS:
            not_improved += 1
        else:
            res_pred, not_improved = res, 0
        if res < IR_EPS or not_improved == 2:
            break
    return xs, steps


def effective_bounds(lo, hi, v):
    """csrc/sbox_bounds.h -> (lo', hi', keep_lo, keep_hi)"""
    lo2, hi2 = lo.copy(), hi.copy()
    pos, neg, zero = v > 0, v < 0, v == 0
    hi2[pos] = np.minimum(hi[pos], 0.0)
    lo2[pos] = np.minimum(lo[pos], hi2[pos])
    lo2[neg] = np.maximum(lo[neg], 0.0)
    hi2[neg] = np.maximum(hi[neg], lo2[neg])
    lo2[zero] = 0.0
    hi2[zero] = 0.0
    return lo2, hi2, lo2 == lo, hi2 == hi


def derivative(kind, P, q, ex, x, epsilon, mode, g=None, tangents=None):
    """mode "bwd": g (n) -> dict(grad_P, grad_q[, g0, g1], steps);  mode "jvp": tangents = (dP, dq[, da, db]), None = zero ->
    dict(dx, steps, A, s, place: the system A w = s that was refined and how dx is read off a solution w).  ex: the kind's
    extras as 1-d arrays.  Also returned: "active", the sets the systems were built on."""
    n = q.shape[0]
    nc = n // 2
    jvp = mode == "jvp"
    if jvp:
        tangents = tuple(tangents) + (None,) * (4 - len(tangents))
        dP = np.zeros((n, n)) if tangents[0] is None else tangents[0]
        dq = np.zeros(n) if tangents[1] is None else tangents[1]
        t = -(_matvec(dP, x) + dq)                       # grad_q = -dl, grad_P = -dl x^T, read the other way round
    Px = _matvec(P, x)
    out = {}
    if kind == "qp":
        gam = -(Px + q)
        gam[x > epsilon] = 0.0
        act = gam < -ACTIVE_EPS
        perm = np.concatenate([np.flatnonzero(act), np.flatnonzero(~act)])
        na = int(act.sum())
        A = np.zeros((n, n))                             # A = [[diag(l_A), 0],[0, P_II]]
        for r in range(n):
            for c in range(n):
                A[r, c] = (x[perm[r]] if r == c else 0.0) if (r < na or c < na) else P[perm[r], perm[c]]
        if not jvp:
            dd = np.where(np.arange(n) < na, 0.0, g[perm])
            b, steps = refine(A.T.copy(), dd)
            dl = np.zeros(n)
            dl[perm] = np.where(np.arange(n) < na, 0.0, b)
        else:
            s = np.where(np.arange(n) < na, 0.0, t[perm])
            w, steps = refine(A, s)

            def place(w):
                dx = np.zeros(n)
                dx[perm] = np.where(np.arange(n) < na, 0.0, w)
                return dx
            dx = place(w)
            out.update(A=A, s=s, place=place)
        out["active"] = act
    elif kind == "qcqp":
        l_n, mu = ex[0], ex[1]
        plq = Px + q
        r = l_n * mu
        xa, xb = x[0::2], x[1::2]
        nrm2 = xa * xa + xb * xb
        slack = r + -np.sqrt(nrm2)
        gam = np.zeros(nc)
        for c in range(nc):
            if not (slack[c] > epsilon or r[c] < epsilon):
                ca, cb = 2 * xa[c], 2 * xb[c]
                G = ca * ca + cb * cb
                rhs = ca * plq[2 * c] + cb * plq[2 * c + 1]
                L = np.sqrt(G)
                gam[c] = -((rhs / L) / L)
        S = -(r * r) + nrm2
        act = (S > -ACTIVE_EPS) & (r > ACTIVE_EPS)
        perm = np.flatnonzero(act)
        na = len(perm)
        m = n + na
        A = np.zeros((m, m))       # [[diag(S_act), (diag(gamma) C^T)_act],[C_act, P + blkdiag(2 gamma I2)]]
        for k, c in enumerate(perm):
            A[k, k] = S[c]
            for i in (2 * c, 2 * c + 1):
                A[k, na + i] = gam[c] * (2 * x[i])
                A[na + i, k] = 2 * x[i]
        for i in range(n):
            for j in range(n):
                A[na + i, na + j] = (2 * gam[i // 2] if i == j else 0.0) + P[i, j]
        e1 = 2 * gam * l_n * l_n * mu
        e2 = 2 * gam * l_n * mu * mu
        if not jvp:
            b, steps = refine(A.T.copy(), np.concatenate([np.zeros(na), g]))
            dg = np.zeros(nc)
            dg[perm] = b[:na]
            dl = b[na:]
            out.update(g0=e2 * dg, g1=e1 * dg, gamma=gam, dgamma=dg)
        else:
            da = np.zeros(nc) if tangents[2] is None else tangents[2]
            db = np.zeros(nc) if tangents[3] is None else tangents[3]
            sm = e2 * da + e1 * db
            s = np.concatenate([sm[perm], t])
            w, steps = refine(A, s)
            dx = w[na:]
            out.update(A=A, s=s, place=lambda w: w[na:])
        out["active"] = act
    else:
        lo, hi = ex[0], ex[1]
        keep_lo = keep_hi = np.ones(n, dtype=bool)
        if kind == "sbox":
            lo, hi, keep_lo, keep_hi = effective_bounds(lo, hi, ex[2])
        aL = ~(x - lo > epsilon)
        aU = ~(x - hi < -epsilon)
        nnl = []
        for i in range(n):
            if aL[i]:
                nnl.append(i)
            if aU[i]:
                nnl.append(n + i)
        nn = len(nnl)

        def id2(idx, i):
            return (-1.0 if idx == i else 0.0) if idx < n else (1.0 if idx - n == i else 0.0)

        gam = np.zeros(2 * n)
        steps_dual = 1
        if nn > 0:
            Id2 = np.array([[id2(nnl[p], i) for p in range(nn)] for i in range(n)])
            rhs = np.zeros(n)
            for j in range(n):
                rhs = rhs + (-P[:, j]) * x[j]
            gnn, steps_dual = refine(Id2, rhs - q)
            gam[nnl] = gnn
        m = nn + n
        A = np.zeros((m, m))       # [[0, B],[Id2, P]], B.row(j) = gamma_j Id2.col(j)^T
        for p in range(nn):
            for i in range(n):
                A[p, nn + i] = gam[nnl[p]] * id2(nnl[p], i)
                A[nn + i, p] = id2(nnl[p], i)
        A[nn:, nn:] = P
        if not jvp:
            b, steps = refine(A.T.copy(), np.concatenate([np.zeros(nn), g]))
            dg = np.zeros(2 * n)
            dg[nnl] = b[:nn]
            dl = b[nn:]
            out.update(g0=np.where(keep_lo, -(dg[:n] * gam[:n]), 0.0), g1=np.where(keep_hi, dg[n:] * gam[n:], 0.0), gamma=gam,
                       dgamma=dg)
        else:
            da = np.zeros(n) if tangents[2] is None else np.where(keep_lo, tangents[2], 0.0)
            db = np.zeros(n) if tangents[3] is None else np.where(keep_hi, tangents[3], 0.0)
            sm = np.concatenate([-(da * gam[:n]), db * gam[n:]])
            s = np.concatenate([sm[nnl], t])
            w, steps = refine(A, s)
            dx = w[nn:]
            out.update(A=A, s=s, place=lambda w: w[nn:])
        steps = (steps_dual, steps)
        out["active"] = np.concatenate([aL, aU])
    out["steps"] = steps
    if jvp:
        out["dx"] = dx
    else:
        out["grad_q"] = -dl
        out["grad_P"] = -np.outer(dl, x)
    return out


def flat(d, kind):
    """make_problem-style dict of (B, ., 1) arrays -> (P (B,n,n), q (B,n), extras as (B,.) arrays)"""
    names = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}[kind]
    B = d["q"].shape[0]
    return np.asarray(d["P"]), np.asarray(d["q"]).reshape(B, -1), tuple(np.asarray(d[k]).reshape(B, -1) for k in names)


def jvp_batch(kind, P, q, ex, x, tangents, epsilon=1e-10):
    """tangents: (dP (B,n,n), dq (B,n)[, da, db]) or None entries -> (dx (B,n), steps)"""
    B = q.shape[0]
    outs = [derivative(kind, P[b], q[b], tuple(e[b] for e in ex), x[b], epsilon, "jvp",
                       tangents=tuple(None if t is None else t[b] for t in tangents)) for b in range(B)]
    return np.stack([o["dx"] for o in outs]), np.array([o["steps"] for o in outs], dtype=np.int32)


def random_tangents(kind, B, n, seed, diag=False):
    """Seeded N(0,1) tangents of every differentiable input; dP full and NOT symmetric (diag: a diagonal dP, full form)."""
    rng = np.random.default_rng(seed)
    dP = rng.standard_normal((B, n, n))
    if diag:
        dP = dP * np.eye(n)
    t = [dP, rng.standard_normal((B, n))]
    if kind != "qp":
        ne = n // 2 if kind == "qcqp" else n
        t += [rng.standard_normal((B, ne)), rng.standard_normal((B, ne))]
    return tuple(t)
