"""Restatement, by plain loops, of the multi-task GPCV step for the Markov variational family under the Kronecker prior
(csrc/gpcv_mt_markov.hip), shared by tests/test_mt_gpcv_markov_host.py and tests/test_gpu_mt_gpcv_markov.py.
Not a test module.

    prior   p(F) = N(1 c', K_M (x) K_t),  K_M = v min(x, x') + j 1 1' (q_0 = v x_0 + j, q_i = v (x_i - x_{i-1})),
            K_t = f f' + diag softplus(raw_var)
    family  q(F) = N(M, P^-1 (x) S_t),  P = Lp Lp' (Lp lower bidiagonal: diagonal e^rho_i, entry (i+1, i) gamma_i e^rho_i),
            S_t = Lt Lt',  Lt = tril(its argument)
    F = w_ell ell - w_kl KL and its closed-form gradients

numpy.  ``step(..., dtype=np.float64)`` is the reference; ``dtype=np.float32`` is the evaluation the kernels make: inputs and
outputs rounded to fp32, the quadrature nodes in fp32, every recurrence and sum in fp64.  ``broken`` switches on ONE
deliberate mistake that only this step can make (the negative controls): "tau_t" -- tau_t dropped from h_i and from dF/dgamma;
"rho_T" -- the -w_kl T of dF/drho written as -w_kl; "g2" -- tr(K_t^-1 G2) dropped from dF/dv; "st_next" -- the st of task
t + 1 used for task t wherever the likelihood side reads it (the variance and the row sums a_n)."""
import math

import numpy as np

import gpcv_markov_ref as MR

J = 1e-3
SCALARS = ("ell", "kl", "quad", "logdet_km", "logdet_kt", "logdet_sx", "logdet_st", "tau_x", "tau_t", "dFdv", "F")   # out[0..10]
GRADS = ("grad_M", "grad_c", "grad_rho", "grad_gamma", "grad_Lt", "grad_f", "grad_raw_var")
# the tiles of csrc/gpcv_mt_markov.hip: a thread's run of the scans is 4 points, a wave's 256, a chunk 2048; the quadrature
# pass takes 16 rows a workgroup, the partial sums of G / G2 128 rows a workgroup staged 32 at a time, grad_M 32 rows a
# workgroup; the "cv" parameter partials are added by 256 threads (257 workgroups from N = 4097 on)
ROWS_TILE, GRAM_TILE, GRAM_STAGE, GRADM_TILE = 16, 128, 32, 32
RHO_SHIFT, RAW_VAR_SHIFT = 0.75, 1.5


def _softplus(v):
    return np.where(v > 20.0, v, np.log1p(np.exp(np.minimum(v, 20.0))))


def step(x, v, j, c, M, rho, gam, Lt, f, raw_var, y, ghx, ghw, w_ell, w_kl, abc=None, min_var=1e-6, min_scale=1e-3,
         dtype=np.float64, broken=None):
    """x, rho, gam [N] (gam[N-1] is not read), M, y [N,T], c, f, raw_var [T], Lt [T,T]; abc None or (a, b, c) each [T,K].
    Returns a dict: the SCALARS, "s" [N], the GRADS and "grad_abc" [T,3,K] = dF/d(a,b,c)."""
    r32 = lambda a: np.asarray(np.asarray(a, dtype=np.float32), dtype=np.float64)
    if dtype == np.float32:                                                        # the inputs as the kernels read them
        x, c, M, rho, gam, Lt, f, raw_var, y = (r32(a) for a in (x, c, M, rho, gam, Lt, f, raw_var, y))
        v, j, w_ell, w_kl = (float(np.float32(a)) for a in (v, j, w_ell, w_kl))
    else:
        x, c, M, rho, gam, Lt, f, raw_var, y = (np.asarray(a, dtype=np.float64) for a in (x, c, M, rho, gam, Lt, f, raw_var, y))
    n, T = M.shape
    f = f.reshape(T)
    Lt = np.tril(Lt)
    delta, q = MR.increments(x, v, j)
    s = MR.variances(rho, gam)
    a2 = np.array([math.exp(-2.0 * r) for r in rho])
    e = np.empty(n)
    for i in range(n):
        e[i] = s[0] if i == 0 else a2[i - 1] + (1.0 + gam[i - 1]) ** 2 * s[i]
    st = np.array([sum(Lt[t, k] ** 2 for k in range(t + 1)) for t in range(T)])
    st_l = np.roll(st, -1) if broken == "st_next" else st                           # the st the likelihood side reads
    # ---- the likelihood: one column of points per task
    ell = 0.0
    gm, gv = np.empty((n, T)), np.empty((n, T))
    gabc = None if abc is None else np.empty((T, 3, np.shape(abc[0])[1]))
    for t in range(T):
        st_t = st_l[t]
        ev, gm[:, t], gv[:, t], ga = MR.rows(M[:, t], s * st_t, y[:, t], ghx, ghw, None if abc is None else [a[t] for a in abc],
                                             min_var, min_scale, dtype)
        ell += float(ev.sum())
        if abc is not None:
            gabc[t] = ga
    a_n = gv @ st_l                                                                # sum_t gv_nt st_t
    b_t = s @ gv                                                                   # sum_n gv_nt s_n
    # ---- the task side
    Kt = np.outer(f, f) + np.diag(_softplus(raw_var))
    Ki = np.linalg.inv(Kt)
    Ki = 0.5 * (Ki + Ki.T)
    St = Lt @ Lt.T
    tau_t = float(np.trace(Ki @ St))
    logdet_kt = float(np.linalg.slogdet(Kt)[1])
    logdet_st = float(sum(math.log(Lt[t, t] ** 2) for t in range(T)))
    # ---- the x side
    R = M - c[None, :]
    D = np.empty((n, T))
    G, G2 = np.zeros((T, T)), np.zeros((T, T))
    tau_x = ldq = srho = x1 = x2 = 0.0
    for i in range(n):
        D[i] = R[0] if i == 0 else M[i] - M[i - 1]
        G += np.outer(D[i], D[i]) / q[i]
        G2 += delta[i] * np.outer(D[i], D[i]) / q[i] ** 2
        tau_x += e[i] / q[i]
        ldq += math.log(q[i])
        srho += rho[i]
        x1 += delta[i] / q[i]
        x2 += delta[i] * e[i] / q[i] ** 2
    quad = float(np.trace(Ki @ G))
    kl = 0.5 * (tau_x * tau_t + quad - n * T + T * ldq + n * logdet_kt + 2.0 * T * srho - n * logdet_st)
    F = w_ell * ell - w_kl * kl
    tr_g2 = 0.0 if broken == "g2" else float(np.trace(Ki @ G2))
    dFdv = -0.5 * w_kl * (T * x1 - tau_t * x2 - tr_g2)
    # ---- the adjoint of s, forward
    tt = 1.0 if broken == "tau_t" else tau_t
    sh = np.empty(n)
    for i in range(n):
        h = w_ell * a_n[i] - w_kl * tt * (1.0 if i == 0 else (1.0 + gam[i - 1]) ** 2) / (2.0 * q[i])
        sh[i] = h if i == 0 else h + gam[i - 1] ** 2 * sh[i - 1]
    g_rho, g_gam, A = np.empty(n), np.zeros(n), np.empty((n, T))
    for i in range(n):
        t_ = sh[i]
        A[i] = D[i] / q[i]
        if i < n - 1:
            A[i] = A[i] - (M[i + 1] - M[i]) / q[i + 1]
            t_ -= w_kl * tau_t / (2.0 * q[i + 1])
            g_gam[i] = 2.0 * gam[i] * s[i + 1] * sh[i] - w_kl * tt * (1.0 + gam[i]) * s[i + 1] / q[i + 1]
        g_rho[i] = -2.0 * a2[i] * t_ - w_kl * (1.0 if broken == "rho_T" else T)
    g_M = w_ell * gm - w_kl * A @ Ki
    g_c = w_kl * Ki @ R[0] / q[0]
    LtiT = np.linalg.inv(Lt).T
    g_Lt = np.tril(2.0 * w_ell * b_t[:, None] * Lt - w_kl * (tau_x * Ki @ Lt - n * LtiT))
    H = 0.5 * (n * Ki - tau_x * Ki @ St @ Ki - Ki @ G @ Ki)
    g_f = -2.0 * w_kl * H @ f
    g_rv = -w_kl * np.diag(H) / (1.0 + np.exp(-raw_var))
    out = dict(ell=ell, kl=kl, quad=quad, logdet_km=ldq, logdet_kt=logdet_kt, logdet_sx=-2.0 * srho, logdet_st=logdet_st,
               tau_x=tau_x, tau_t=tau_t, dFdv=dFdv, F=F, s=s, grad_M=g_M, grad_c=g_c, grad_rho=g_rho, grad_gamma=g_gam,
               grad_Lt=g_Lt, grad_f=g_f, grad_raw_var=g_rv, grad_abc=None if gabc is None else w_ell * gabc)
    if dtype == np.float32:                                                        # the outputs as the kernels write them
        out = {k: (None if a is None else r32(a)) if k != "s" else a for k, a in out.items()}
    return out


def make_abc(T, K, seed):
    """(a, b, c) [T,K] from spread per-task raws (mt_gpcv_cv_ref.draw_raws(spread=True)) through the constraints, fp32 values."""
    import gpcv_cv_ref as CV
    import mt_gpcv_cv_ref as MC
    raws = MC.draw_raws(T, K, seed, spread=True)
    r32 = lambda a: np.asarray(np.asarray(a, dtype=np.float32), dtype=np.float64)
    return tuple(r32(t.numpy()) for t in CV.constrain(raws["raw_a"], raws["raw_b"], raws["raw_c"]))


def make_inputs(n, T, seed, x0_zero=False, v=0.2, Kc=0, kind="plain"):
    """A test problem: gpcv_markov_ref.make_inputs' grid and root (perturbed around the optimum's structure), T columns of
    means and data of different scales, a task root with junk above its diagonal, covar_factor of both signs.  Everything
    fp64 but exactly representable in fp32.  kind "floored": rho[::2] = 8 and every second coupling 1e-4 (every second
    variance under min_var); "clamped": M[::3] = -7.5 ("cv": 1.25 under each task's threshold): nodes under min_scale."""
    g = np.random.default_rng(7000 + seed)
    r32 = lambda a: np.asarray(np.asarray(a, dtype=np.float32), dtype=np.float64)
    p = MR.make_inputs(n, seed, x0_zero=x0_zero, v=v)
    t = np.arange(T)
    M = r32(-1.0 + 0.5 * (t % 3 - 1)[None, :] + 0.3 * g.standard_normal((n, T)))
    y = r32(np.exp(M) * g.standard_normal((n, T)) * (0.5 * (1 + t % 4))[None, :])
    c = r32(-0.9 + 0.1 * g.standard_normal(T))
    # (rows of the task root of visibly different size, so that a task evaluated with its neighbour's st shows)
    Lt = r32(np.tril(np.eye(T) * 0.7 + 0.2 * g.standard_normal((T, T)) / math.sqrt(T)) * (1.5 + (t % 3))[:, None]
             + np.triu(g.standard_normal((T, T)), 1))
    f = 0.5 * g.standard_normal(T)
    if T > 1:
        f[0], f[1] = abs(f[0]) + 0.1, -abs(f[1]) - 0.1
    # (the root RHO_SHIFT under the optimum's, so that the variances s_n st_t are large enough for the likelihood term to
    # feel them: a mistake in the variance must show in ell, whose bound does not depend on the weights)
    # (not the last point: its pivot, and so its rho, is far smaller already, and it would dominate every gradient)
    rho, gam = p["rho"].copy(), p["gam"].copy()
    rho[:-1] = r32(rho[:-1] - RHO_SHIFT)
    if kind == "floored":
        rho[1:-1:2] -= np.float32(0.5)
        rho[::2] = 8.0                                                  # e^-16 = 1.1e-7, and next to nothing from the neighbour
        gam[::2] = np.float32(1e-4) * np.where(gam[::2] < 0, -1.0, 1.0)
    abc = make_abc(T, Kc, seed + 1) if Kc else None
    if kind == "clamped":
        # "exp": e^-7.5 = 5.5e-4 < min_scale.  "cv": the spread warps of some tasks are still above min_scale at -7.5, so each
        # task's rows go 1.25 below ITS threshold f_t, scale_t(f_t) = min_scale (bisection: scale_t is increasing)
        M[::3] = np.float32(-7.5) if abc is None else r32(_scale_threshold(abc, 1e-3) - 1.25)[None, :]
        y[::3] = r32(1e-3 * g.standard_normal(y[::3].shape))           # (data of the clamped scale's size: y / scale stays O(1))
    return dict(x=p["x"], v=p["v"], c=c, M=M, rho=rho, gam=gam, Lt=Lt, f=r32(f), raw_var=r32(g.standard_normal(T) + RAW_VAR_SHIFT), y=y,
                abc=abc)


def _scale_threshold(abc, target):
    """f_t with sum_k a_tk softplus(b_tk f_t + c_tk) = target, per task."""
    a, b, c = abc
    lo, hi = np.full(a.shape[0], -200.0), np.full(a.shape[0], 20.0)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        up = (a * np.logaddexp(0.0, b * mid[:, None] + c)).sum(-1) < target
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    return 0.5 * (lo + hi)


def step_of(p, we, wk, **kw):
    ghx, ghw = MR.gauss_hermite(75)
    return step(p["x"], p["v"], J, p["c"], p["M"], p["rho"], p["gam"], p["Lt"], p["f"], p["raw_var"], p["y"], ghx, ghw, we, wk,
                abc=p["abc"], **kw)


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
# tests/test_gpu_mt_gpcv_markov.py runs the kernels at exactly these (N, T, Kc, kind); tests/test_mt_gpcv_markov_host.py
# evaluates the fp32 restatement and the negative controls at exactly these.
VOLS = (0.2, 0.05, 0.9)
GENERIC = [(n, T) for n in (1, 2, 3, 63, 64, 65, 129, 399) for T in (1, 2, 15, 16, 17, 63, 64) if n * T <= 3000]
# both sides of the scans' boundaries and of every tile edge of the quadrature, partial-sum and grad_M passes
SCAN_N = (4, 5, 255, 256, 257, 2047, 2048, 2049, 4097)
TILE_N = (15, 16, 17, 31, 32, 33, 127, 128)                              # (129 is among the generic shapes)
BOUNDARIES = [(n, T) for n in SCAN_N + TILE_N for T in (1, 3)]
EXP_CASES = [(n, T, 0, "plain") for n, T in GENERIC + BOUNDARIES]
CV_CASES = ([(n, T, 5, "plain") for n, T in GENERIC if T in (1, 2, 17, 64) or n in (65, 399)]
            + [(n, T, Kc, "plain") for Kc in (1, 8) for n, T in ((3, 2), (65, 17), (129, 16), (399, 2))]
            + [(n, T, Kc, "plain") for Kc in (1, 5, 8) for n, T in ((17, 3), (257, 3), (2049, 1), (4097, 3))])
KIND_CASES = [(130, 3, Kc, kind) for kind in ("floored", "clamped") for Kc in (0, 5)]
ALL_CASES = EXP_CASES + CV_CASES + KIND_CASES
_CASES = {}


def case_inputs(n, T, Kc=0, kind="plain"):
    """The inputs of a GPU case (x_0 = 0 when n + T is odd) and the weights (w_ell, w_kl: not the model's 1/N, 1/(N T); the
    KL's is large enough for a mistake in a KL-only term to show beside the likelihood's gradients)."""
    p = make_inputs(n, T, 100 * n + T, x0_zero=(n + T) % 2 == 1, v=VOLS[(n + T) % 3], Kc=Kc, kind=kind)
    return p, 0.37 / n, 2.5 / (n + 3)


def case(n, T, Kc=0, kind="plain"):
    """(inputs, their fp64 reference, w_ell, w_kl) of a GPU case; computed once."""
    key = (n, T, Kc, kind)
    if key not in _CASES:
        p, we, wk = case_inputs(n, T, Kc, kind)
        _CASES[key] = (p, step_of(p, we, wk), we, wk)
    return _CASES[key]


SCALAR_TOL, GRAD_TOL, DV_TOL, ABC_TOL = 5e-5, 2e-3, 2e-3, 2e-3          # the project's GPCV bounds


def bound_excess(o, ref, n):
    """Each quantity's error as a multiple of the GPU tests' bound for it (<= 1 passes): scalars and F at SCALAR_TOL
    max(1, |ref|); gradients at GRAD_TOL of the gradient's largest reference entry (grad_abc: ABC_TOL); dF/dv at
    DV_TOL |ref|, and exactly 0 where the reference is (N = 1, x_0 = 0: K_M does not depend on v)."""
    ex = {k: abs(float(o[k]) - ref[k]) / (SCALAR_TOL * max(1.0, abs(ref[k]))) for k in SCALARS if k != "dFdv"}
    ex["dFdv"] = abs(float(o["dFdv"]) - ref["dFdv"]) / (DV_TOL * abs(ref["dFdv"])) if ref["dFdv"] != 0 else float(o["dFdv"] != 0)
    for k in GRADS:
        if k == "grad_gamma" and n == 1:
            ex[k] = float(np.abs(o[k]).max())                                       # no coupling: exactly 0
            continue
        ex[k] = float(np.abs(np.asarray(o[k]).reshape(ref[k].shape) - ref[k]).max() / (GRAD_TOL * max(np.abs(ref[k]).max(), 1e-300)))
    if ref.get("grad_abc") is not None:
        ex["grad_abc"] = float(np.abs(np.asarray(o["grad_abc"]) - ref["grad_abc"]).max() / (ABC_TOL * np.abs(ref["grad_abc"]).max()))
    return {k: (e if e == e else float("inf")) for k, e in ex.items()}


def learn(x, yy, start, iters, j=J, lr=0.01, vol0=0.2, num_gh=75):
    """fp64 Adam (torch.optim.Adam's update) on -F of the "exp" step with the closed-form gradients, from ``start`` =
    (M, rho, gamma, Lt, c, f, raw_var); raw_vol starts at logit(vol0); w_ell = 1/N, w_kl = 1/(N T) as VariationalELBO sets
    them for the multi-task model.  Returns (losses, [M, rho, gamma, Lt, c, f, raw_var, raw_vol])."""
    ghx, ghw = MR.gauss_hermite(num_gh)
    n, T = yy.shape
    ps = [np.array(t, dtype=np.float64) for t in start] + [np.array([math.log(vol0 / (1 - vol0))])]
    mom = [(np.zeros_like(p), np.zeros_like(p)) for p in ps]
    b1, b2, eps = 0.9, 0.999, 1e-8
    losses = []
    for it in range(1, iters + 1):
        M, rho, gam, Lt, c, f, rv, raw_vol = ps
        v = 1.0 / (1.0 + math.exp(-raw_vol[0]))
        o = step(x, v, j, c, M, rho, gam, Lt, f, rv, yy, ghx, ghw, 1.0 / n, 1.0 / (n * T))
        losses.append(-o["F"])
        grads = [-o["grad_M"], -o["grad_rho"], -o["grad_gamma"], -o["grad_Lt"], -o["grad_c"], -o["grad_f"].reshape(f.shape),
                 -o["grad_raw_var"], np.array([-o["dFdv"] * v * (1 - v)])]
        for p, g, (m1, m2) in zip(ps, grads, mom):
            m1 *= b1
            m1 += (1 - b1) * g
            m2 *= b2
            m2 += (1 - b2) * g * g
            p -= lr / (1 - b1 ** it) * m1 / (np.sqrt(m2) / math.sqrt(1 - b2 ** it) + eps)
    return losses, ps
