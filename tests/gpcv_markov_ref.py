"""Restatement, by plain loops, of the O(N) GPCV step for the Markov variational family (csrc/gpcv_markov.hip),
shared by tests/test_gpcv_markov_host.py and tests/test_gpu_gpcv_markov.py.  Not a test module.

    prior   f - mu Brownian motion from an N(0, j) level: K_M = v min(x, x') + j 1 1', q_0 = v x_0 + j, q_i = v (x_i - x_{i-1})
    family  q = N(m, P^-1), P = Lp Lp', Lp lower bidiagonal: diagonal e^rho_i, entry (i+1, i) gamma_i e^rho_i
    F = w_ell ell - w_kl KL and its closed-form gradients

numpy.  ``step(..., dtype=np.float64)`` is the reference; ``dtype=np.float32`` is the evaluation the kernel makes: inputs and
outputs rounded to fp32, the quadrature in fp32, the recurrences and sums in fp64.  ``broken`` switches on ONE deliberate
mistake (the negative controls): "e" -- e_i without its (1 + gamma)^2 factor; "q0" -- q_0 without j; "adjoint" -- the adjoint
recurrence run backward."""
import math

import numpy as np

LOG_SQRT_2PI = 0.91893853320467274
SCALARS = ("ell", "kl", "quad", "logdet_k", "logdet_s", "trace", "dFdv", "F")
GRADS = ("grad_m", "grad_mu", "grad_rho", "grad_gamma")


def gauss_hermite(n=75):
    """hermgauss nodes, and weights / sqrt(pi) (what the step takes)."""
    x, w = np.polynomial.hermite.hermgauss(n)
    return x, w / math.sqrt(math.pi)


def increments(x, v, j, broken=None):
    n = len(x)
    delta, q = np.empty(n), np.empty(n)
    for i in range(n):
        delta[i] = x[0] if i == 0 else x[i] - x[i - 1]
        q[i] = v * delta[i]
    if broken != "q0":
        q[0] += j
    return delta, q


def variances(rho, gam):
    """s = diag P^-1, backward."""
    n = len(rho)
    s = np.empty(n)
    s[n - 1] = math.exp(-2.0 * rho[n - 1])
    for i in range(n - 2, -1, -1):
        s[i] = math.exp(-2.0 * rho[i]) + gam[i] ** 2 * s[i + 1]
    return s


def rows(m, s, y, ghx, ghw, abc, min_var, min_scale, dt):
    """Per point: E log p, dE/dm, dE/dvar (0 where the variance is floored), and the "cv" parameter sums [3,K] -- the node
    formulas of gh_ell_kernel / gh_cv_ell_kernel, vectorised over points and nodes, in ``dt``."""
    f = lambda a: np.asarray(a, dtype=dt)
    m, y, ghx, ghw, var = f(m), f(y), f(ghx), f(ghw), f(s)
    floored = var < dt(min_var)
    var = np.where(floored, dt(min_var), var)
    sd2 = np.sqrt(dt(2) * var)
    F = m[:, None] + sd2[:, None] * ghx[None, :]                                   # [N,Q]
    ms = dt(min_scale)
    gabc = None
    if abc is None:
        ef = np.exp(F)
        live = ef > ms
        sc = np.where(live, ef, ms)
        r = y[:, None] / sc
        logp = dt(-0.5) * r * r - np.where(live, F, np.log(ms)) - dt(LOG_SQRT_2PI)
        g = np.where(live, r * r - dt(1), dt(0)) * ghw[None, :]
    else:
        a, b, c = (f(t)[None, None, :] for t in abc)
        u = b * F[:, :, None] + c                                                  # [N,Q,K]
        t = np.exp(-np.abs(u))
        sp = np.maximum(u, dt(0)) + np.log1p(t)
        sg = np.where(u >= 0, dt(1) / (dt(1) + t), t / (dt(1) + t))
        sw = (a * sp).sum(-1)
        live = sw > ms
        sc = np.where(live, sw, ms)
        r = y[:, None] / sc
        logp = dt(-0.5) * r * r - np.log(sc) - dt(LOG_SQRT_2PI)
        wg = np.where(live, ghw[None, :] * (r * r - dt(1)) / sc, dt(0))            # w_q g_s
        asg = a * sg
        g = wg * (asg * b).sum(-1)
        gabc = np.stack([(wg[:, :, None] * sp).astype(np.float64).sum((0, 1)),
                         (wg[:, :, None] * asg * F[:, :, None]).astype(np.float64).sum((0, 1)),
                         (wg[:, :, None] * asg).astype(np.float64).sum((0, 1))])
    e = (ghw[None, :] * logp).sum(-1)
    gm = g.sum(-1)
    gv = np.where(floored, dt(0), (g * ghx[None, :]).sum(-1) / sd2)
    return e.astype(np.float64), gm.astype(np.float64), gv.astype(np.float64), gabc


def step(x, v, j, mu, m, rho, gam, y, ghx, ghw, w_ell, w_kl, abc=None, min_var=1e-6, min_scale=1e-3, dtype=np.float64,
         broken=None):
    """One series.  x, m, rho, gam, y [N] (gam[N-1] is not read), mu a number or [N]; abc None or (a, b, c) each [K].
    Returns a dict: the SCALARS, "s" [N], the GRADS [N] (grad_gamma[N-1] = 0) and "grad_abc" [3,K] = dF/d(a,b,c)."""
    if dtype == np.float32:                                                        # the inputs as the kernel reads them
        r32 = lambda a: np.asarray(np.asarray(a, dtype=np.float32), dtype=np.float64)
        x, m, rho, gam, y, mu = r32(x), r32(m), r32(rho), r32(gam), r32(y), r32(mu)
        v, j, w_ell, w_kl = float(np.float32(v)), float(np.float32(j)), float(np.float32(w_ell)), float(np.float32(w_kl))
        d = r32(np.float32(m) - np.float32(mu)) * np.ones(len(m))                  # resid = m - mu is formed in fp32
    else:
        x, m, rho, gam, y = (np.asarray(a, dtype=np.float64) for a in (x, m, rho, gam, y))
        d = m - np.asarray(mu, dtype=np.float64) * np.ones(len(m))
    n = len(m)
    delta, q = increments(x, v, j, broken)
    s = variances(rho, gam)
    a2 = np.array([math.exp(-2.0 * r) for r in rho])
    e, dd = np.empty(n), np.empty(n)
    for i in range(n):
        if i == 0:
            e[i], dd[i] = s[0], d[0]
        else:
            fac = 1.0 if broken == "e" else (1.0 + gam[i - 1]) ** 2
            e[i], dd[i] = a2[i - 1] + fac * s[i], d[i] - d[i - 1]
    trace = quad = logdet_k = srho = dv = 0.0
    for i in range(n):
        trace += e[i] / q[i]
        quad += dd[i] ** 2 / q[i]
        logdet_k += np.log(q[i])
        srho += rho[i]
        dv += delta[i] * (1.0 / q[i] - (e[i] + dd[i] ** 2) / q[i] ** 2)
    logdet_s = -2.0 * srho
    ev, gm, gv, gabc = rows(m, s, y, ghx, ghw, abc, min_var, min_scale, dtype)
    ell = float(ev.sum())
    kl = 0.5 * (trace + quad - n + logdet_k - logdet_s)
    # the adjoint of s
    h = np.empty(n)
    for i in range(n):
        h[i] = w_ell * gv[i] - w_kl * (1.0 if i == 0 else (1.0 + gam[i - 1]) ** 2) / (2.0 * q[i])
    sh = np.empty(n)
    if broken == "adjoint":
        sh[n - 1] = h[n - 1]
        for i in range(n - 2, -1, -1):
            sh[i] = h[i] + gam[i] ** 2 * sh[i + 1]
    else:
        sh[0] = h[0]
        for i in range(1, n):
            sh[i] = h[i] + gam[i - 1] ** 2 * sh[i - 1]
    g_m, g_mu, g_rho, g_gam = np.empty(n), np.empty(n), np.empty(n), np.zeros(n)
    for i in range(n):
        kd = dd[i] / q[i]
        t = sh[i]
        if i < n - 1:
            kd -= dd[i + 1] / q[i + 1]
            t -= w_kl / (2.0 * q[i + 1])
            g_gam[i] = 2.0 * gam[i] * s[i + 1] * sh[i] - w_kl * (1.0 + gam[i]) * s[i + 1] / q[i + 1]
        g_rho[i] = -2.0 * a2[i] * t - w_kl
        g_m[i] = w_ell * gm[i] - w_kl * kd
        g_mu[i] = w_kl * kd
    out = dict(ell=ell, kl=kl, quad=quad, logdet_k=logdet_k, logdet_s=logdet_s, trace=trace, dFdv=-0.5 * w_kl * dv,
               F=w_ell * ell - w_kl * kl, s=s, grad_m=g_m, grad_mu=g_mu, grad_rho=g_rho, grad_gamma=g_gam,
               grad_abc=None if gabc is None else w_ell * gabc)
    if dtype == np.float32:                                                        # the outputs as the kernel writes them
        out = {k: (None if a is None else np.asarray(np.asarray(a, dtype=np.float32), dtype=np.float64)) if k != "s" else a
               for k, a in out.items()}
    return out


def draw(m, rho, gam, eps):
    """m + Lp^-T eps by the backward recurrence; eps [..., N]."""
    n = len(m)
    eps = np.asarray(eps, dtype=np.float64)
    u = np.empty_like(eps)
    u[..., n - 1] = eps[..., n - 1] * math.exp(-rho[n - 1])
    for i in range(n - 2, -1, -1):
        u[..., i] = eps[..., i] * math.exp(-rho[i]) - gam[i] * u[..., i + 1]
    return np.asarray(m, dtype=np.float64) + u


def dense_root(rho, gam):
    """Lp [N,N]."""
    n = len(rho)
    Lp = np.zeros((n, n))
    for i in range(n):
        Lp[i, i] = math.exp(rho[i])
        if i + 1 < n:
            Lp[i + 1, i] = gam[i] * Lp[i, i]
    return Lp


def prior_cov(x, v, j):
    x = np.asarray(x, dtype=np.float64)
    return v * np.minimum(x[:, None], x[None, :]) + j


def tridiag_root(diag, off):
    """(rho, gamma) of the bidiagonal Cholesky factor of the tridiagonal matrix (diag [N], off[i] = entry (i+1, i))."""
    n = len(diag)
    rho, gam = np.zeros(n), np.zeros(n)
    l2 = diag[0]
    for i in range(n):
        rho[i] = 0.5 * math.log(l2)
        if i + 1 < n:
            gam[i] = off[i] / l2
            l2 = diag[i + 1] - gam[i] ** 2 * l2
    return rho, gam


def prior_precision(x, v, j):
    """K_M^-1 as (diag [N], off [N-1])."""
    _, q = increments(x, v, j)
    diag = 1.0 / q
    diag[:-1] += 1.0 / q[1:]
    return diag, -1.0 / q[1:]


def make_inputs(n, seed, x0_zero=False, v=0.2, j=1e-3, dt=1.0 / 252, spread=0.1, lam=(0.5, 4.0)):
    """A test problem: the grid, data, and a root perturbed by ``spread`` around chol(K_M^-1 + diag(lambda)) -- the optimum's
    structure.  Everything fp64 but already exactly representable in fp32 (so that both sides read the same numbers)."""
    g = np.random.default_rng(seed)
    r32 = lambda a: np.asarray(np.asarray(a, dtype=np.float32), dtype=np.float64)
    x = r32((np.arange(n) + (0 if x0_zero else 1)) * dt)
    v = float(np.float32(v))
    diag, off = prior_precision(x, v, float(np.float32(j)))
    rho, gam = tridiag_root(diag + g.uniform(*lam, n), off)
    rho = r32(rho + spread * g.standard_normal(n))
    gam = r32(gam * (1.0 + spread * g.standard_normal(n)))
    m = r32(-1.0 + 0.3 * g.standard_normal(n))
    y = r32(np.exp(m) * g.standard_normal(n))
    mu = float(np.float32(-0.9))
    return dict(x=x, v=v, mu=mu, m=m, rho=rho, gam=gam, y=y)


def make_abc(K, seed):
    """(a, b, c) [K] as the constraints map VolatilityGaussianLikelihood's start-up draws, rounded to fp32."""
    g = np.random.default_rng(1000 + seed)
    ra, rb, rc = g.uniform(0, 1, K), 0.1 * g.uniform(0, 1, K), g.uniform(0, 1, K)
    sig = lambda t: 1.0 / (1.0 + np.exp(-t))
    r32 = lambda a: np.asarray(np.asarray(a, dtype=np.float32), dtype=np.float64)
    return r32(np.log1p(np.exp(ra))), r32(3.0 * sig(rb)), r32(6.0 * sig(rc) - 3.0)


def learn(x, yy, start, iters, j=1e-3, lr=0.01, vol0=0.2, num_gh=75):
    """fp64 Adam (torch.optim.Adam's update) on -F of the "exp" step with the closed-form gradients, from ``start`` =
    (m, rho, gamma, mean constant); raw_vol starts at logit(vol0); w_ell = w_kl = 1/N as VariationalELBO sets them.
    Returns (losses, [m, rho, gamma, const, raw_vol])."""
    ghx, ghw = gauss_hermite(num_gh)
    n = len(yy)
    ps = [np.array(t, dtype=np.float64).reshape(-1) for t in start] + [np.array([math.log(vol0 / (1 - vol0))])]
    mom = [(np.zeros_like(p), np.zeros_like(p)) for p in ps]
    b1, b2, eps = 0.9, 0.999, 1e-8
    losses = []
    for it in range(1, iters + 1):
        m, rho, gam, const, raw_vol = ps
        v = 1.0 / (1.0 + math.exp(-raw_vol[0]))
        o = step(x, v, j, const[0], m, rho, gam, yy, ghx, ghw, 1.0 / n, 1.0 / n)
        losses.append(-o["F"])
        grads = [-o["grad_m"], -o["grad_rho"], -o["grad_gamma"], np.array([-o["grad_mu"].sum()]),
                 np.array([-o["dFdv"] * v * (1 - v)])]
        for p, g, (m1, m2) in zip(ps, grads, mom):
            m1 *= b1
            m1 += (1 - b1) * g
            m2 *= b2
            m2 += (1 - b2) * g * g
            p -= lr / (1 - b1 ** it) * m1 / (np.sqrt(m2) / math.sqrt(1 - b2 ** it) + eps)
    return losses, ps


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
# tests/test_gpu_gpcv_markov.py runs the kernel at exactly these; tests/test_gpcv_markov_host.py evaluates the fp32 restatement
# and the negative controls at exactly these.
J = 1e-3
VOLS = (0.2, 0.05, 0.9)
SHAPES = [(n, B) for n in (1, 2, 3, 63, 64, 65, 129, 399) for B in (1, 3, 65)]
# both sides of the scan's boundaries: a thread's run is 4 points, a wave's 256, the step's workgroup chunk 2048
BOUNDARIES = [(4, 2), (5, 2), (255, 2), (256, 1), (257, 2), (2047, 1), (2048, 2), (2049, 1), (4097, 2)]
EXP_CASES = [(n, B, 0, "plain") for n, B in SHAPES + BOUNDARIES]
CV_CASES = [(n, B, Kc, "plain") for Kc in (1, 5, 8) for n, B in SHAPES + [(257, 2), (2049, 1)]]
KIND_CASES = [(130, 3, Kc, kind) for kind in ("floored", "clamped") for Kc in (0, 5)]
ALL_CASES = EXP_CASES + CV_CASES + KIND_CASES
_CASES = {}


def case_inputs(n, B, Kc=0, kind="plain"):
    """The B series of a GPU case over one grid (x_0 = 0 when n + B is odd) and the weights (w_ell, w_kl != 1/N).  kind
    "floored": rho so large, and every second coupling so small, that every second variance is under min_var; "clamped": means
    so low that nodes fall under min_scale."""
    x0_zero = (n + B) % 2 == 1
    ps = []
    for b in range(B):
        p = make_inputs(n, 100 * n + b, x0_zero=x0_zero, v=VOLS[b % 3])
        p["mu"] = float(np.float32(-0.9 + 0.05 * b))
        if kind == "floored":
            p["rho"][::2] = 8.0                                         # e^-16 = 1.1e-7, and next to nothing from the neighbour
            p["gam"][::2] = np.float32(1e-4) * np.sign(p["gam"][::2])
        if kind == "clamped":
            p["m"][::3] = np.float32(-7.5)
        p["abc"] = make_abc(Kc, 10 * n + b) if Kc else None
        ps.append(p)
    return ps, 1.0 / n, 0.7 / (n + 3)


def step_of(p, we, wk, **kw):
    ghx, ghw = gauss_hermite(75)
    return step(p["x"], p["v"], J, p["mu"], p["m"], p["rho"], p["gam"], p["y"], ghx, ghw, we, wk, abc=p["abc"], **kw)


def case(n, B, Kc=0, kind="plain"):
    """(inputs, their fp64 references, w_ell, w_kl) of a GPU case; computed once."""
    key = (n, B, Kc, kind)
    if key not in _CASES:
        ps, we, wk = case_inputs(n, B, Kc, kind)
        _CASES[key] = (ps, [step_of(p, we, wk) for p in ps], we, wk)
    return _CASES[key]
