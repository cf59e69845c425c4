"""Restatement, by plain loops, of the natural-gradient update of the Markov variational family (csrc/gpcv_markov_ng.hip;
DESIGN 4.23), shared by tests/test_gpcv_natgrad_host.py and tests/test_gpu_gpcv_natgrad.py.  Not a test module.

    sites     lam1, lam2 [N]:  the optimal q has precision K_M^-1 + diag(lam2) and mean mu + P^-1 lam1
    targets   t2_i = max(-2 r gv_i, 0),  t1_i = r gm_i + t2_i (m_i - mu_i),  r = w_ell / w_kl, gm = dE/dm, gv = dE/ds at q
    update    lam <- (1 - beta) lam + beta t;  (rho, gamma) = tridiag_root(K_M^-1 + diag(lam2));  m = mu + P^-1 lam1

numpy.  ``update(..., dtype=np.float64)`` is the reference; ``dtype=np.float32`` runs the quadrature (``rows``) in fp32 as the
kernel does, everything else in fp64, and rounds nothing on the way out.  ``broken`` switches on ONE deliberate mistake (the
negative controls): "t1" -- t1 without t2 d; "r" -- r = 1; "clamp" -- t2 not clamped at 0."""
import math

import numpy as np

import gpcv_markov_ref as MR
from gpcv_markov_ref import increments, prior_precision, rows, variances  # noqa: F401


def solve_root(rho, gam, rhs):
    """delta with Lp Lp' delta = rhs by the two serial sweeps: t_0 = rhs_0, t_i = rhs_i - gamma_{i-1} t_{i-1};
    delta_{N-1} = t_{N-1} / d_{N-1}, delta_i = t_i / d_i - gamma_i delta_{i+1}, d_i = e^{2 rho_i}."""
    n = len(rho)
    t, delta = np.empty(n), np.empty(n)
    for i in range(n):
        t[i] = rhs[i] - (gam[i - 1] * t[i - 1] if i > 0 else 0.0)
    for i in range(n - 1, -1, -1):
        delta[i] = t[i] * math.exp(-2.0 * rho[i]) - (gam[i] * delta[i + 1] if i + 1 < n else 0.0)
    return delta


def update(x, v, j, mu, m, rho, gam, y, ghx, ghw, w_ell, w_kl, lam1, lam2, beta=1.0, abc=None, min_var=1e-6, min_scale=1e-3,
           dtype=np.float64, broken=None):
    """One update of one series.  x, m, rho, gam, y, lam1, lam2 [N] (gam[N-1] is not read), mu a number or [N].
    Returns a dict: "lam1", "lam2", "m", "rho", "gam" (gam[N-1] = 0), "clamped" (the number of sites with gv > 0),
    "gm", "gv", "s" (of the q that went in) and "change" = max |new - old| of (m, rho, gam[:N-1])."""
    x, m, rho, gam, y, lam1, lam2 = (np.asarray(a, dtype=np.float64) for a in (x, m, rho, gam, y, lam1, lam2))
    n = len(m)
    mu = np.asarray(mu, dtype=np.float64) * np.ones(n)
    r = 1.0 if broken == "r" else w_ell / w_kl
    s = variances(rho, gam)
    _, gm, gv, _ = rows(m, s, y, ghx, ghw, abc, min_var, min_scale, dtype)
    t2 = -2.0 * r * gv
    if broken != "clamp":
        t2 = np.maximum(t2, 0.0)
    t1 = r * gm + (0.0 if broken == "t1" else t2 * (m - mu))
    l2 = (1.0 - beta) * lam2 + beta * t2
    l1 = (1.0 - beta) * lam1 + beta * t1
    diag, off = prior_precision(x, v, j)
    nrho, ngam = MR.tridiag_root(diag + l2, off)
    nm = mu + solve_root(nrho, ngam, l1)
    change = (np.abs(nm - m).max(), np.abs(nrho - rho).max(), np.abs(ngam[:-1] - gam[:-1]).max() if n > 1 else 0.0)
    return dict(lam1=l1, lam2=l2, m=nm, rho=nrho, gam=ngam, clamped=int((gv > 0).sum()), gm=gm, gv=gv, s=s, change=change)


def iterate(p, we, wk, iters, beta=1.0, dtype=np.float64, broken=None, lam=None):
    """``iters`` updates of the case ``p`` (a dict of gpcv_markov_ref.make_inputs / case_inputs) from the sites ``lam``
    (zeros: q = prior).  Returns (the last update's dict, the list of F after each update, the state p')."""
    ghx, ghw = MR.gauss_hermite(75)
    n = len(p["m"])
    l1, l2 = (np.zeros(n), np.zeros(n)) if lam is None else lam
    q = dict(p)
    Fs, u = [], None
    for _ in range(iters):
        u = update(q["x"], q["v"], MR.J, q["mu"], q["m"], q["rho"], q["gam"], q["y"], ghx, ghw, we, wk, l1, l2, beta,
                   abc=q["abc"], dtype=dtype, broken=broken)
        l1, l2 = u["lam1"], u["lam2"]
        q = dict(q, m=u["m"], rho=u["rho"], gam=u["gam"])
        Fs.append(float(MR.step_of(q, we, wk)["F"]))
    return u, Fs, q


def fit(x, yy, start, iters, j=1e-3, lr=0.01, vol0=0.2, num_gh=75, beta=1.0):
    """The "natgrad" trainer in fp64: per iteration ONE update of q (sites from zeros) under the current mean constant and
    vol, then the step at the new q -- its -F is the iteration's loss -- and ``learn()``'s Adam on the constant and raw_vol
    alone.  ``start`` = (m, rho, gamma, mean constant) as gpcv_markov_ref.learn takes it.
    Returns (losses, [m, rho, gamma, const, raw_vol])."""
    ghx, ghw = MR.gauss_hermite(num_gh)
    n = len(yy)
    m, rho, gam = (np.array(t, dtype=np.float64).reshape(-1) for t in start[:3])
    hs = [np.array(start[3], dtype=np.float64).reshape(-1), np.array([math.log(vol0 / (1 - vol0))])]
    mom = [(np.zeros_like(p), np.zeros_like(p)) for p in hs]
    l1, l2 = np.zeros(n), np.zeros(n)
    b1, b2, eps = 0.9, 0.999, 1e-8
    losses = []
    for it in range(1, iters + 1):
        const, raw_vol = hs
        v = 1.0 / (1.0 + math.exp(-raw_vol[0]))
        u = update(x, v, j, const[0], m, rho, gam, yy, ghx, ghw, 1.0 / n, 1.0 / n, l1, l2, beta)
        l1, l2, m, rho, gam = u["lam1"], u["lam2"], u["m"], u["rho"], u["gam"]
        o = MR.step(x, v, j, const[0], m, rho, gam, yy, ghx, ghw, 1.0 / n, 1.0 / n)
        losses.append(-o["F"])
        grads = [np.array([-o["grad_mu"].sum()]), np.array([-o["dFdv"] * v * (1 - v)])]
        for p, g, (m1, m2) in zip(hs, grads, mom):
            m1 *= b1
            m1 += (1 - b1) * g
            m2 *= b2
            m2 += (1 - b2) * g * g
            p -= lr / (1 - b1 ** it) * m1 / (np.sqrt(m2) / math.sqrt(1 - b2 ** it) + eps)
    return losses, [m, rho, gam, hs[0], hs[1]]


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
# One update at gpcv_markov_ref.case_inputs; tests/test_gpcv_natgrad_host.py evaluates the same cases in fp32 and fp64 and
# checks the clamped-count cap, tests/test_gpu_gpcv_natgrad.py runs the kernel at them.
EXP_CASES = [(n, B, 0, "plain") for n, B in MR.SHAPES + MR.BOUNDARIES]
CV_CASES = [(n, B, Kc, "plain") for Kc in (1, 5, 8) for n, B in ((65, 3), (257, 2), (2049, 1))]
KIND_CASES = [(130, 3, Kc, kind) for kind in ("floored", "clamped") for Kc in (0, 5)]
ALL_CASES = EXP_CASES + CV_CASES + KIND_CASES
BETAS = (1.0, 0.5)
SITE_TOL = 2e-3                       # the project's bound for what comes from the fp32 quadrature (GRAD_TOL)
_CASES = {}


def case_sites(n, B, beta):
    """Random non-zero input sites (lam1, lam2 >= 0) of the B series of a beta case."""
    g = np.random.default_rng(7000 + 13 * n + B)
    return [(g.standard_normal(n) * 3.0, g.uniform(0.0, 8.0, n)) for _ in range(B)]


def case(n, B, Kc=0, kind="plain", beta=1.0, random_sites=False):
    """(inputs, input sites, fp64 references, fp32-rows references, w_ell, w_kl) of a GPU case; computed once."""
    key = (n, B, Kc, kind, beta, random_sites)
    if key not in _CASES:
        ps, we, wk = MR.case_inputs(n, B, Kc, kind)
        ghx, ghw = MR.gauss_hermite(75)
        sites = case_sites(n, B, beta) if random_sites else [(np.zeros(n), np.zeros(n)) for _ in range(B)]
        run = lambda p, s, dt: update(p["x"], p["v"], MR.J, p["mu"], p["m"], p["rho"], p["gam"], p["y"], ghx, ghw, we, wk,
                                      s[0], s[1], beta, abc=p["abc"], dtype=dt)
        _CASES[key] = (ps, sites, [run(p, s, np.float64) for p, s in zip(ps, sites)],
                       [run(p, s, np.float32) for p, s in zip(ps, sites)], we, wk)
    return _CASES[key]


def site_scales(refs):
    """The largest |lam1| and |lam2| of a case's reference ARRAYS [B,N]: what SITE_TOL is a share of.  Not the series' own
    largest: the fp32 quadrature's error in dE/ds is absolute (about 1e-7, the rounding of 75 terms of order 1 that cancel),
    and at N = 1 a series' only gv can be a thousand times smaller than that of its neighbours in the batch."""
    return {k: max(max(np.abs(r[k]).max() for r in refs), 1e-300) for k in ("lam1", "lam2")}


def rows_effect(refs, refs32):
    """Per CASE: the difference between update(dtype=float32) and update(dtype=float64) in m, rho, gamma, as a share of the
    series' largest entry, the worst of the case's series."""
    return {k: max(np.abs(r32[k] - r[k]).max() / max(np.abs(r[k]).max(), 1e-300) for r, r32 in zip(refs, refs32))
            for k in ("m", "rho", "gam")}


def bounds(ref, scales, effect):
    """The GPU bounds of one series: sites SITE_TOL of the reference array's largest entry (``site_scales``); m, rho, gamma
    one fp32 rounding plus 8 x the case's ``rows_effect`` (the kernel sums the 75 nodes in another order than numpy), of the
    series' largest entry."""
    out = {k: SITE_TOL * scales[k] for k in ("lam1", "lam2")}
    for k in ("m", "rho", "gam"):
        out[k] = (2.0 ** -23 + 8.0 * effect[k]) * np.abs(ref[k]).max()
    return out


def doubtful(ref, ref32):
    """Points whose clamp decision (gv > 0) the fp32 quadrature cannot be held to: |gv| under the bound a gv of the kernel
    is held to -- one fp32 rounding of the largest plus 8 x the effect of fp32 rows on the CPU, the rule of ``bounds`` (the
    sites' own bound, SITE_TOL of the largest site, would leave out 11 % of the points of the cases here: gv is heavy-tailed).
    A gv of exactly 0 (a floored variance) is never in doubt."""
    thr = 2.0 ** -23 * np.abs(ref["gv"]).max() + 8.0 * np.abs(ref32["gv"] - ref["gv"]).max()
    return (np.abs(ref["gv"]) < thr) & (ref["gv"] != 0)
