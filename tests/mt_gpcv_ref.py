"""fp64 restatements of the multi-task GPCV ELBO (MultitaskVariationalGP, voltron/models/multi_task_variational_gp.py),
shared by tests/test_mt_gpcv_host.py, tests/test_gpu_mt_gpcv.py and tests/test_gpu_mt_gpcv_kernel.py (whose inputs, oracle
and bounds are the named Cases at the end).  Not a test module.

    q(F) = N(M, S_x (x) S_t),  p(F) = N(mu, (K_x + j I) (x) K_t),  mu[n,t] = c_t,  element (n,t) of vec F at n T + t
    F    = ell / N - KL / (N T)

* ``dense``  : the definition -- torch.kron of both covariances, the NT x NT Cholesky, the textbook Gaussian KL.
* ``struct`` : the Kronecker-structured form the HIP step implements (one N x N and one T x T factorisation).  The host
  test checks the two against each other (value and all autograd gradients) at small sizes; the structured form is then
  the oracle at sizes where NT x NT is out of reach.
Parameters travel as a dict: m [N,T], Lx [N,N], Lt [T,T] (what lies above the diagonals is ignored), c [T], raw_vol [1],
F [T,1] (covar_factor), raw_var [T]."""
import collections
import functools
import math

import numpy as np
import torch
import torch.nn.functional as Fn

JITTER = 1e-3
MIN_VAR = 1e-6
MIN_SCALE = 1e-3
NUM_GH = 75
KEYS = ("m", "Lx", "Lt", "c", "raw_vol", "F", "raw_var")


def gauss_hermite(n, dtype=torch.float64):
    """numpy hermgauss nodes and weights / sqrt(pi) (GaussHermiteQuadrature1D)."""
    x, w = np.polynomial.hermite.hermgauss(n)
    return torch.tensor(x, dtype=dtype), torch.tensor(w / math.sqrt(math.pi), dtype=dtype)


def ell_fn(m, var, y, Q=NUM_GH):
    x, w = gauss_hermite(Q, m.dtype)
    var = var.clamp_min(MIN_VAR)
    f = m[..., None] + torch.sqrt(2 * var)[..., None] * x
    s = f.exp().clamp(min=MIN_SCALE)
    lp = -0.5 * (y[..., None] / s) ** 2 - s.log() - 0.5 * math.log(2 * math.pi)
    return (lp * w).sum(-1).sum()


def data_cov(x, raw_vol, kernel="bm"):
    vol = torch.sigmoid(raw_vol).reshape(())
    a, b = x[:, None], x[None, :]
    if kernel == "bm":
        return vol * torch.minimum(a, b)
    h2 = 2.0 * vol
    return (a.abs().pow(h2) + b.abs().pow(h2) - (a - b).abs().pow(h2)) / 2.0


def task_cov(p):
    return p["F"] @ p["F"].T + torch.diag(Fn.softplus(p["raw_var"]))


def case(N, T, seed, x0=1, dt=torch.float64):
    """Seeded inputs: x = (arange(N) + x0) / 252, junk above both diagonals, covar_factor of both signs."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=dt)
    x = (torch.arange(N, dtype=dt) + x0) / 252
    Lx = (torch.eye(N, dtype=dt) * 0.3 + 0.1 * r(N, N) / math.sqrt(N)).tril() + torch.triu(r(N, N), 1)
    Lt = (torch.eye(T, dtype=dt) + 0.2 * r(T, T)).tril() + torch.triu(r(T, T), 1)
    F = 0.5 * r(T, 1)
    if T > 1:
        F[0], F[1] = F[0].abs() + 0.1, -F[1].abs() - 0.1
    p = dict(m=-1.5 + 0.3 * r(N, T), Lx=Lx, Lt=Lt, c=-1.5 + 0.1 * r(T), raw_vol=torch.tensor([-1.0], dtype=dt), F=F,
             raw_var=r(T) - 1)
    y = r(N, T) * 0.25
    return p, x, y


def _var(p):
    Lx, Lt = p["Lx"].tril(), p["Lt"].tril()
    return (Lx ** 2).sum(-1)[:, None] * (Lt ** 2).sum(-1)[None, :]


def _ell(p, y, Q=NUM_GH):
    return ell_fn(p["m"], _var(p), y, Q)


def _objective(e, kl, N, T, w_ell, w_kl):
    """F = w_ell ell - w_kl KL; the model's weights 1/N and 1/(N T) unless others are given."""
    return (1.0 / N if w_ell is None else w_ell) * e - (1.0 / (N * T) if w_kl is None else w_kl) * kl


def dense(p, x, y, K=None, kernel="bm", j=JITTER, Q=NUM_GH, w_ell=None, w_kl=None):
    N, T = y.shape
    K = data_cov(x, p["raw_vol"], kernel) if K is None else K
    Kj = K + j * torch.eye(N, dtype=K.dtype)
    Lx, Lt = p["Lx"].tril(), p["Lt"].tril()
    P = torch.kron(Kj, task_cov(p))
    S = torch.kron(Lx @ Lx.T, Lt @ Lt.T)
    r = (p["m"] - p["c"][None, :]).reshape(-1)
    LP = torch.linalg.cholesky(P)
    kl = 0.5 * (torch.cholesky_solve(S, LP).diagonal().sum() + r @ torch.cholesky_solve(r[:, None], LP)[:, 0] - N * T
                + 2 * LP.diagonal().log().sum() - torch.logdet(S))
    e = _ell(p, y, Q)
    return {"F": _objective(e, kl, N, T, w_ell, w_kl), "ell": e, "kl": kl}


def struct(p, x, y, K=None, kernel="bm", j=JITTER, Q=NUM_GH, w_ell=None, w_kl=None):
    N, T = y.shape
    K = data_cov(x, p["raw_vol"], kernel) if K is None else K
    Kj = K + j * torch.eye(N, dtype=K.dtype)
    Kt = task_cov(p)
    Lx, Lt = p["Lx"].tril(), p["Lt"].tril()
    L, C = torch.linalg.cholesky(Kj), torch.linalg.cholesky(Kt)
    R = p["m"] - p["c"][None, :]
    tau_x = (torch.linalg.solve_triangular(L, Lx, upper=False) ** 2).sum()
    tau_t = (torch.linalg.solve_triangular(C, Lt, upper=False) ** 2).sum()
    A = torch.cholesky_solve(R, L)
    q = torch.cholesky_solve(R.T @ A, C).diagonal().sum()
    ld_k, ld_kt = 2 * L.diagonal().log().sum(), 2 * C.diagonal().log().sum()
    ld_sx, ld_st = (Lx.diagonal() ** 2).log().sum(), (Lt.diagonal() ** 2).log().sum()
    kl = 0.5 * (tau_x * tau_t + q - N * T + T * ld_k + N * ld_kt - T * ld_sx - N * ld_st)
    e = _ell(p, y, Q)
    with torch.no_grad():
        Kinv = torch.cholesky_inverse(L)
        extra = {"tr_kinv": Kinv.diagonal().sum(), "gg": ((Kinv @ Lx) ** 2).sum(),
                 "tr_aa": torch.cholesky_solve(A.T @ A, C).diagonal().sum()}
    return {"F": _objective(e, kl, N, T, w_ell, w_kl), "ell": e, "kl": kl, "q": q, "ld_k": ld_k, "ld_kt": ld_kt, "ld_sx": ld_sx,
            "ld_st": ld_st, "tau_x": tau_x, "tau_t": tau_t, **extra}


def value_and_grads(fn, p, x, y, kernel="bm", with_K=False, K=None, **kw):
    """fn = dense / struct.  Returns (terms, {name: gradient of F}); with_K adds "K" = dF/dK (K detached from raw_vol).
    ``K``: a prior covariance of the caller's in place of the kernel's (it implies with_K: there is no raw_vol behind it);
    ``kw`` (Q, w_ell, w_kl) goes to fn."""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    with_K = with_K or K is not None
    if with_K:
        K = (data_cov(x, p["raw_vol"].detach(), kernel) if K is None else K).detach().clone().requires_grad_(True)
    t = fn(q, x, y, K=K, kernel=kernel, **kw)
    names = [k for k in KEYS if not (with_K and k == "raw_vol")]
    gs = torch.autograd.grad(t["F"], [q[k] for k in names] + ([K] if with_K else []))
    grads = dict(zip(names + (["K"] if with_K else []), [g.detach() for g in gs]))
    return {k: v.detach() for k, v in t.items()}, grads


def scaled_returns(train_x, train_y):
    """train_utils.py:16-18 for train_y [T,N+1] -> [N,T]."""
    dt = train_x[1] - train_x[0]
    return ((train_y[:, 1:] - train_y[:, :-1]) / train_y[:, :-1] / dt ** 0.5).T.contiguous()


def init_variational(x, y, vol=0.2, kernel="bm"):
    """multi_task_variational_gp.py:38-88 ("exp"), y [N,T] -> (f [N,T], S_root [N,N] (full, x10), constants [T]).
    kuu gets gpytorch's jitter ladder only if it needs it (x[0] = 0); root_inv_decomposition on its Cholesky route."""
    N, T = y.shape
    rs = torch.full((N, T), float("nan"), dtype=y.dtype)
    for i in range(2, N):
        rs[i] = y[:i].std(0)
    rs[:10] = rs[10]
    f = rs.clamp(min=1e-4).log()
    ih = torch.diag_embed((0.5 * y.pow(-2.0) * (f * 2.0).exp()).T).clamp(min=1e-4, max=1000.0).mean(0)
    kuu = data_cov(x, torch.logit(torch.tensor([vol], dtype=x.dtype)), kernel)
    L, info = torch.linalg.cholesky_ex(kuu)
    jit = 1e-8 if x.dtype == torch.float64 else 1e-6
    while info.any():
        L, info = torch.linalg.cholesky_ex(kuu + jit * torch.eye(N, dtype=x.dtype))
        jit *= 10
    inner = L.T @ ih @ L + torch.eye(N, dtype=x.dtype)
    C = torch.linalg.cholesky(inner)
    S_root = L @ torch.linalg.solve_triangular(C, torch.eye(N, dtype=x.dtype), upper=False).T
    return f, S_root * 10.0, rs.clamp(min=1e-4).mean(0).log()


def fit(x, yy, start, iters, lr=0.01, kernel="bm"):
    """fp64 Adam on -F from ``start`` (a parameter dict): the loss of every iteration and the final parameters."""
    ps = {k: v.detach().clone().double().requires_grad_(True) for k, v in start.items()}
    opt = torch.optim.Adam(list(ps.values()), lr=lr)
    rec = []
    for _ in range(iters):
        opt.zero_grad()
        loss = -struct(ps, x, yy, kernel=kernel)["F"]
        loss.backward()
        rec.append(float(loss.detach()))
        opt.step()
    return rec, {k: v.detach() for k, v in ps.items()}


# ------------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_mt_gpcv_kernel.py, named so that tests/test_mt_gpcv_host.py can put the fp32 CPU evaluation
# of ``struct`` through the same bounds first: a bound the restatement itself misses in fp32 says nothing about the kernel.
Case = collections.namedtuple("Case", "prior N T x0 clamp Q w_ell w_kl seed", defaults=(1, None, NUM_GH, None, None, None))
SCALAR_KEYS = ("ell", "kl", "q", "ld_k", "ld_kt", "ld_sx", "ld_st", "tau_x", "tau_t", "tr_kinv", "gg", "tr_aa", "F")
GRAD_KEYS = ("m", "Lx", "Lt", "F", "raw_var", "c")
TOL_SCALAR, TOL_GRAD, TOL_GRAD_K = 5e-5, 2e-3, 5e-3         # tests/test_gpu_mt_gpcv.py's own

GENERIC_SHAPES = ((33, 1), (129, 3), (257, 4), (399, 8), (640, 5), (640, 64))
GENERIC_CASES = tuple(Case(k, N, T) for k in ("rbf", "wishart") for N, T in GENERIC_SHAPES)
# (a) root x 10: clamped nodes only; (b) every third row x 1e-3 and m[1::7] = -9: floored rows, fully clamped (n, t);
# (c) both (rows x 1e-4).  At (200, 3) on the model's prior, (c) again at (399, 8) on rbf.
CLAMP_CASES = tuple(Case("bm", 200, 3, clamp=c, seed=41) for c in "abc") + (Case("rbf", 399, 8, clamp="c", seed=41),)
CLAMP_SHARES = {"a": (0.0, 0.437), "b": (0.335, 0.126), "c": (0.335, 0.344)}     # (floored, clamped) at (200, 3)
EDGE_N, EDGE_T = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129), (1, 2, 15, 16, 17, 63, 64)
EDGE_SHAPES = tuple((N, T) for N in EDGE_N for T in EDGE_T if N * T <= 3000)


def edge_cases(N, T):
    return (Case("bm", N, T, 0), Case("bm", N, T, 1)) + ((Case("wishart", N, T),) if N >= 15 else ())


Q_CASES = tuple(Case("bm", 65, 17, Q=Q) for Q in (1, 20, 75))
W_CASE = Case("bm", 129, 3, w_ell=0.37, w_kl=2.5)
BM_DK_CASES = (Case("bm", 399, 8), Case("bm", 1024, 8))      # test_step_matches_oracle's, where grad_K is now checked
ALL_CASES = (GENERIC_CASES + CLAMP_CASES + tuple(c for s in EDGE_SHAPES for c in edge_cases(*s)) + Q_CASES + (W_CASE,)
             + BM_DK_CASES)


def prior(kind, N, seed):
    """"rbf" / "wishart" [N,N] fp64, exactly as the single-task suite takes them (rbf_irregular as it is, wishart x 2^-5)."""
    # (imported, not copied, so the two suites cannot drift apart; that module is GPU-marked but imports without a device:
    # at module level it needs only numpy, torch, spd_families, oracle.gpcv_oracle and volt_amd.synthetic)
    from test_gpu_gpcv import _prior
    return _prior(kind, torch.empty(N), None, seed)


def make(cs):
    """The inputs of a Case: p, x, y, K (fp64), and the keywords (Q, w_ell, w_kl) of the reference."""
    p, x, y = case(cs.N, cs.T, seed=100 + cs.N + cs.T if cs.seed is None else cs.seed, x0=cs.x0)
    if cs.clamp:
        low, junk = p["Lx"].tril(), p["Lx"].triu(1)
        if cs.clamp in "ac":
            low = low * 10
        if cs.clamp in "bc":
            low[::3] *= 1e-3 if cs.clamp == "b" else 1e-4
            p["m"][1::7] = -9.0
        p["Lx"] = low + junk
    K = data_cov(x, p["raw_vol"]) if cs.prior == "bm" else prior(cs.prior, cs.N, cs.N + cs.T)
    return dict(p=p, x=x, y=y, K=K, kw=dict(Q=cs.Q, w_ell=cs.w_ell, w_kl=cs.w_kl))


def weights(cs):
    return (1.0 / cs.N if cs.w_ell is None else cs.w_ell), (1.0 / (cs.N * cs.T) if cs.w_kl is None else cs.w_kl)


def clamp_stats(p, y, Q=NUM_GH):
    """Which branches of the quadrature pass a case takes, and how far from their thresholds: the shares of floored (n, t)
    (var < MIN_VAR) and of clamped nodes (exp f <= MIN_SCALE), the masks of rows floored at every t and of (n, t) clamped
    at every node, and the margin counts: nodes with |f - log MIN_SCALE| < 1e-5, variances within 0.1 % of MIN_VAR (where
    fp32 and fp64 could take different branches)."""
    x, _ = gauss_hermite(Q, p["m"].dtype)
    var = _var(p)
    floored = var < MIN_VAR
    f = p["m"][..., None] + torch.sqrt(2 * var.clamp_min(MIN_VAR))[..., None] * x
    clamped = f.exp() <= MIN_SCALE
    return dict(floored=float(floored.double().mean()), clamped=float(clamped.double().mean()),
                near_scale=int(((f - math.log(MIN_SCALE)).abs() < 1e-5).sum()),
                near_var=int(((var / MIN_VAR - 1).abs() < 1e-3).sum()),
                floored_rows=floored.all(1), all_clamped=clamped.all(-1))


@functools.lru_cache(maxsize=None)
def reference(cs):
    """(terms, grads) of ``struct`` in fp64 with dF/dK; for the model's prior also d/d raw_vol.  Computed once per Case."""
    c = make(cs)
    terms, grads = value_and_grads(struct, c["p"], c["x"], c["y"], K=c["K"], **c["kw"])
    if cs.prior == "bm":
        grads["raw_vol"] = value_and_grads(struct, c["p"], c["x"], c["y"], **c["kw"])[1]["raw_vol"]
    return terms, grads


@functools.lru_cache(maxsize=None)
def reference_kl_only(cs):
    """The gradients of -w_kl KL alone (w_ell = 0): what is left of grad_Lx in a row floored at every t, and of grad_M where
    every node is clamped."""
    c = make(cs)
    return value_and_grads(struct, c["p"], c["x"], c["y"], K=c["K"], **{**c["kw"], "w_ell": 0.0, "w_kl": weights(cs)[1]})[1]


def restate_f32(cs, kl_only=False):
    """``struct`` and its autograd gradients evaluated in fp32 on the CPU: (out [13] in SCALAR_KEYS order, grads), fp64.
    ``kl_only``: at w_ell = 0, as ``reference_kl_only``."""
    c = make(cs)
    f = lambda t: t.float()
    kw = {**c["kw"], "w_ell": 0.0, "w_kl": weights(cs)[1]} if kl_only else c["kw"]
    terms, grads = value_and_grads(struct, {k: f(v) for k, v in c["p"].items()}, f(c["x"]), f(c["y"]), K=f(c["K"]), **kw)
    return torch.stack([terms[k].double() for k in SCALAR_KEYS]), {k: v.double() for k, v in grads.items()}


def raw_vol_grad(cs, out):
    """d F / d raw_vol of the model's prior K = vol min(x, x') from the step's scalars, as the model forms it.  The jitter
    in that formula is the one the step applied: the fp32 value of 1e-3 (the step takes a float, and the model evaluates the
    formula on the fp32 ``out``), not the double 1e-3, which is 4.7e-8 away -- a fifth of the N = 1 bound of ``ratios``."""
    from volt_amd.variational import mt_dkl_dscale
    vol = torch.sigmoid(make(cs)["p"]["raw_vol"]).reshape(())
    dkl = mt_dkl_dscale(out, vol, cs.N, cs.T, jitter=float(np.float32(JITTER)))
    return -weights(cs)[1] * float(dkl) * float(vol * (1 - vol))


def _rows(a, r):
    """Largest error of a row over the row's largest reference entry."""
    return float(((a - r).abs().amax(1) / r.abs().amax(1)).max())


def ratios(cs, out, g):
    """error / bound of every quantity (<= 1 passes), for the 13 scalars ``out`` and the gradients ``g`` (m, Lx, Lt, F,
    raw_var, c, K; fp64 on the CPU).  Scalars: TOL_SCALAR max(1, |ref|); gradients: TOL_GRAD (K: TOL_GRAD_K) of the largest
    reference entry; on the model's prior d/d raw_vol: TOL_GRAD |ref|.  Clamp cases add grad_Lx and grad_M row by row."""
    terms, grads = reference(cs)
    out = out.double().reshape(-1)
    r = {k: abs(float(out[i] - terms[k])) / (TOL_SCALAR * max(1.0, abs(float(terms[k])))) for i, k in enumerate(SCALAR_KEYS)}
    for k in GRAD_KEYS + ("K",):
        ref = grads[k]
        r["grad_" + k] = float((g[k].reshape(ref.shape) - ref).abs().max() / ref.abs().max()) / (TOL_GRAD_K if k == "K" else TOL_GRAD)
    if cs.prior == "bm":
        ref = float(grads["raw_vol"])
        tol = TOL_GRAD * abs(ref)
        if cs.N == 1 and cs.x0 == 0:
            # K = vol min(0, 0) = 0 does not depend on vol: the gradient is exactly zero, and what is left is the rounding
            # of the fp32 scalars it is a difference of -- one rounding of each term, 2^-23 of the terms' magnitude
            # (tests/test_gpu_gpcv_bm.py, the same case).  No fp32 evaluation has much room under it: tr K^-1 alone goes
            # through four roundings (the jitter, its root, the reciprocal, the square) and arrives 1.5 x 2^-23 off.  The
            # fp32 CPU restatement sits at 0.1 .. 1.1 of this bound over T and seeds, the MI355X at 0.29 .. 0.94 at T =
            # 1, 2, 15, 16, 17, 63, 64.
            vol = float(torch.sigmoid(make(cs)["p"]["raw_vol"]))
            t = {k: abs(float(v)) for k, v in terms.items()}
            scale = 0.5 * (cs.T * cs.N + cs.T * JITTER * t["tr_kinv"] + t["tau_t"] * t["tau_x"] + t["tau_t"] * JITTER * t["gg"]
                           + t["q"] + JITTER * t["tr_aa"]) / vol
            tol = 2.0 ** -23 * weights(cs)[1] * scale * vol * (1 - vol)
        r["grad_raw_vol"] = abs(raw_vol_grad(cs, out) - ref) / tol
    if cs.clamp:
        N, T = cs.N, cs.T
        r["grad_Lx_rows"] = _rows(g["Lx"].reshape(N, N).tril(), grads["Lx"]) / TOL_GRAD
        r["grad_m_rows"] = _rows(g["m"].reshape(N, T), grads["m"]) / TOL_GRAD
    return r


def kl_only_ratios(cs, gLx, gM):
    """error / bound (TOL_GRAD of the row's largest reference entry) against the KL-only reference where the likelihood
    cannot contribute: the rows of grad_Lx floored at every t, the (n, t) of grad_M clamped at every node."""
    c = make(cs)
    s, ref = clamp_stats(c["p"], c["y"], cs.Q), reference_kl_only(cs)
    rows, nt = s["floored_rows"], s["all_clamped"]
    gLx, gM = gLx.double().reshape(cs.N, cs.N), gM.double().reshape(cs.N, cs.T)
    e_rows = ((gLx[rows] - ref["Lx"][rows]).abs().amax(1) / ref["Lx"][rows].abs().amax(1)).max()
    e_nt = ((gM[nt] - ref["m"][nt]).abs() / ref["m"].abs().amax(1, keepdim=True).expand(-1, cs.T)[nt]).max()
    return {"grad_Lx_floored_rows": float(e_rows) / TOL_GRAD, "grad_m_clamped": float(e_nt) / TOL_GRAD}


def over(r, limit=1.0):
    """The entries of a ratio dict that are not <= limit -- NaN among them (max() would skip one)."""
    return {k: v for k, v in r.items() if not v <= limit}
