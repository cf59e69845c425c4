"""fp64 restatements of the multi-task GPCV ELBO (MultitaskVariationalGP, voltron/models/multi_task_variational_gp.py),
shared by tests/test_mt_gpcv_host.py and tests/test_gpu_mt_gpcv.py.  Not a test module.

    q(F) = N(M, S_x (x) S_t),  p(F) = N(mu, (K_x + j I) (x) K_t),  mu[n,t] = c_t,  element (n,t) of vec F at n T + t
    F    = ell / N - KL / (N T)

* ``dense``  : the definition -- torch.kron of both covariances, the NT x NT Cholesky, the textbook Gaussian KL.
* ``struct`` : the Kronecker-structured form the HIP step implements (one N x N and one T x T factorisation).  The host
  test checks the two against each other (value and all autograd gradients) at small sizes; the structured form is then
  the oracle at sizes where NT x NT is out of reach.
Parameters travel as a dict: m [N,T], Lx [N,N], Lt [T,T] (what lies above the diagonals is ignored), c [T], raw_vol [1],
F [T,1] (covar_factor), raw_var [T]."""
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


def _ell(p, y):
    Lx, Lt = p["Lx"].tril(), p["Lt"].tril()
    var = (Lx ** 2).sum(-1)[:, None] * (Lt ** 2).sum(-1)[None, :]
    return ell_fn(p["m"], var, y)


def dense(p, x, y, K=None, kernel="bm", j=JITTER):
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
    e = _ell(p, y)
    return {"F": e / N - kl / (N * T), "ell": e, "kl": kl}


def struct(p, x, y, K=None, kernel="bm", j=JITTER):
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
    e = _ell(p, y)
    with torch.no_grad():
        Kinv = torch.cholesky_inverse(L)
        extra = {"tr_kinv": Kinv.diagonal().sum(), "gg": ((Kinv @ Lx) ** 2).sum(),
                 "tr_aa": torch.cholesky_solve(A.T @ A, C).diagonal().sum()}
    return {"F": e / N - kl / (N * T), "ell": e, "kl": kl, "q": q, "ld_k": ld_k, "ld_kt": ld_kt, "ld_sx": ld_sx,
            "ld_st": ld_st, "tau_x": tau_x, "tau_t": tau_t, **extra}


def value_and_grads(fn, p, x, y, kernel="bm", with_K=False):
    """fn = dense / struct.  Returns (terms, {name: gradient of F}); with_K adds "K" = dF/dK (K detached from raw_vol)."""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    K = None
    if with_K:
        K = data_cov(x, p["raw_vol"].detach(), kernel).detach().requires_grad_(True)
    t = fn(q, x, y, K=K, kernel=kernel)
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
