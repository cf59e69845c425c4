"""fp64 restatement of the multi-task GPCV ELBO with the copula-process ("cv") likelihood, ONE WARP PER TASK
(multi_task_variational_gp.py:58-69 over volatility_likelihood.py:19-22,45-47 with [T,K] parameters), shared by
tests/test_mt_gpcv_cv_host.py and tests/test_gpu_mt_gpcv_cv.py.  Not a test module.

    scale_t(f) = sum_k a_tk softplus(b_tk f + c_tk),   y_nt | f ~ N(0, max(scale_t(f), 1e-3))
    a = softplus(raw_a),  b = 3 sigmoid(raw_b),  c = 6 sigmoid(raw_c) - 3          (gpcv_cv_ref.constrain, raws [T,K])
    F = w_ell ell - w_kl KL

The KL and every piece of it are ``mt_gpcv_ref.struct`` / ``dense`` untouched; only the likelihood term is replaced.
``wrong`` names the three mistakes the multi-task "cv" pass can make that no other kernel can (the negative controls of the
host test): "next_task" evaluates task t with the warp of task t + 1, "floor" lets the variance derivative through where the
variance is floored (the value is unchanged), and "no_f" -- applied to the gradients, see ``value_and_grads`` -- drops the
factor f from d/db, which leaves d/dc in its place."""
import collections
import functools
import math

import torch

import gpcv_cv_ref as CV
import mt_gpcv_ref as R

RAW_KEYS = ("raw_a", "raw_b", "raw_c")
ABC_KEYS = ("lik_a", "lik_b", "lik_c")      # dF/d(a,b,c) in a gradient dict ("c" alone is the mean constants' gradient)
TOL_ABC = 2e-3                      # tests/test_gpu_gpcv_cv.py's bound on grad_a, grad_b, grad_c


def draw_raws(T, K, seed, dtype=torch.float64, spread=True):
    """[T,K] raws.  spread=False: VolatilityGaussianLikelihood's own draws (U(0,1), 0.1 U(0,1), U(0,1)); True: per-task
    offsets on top, so that neighbouring tasks have visibly different warps (the "next_task" control must show)."""
    g = torch.Generator().manual_seed(seed)
    ra, rb, rc = torch.rand(T, K, generator=g), 0.1 * torch.rand(T, K, generator=g), torch.rand(T, K, generator=g)
    if spread:
        t = torch.arange(T).reshape(T, 1).float()
        ra, rb, rc = ra - 1.5 + 1.3 * (t % 3), rb - 1.0 + 0.8 * (t % 2), rc - 0.5 + 0.6 * ((t + 1) % 3)
    return {"raw_a": ra.to(dtype), "raw_b": rb.to(dtype), "raw_c": rc.to(dtype)}


def warp(f, a, b, c):
    """f [..., T] -> sum_k a_tk softplus(b_tk f + c_tk), unclamped; a, b, c [T,K]."""
    return (torch.nn.functional.softplus(b * f.unsqueeze(-1) + c) * a).sum(-1)


def ell_abc(p, y, abc, Q=R.NUM_GH, wrong=None):
    """sum_nt GH_Q[log N(y_nt; 0, max(scale_t(f), MIN_SCALE))], f ~ N(m_nt, max(var_nt, MIN_VAR)), on the TRANSFORMED
    a, b, c [T,K] (so that autograd returns what the step returns, d/d(a,b,c)), and the share of nodes under the clamp."""
    x, w = R.gauss_hermite(Q, p["m"].dtype)
    var = R._var(p)
    floored = var.clamp_min(R.MIN_VAR)
    if wrong == "floor":
        floored = var + (floored - var).detach()
    a, b, c = abc
    if wrong == "next_task":
        a, b, c = (t.roll(-1, 0) for t in (a, b, c))
    f = (p["m"][..., None] + torch.sqrt(2 * floored)[..., None] * x).movedim(-1, 0)           # [Q,N,T]
    s = warp(f, a, b, c)
    sc = s.clamp(min=R.MIN_SCALE)
    lp = -0.5 * (y / sc) ** 2 - sc.log() - 0.5 * math.log(2 * math.pi)
    return (lp * w.reshape(-1, 1, 1)).sum(), float((s <= R.MIN_SCALE).double().mean())


def ell(p, y, raws, Q=R.NUM_GH, wrong=None):
    return ell_abc(p, y, CV.constrain(*(raws[k] for k in RAW_KEYS)), Q, wrong)


def _with_cv(fn, p, x, y, raws, K=None, kernel="bm", Q=R.NUM_GH, w_ell=None, w_kl=None, wrong=None):
    t = dict(fn(p, x, y, K=K, kernel=kernel, Q=Q, w_ell=w_ell, w_kl=w_kl))
    e, clamped = ell(p, y, raws, Q, wrong)
    t.update(ell=e, F=R._objective(e, t["kl"], *y.shape, w_ell, w_kl), clamped=clamped)
    return t


def dense(p, x, y, raws, **kw):
    return _with_cv(R.dense, p, x, y, raws, **kw)


def struct(p, x, y, raws, **kw):
    return _with_cv(R.struct, p, x, y, raws, **kw)


def value_and_grads(fn, p, x, y, raws, kernel="bm", K=None, with_K=False, wrong=None, Q=R.NUM_GH, w_ell=None, w_kl=None):
    """As mt_gpcv_ref.value_and_grads (fn = dense / struct of this module) with the three likelihood arrays besides:
    (terms, {name: dF/d name}), "lik_a", "lik_b", "lik_c" = dF/d(a,b,c) [T,K] at the transformed values, which is what the
    step returns ("c" alone is the mean constants' gradient, as in mt_gpcv_ref)."""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    abc = [t.detach().clone().requires_grad_(True) for t in CV.constrain(*(raws[k] for k in RAW_KEYS))]
    with_K = with_K or K is not None
    if with_K:
        K = (R.data_cov(x, p["raw_vol"].detach(), kernel) if K is None else K).detach().clone().requires_grad_(True)
    t = dict((R.struct if fn is struct else R.dense)(q, x, y, K=K, kernel=kernel, Q=Q, w_ell=w_ell, w_kl=w_kl))
    e, clamped = ell_abc(q, y, abc, Q, wrong if wrong != "no_f" else None)
    F = R._objective(e, t["kl"], *y.shape, w_ell, w_kl)
    t.update(ell=e, F=F, clamped=clamped)
    names = [k for k in R.KEYS if not (with_K and k == "raw_vol")]
    leaves = [q[k] for k in names] + abc + ([K] if with_K else [])
    gs = torch.autograd.grad(F, leaves)
    grads = dict(zip(names + list(ABC_KEYS) + (["K"] if with_K else []), [g.detach() for g in gs]))
    if wrong == "no_f":
        grads["lik_b"] = grads["lik_c"].clone()
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in t.items()}, grads


def raw_grads(p, x, y, raws, fn=None, **kw):
    """dF/d(raw_a, raw_b, raw_c) by autograd straight through the constraints (what VariationalELBO.backward must give)."""
    rs = {k: v.detach().clone().requires_grad_(True) for k, v in raws.items()}
    t = (fn or struct)({k: v.detach() for k, v in p.items()}, x, y, rs, **kw)
    return dict(zip(RAW_KEYS, torch.autograd.grad(t["F"], [rs[k] for k in RAW_KEYS])))


def ell_and_abc_grads(p, y, raws, Q=R.NUM_GH):
    """The O(N T Q K) part alone: (ell, {"lik_a", "lik_b", "lik_c": d ell / d(a,b,c)}) -- for shapes whose N^3 part is out of reach."""
    abc = [t.detach().clone().requires_grad_(True) for t in CV.constrain(*(raws[k] for k in RAW_KEYS))]
    e, _ = ell_abc({k: v.detach() for k, v in p.items()}, y, abc, Q)
    return e.detach(), dict(zip(ABC_KEYS, torch.autograd.grad(e, abc)))


def init_variational_cv(x, y, raws, vol=0.2, kernel="bm"):
    """multi_task_variational_gp.py:38-88 on the "cv" branch (:58-69), K = 1, y [N,T], raws [T,1] -> (f [N,T], S_root [N,N]
    (full, x10), constants [T]).  Quirks kept: ``y = f.t()`` replaces the returns by the log running std; no clamp on the
    diag_embed-ed inverse Hessian (zeros off the diagonal survive the mean over tasks); root_inv_decomposition on its
    Cholesky route; kuu gets gpytorch's jitter ladder only if it needs it."""
    N, T = y.shape
    rs = torch.full((N, T), float("nan"), dtype=y.dtype)
    for i in range(2, N):
        rs[i] = y[:i].std(0)
    rs[:10] = rs[10]
    a, b, c = CV.constrain(*(raws[k].to(y.dtype) for k in RAW_KEYS))          # [T,1]
    yl = rs.clamp(min=1e-4).log().T                                            # [T,N]
    f = ((yl / a).exp() - 1 - c) / b
    sigma = warp(f.T, a, b, c).clamp(min=R.MIN_SCALE).T                        # likelihood(f.t()).scale.t()
    scaling = ((2 + 3 * yl.pow(2.0)) * (a * b.pow(2.0) / 2)).pow(-1.0)
    ih = torch.diag_embed(scaling * sigma.pow(2.0) * (1 + torch.cosh(b * yl + c))).mean(0)
    kuu = R.data_cov(x, torch.logit(torch.tensor([vol], dtype=x.dtype)), kernel)
    L, info = torch.linalg.cholesky_ex(kuu)
    jit = 1e-8 if x.dtype == torch.float64 else 1e-6
    while info.any():
        L, info = torch.linalg.cholesky_ex(kuu + jit * torch.eye(N, dtype=x.dtype))
        jit *= 10
    inner = L.T @ ih @ L + torch.eye(N, dtype=x.dtype)
    C = torch.linalg.cholesky(inner)
    S_root = L @ torch.linalg.solve_triangular(C, torch.eye(N, dtype=x.dtype), upper=False).T
    return f.T.contiguous(), S_root * 10.0, rs.clamp(min=1e-4).mean(0).log()


def pred_scale(p, eps, raws):
    """LearnGPCVMultitask's return for the "cv" likelihood: mean over the samples F = M + Lx E Lt' (E [S,N,T]) of
    max(scale_t(F), 1e-3), as [T,N]."""
    F = p["m"] + p["Lx"].tril() @ eps @ p["Lt"].tril().T
    a, b, c = CV.constrain(*(raws[k] for k in RAW_KEYS))
    return warp(F, a, b, c).clamp(min=R.MIN_SCALE).mean(0).T


def fit(x, yy, start, raws, iters, lr=0.01, kernel="bm", train_likelihood=True):
    """fp64 Adam on -F from ``start`` (a parameter dict) and the raws: (losses, parameters, raws)."""
    ps = {k: v.detach().clone().double().requires_grad_(True) for k, v in start.items()}
    rs = {k: v.detach().clone().double().requires_grad_(bool(train_likelihood)) for k, v in raws.items()}
    opt = torch.optim.Adam(list(ps.values()) + (list(rs.values()) if train_likelihood else []), lr=lr)
    rec = []
    for _ in range(iters):
        opt.zero_grad()
        loss = -struct(ps, x, yy, rs, kernel=kernel)["F"]
        loss.backward()
        rec.append(float(loss.detach()))
        opt.step()
    return rec, {k: v.detach() for k, v in ps.items()}, {k: v.detach() for k, v in rs.items()}


# ------------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_mt_gpcv_cv.py, named so that tests/test_mt_gpcv_cv_host.py can put the fp32 CPU evaluation of
# ``struct`` through half of the same bounds first, and the three negative controls through ten times them.
Case = collections.namedtuple("Case", "N T K kernel x0 dk Q w_ell w_kl clamp seed",
                              defaults=(5, "bm", 1, False, R.NUM_GH, None, None, None, None))
STEP_CASES = tuple(Case(N, T) for N, T in ((33, 1), (200, 3), (399, 64), (640, 5), (1024, 8))) + (
    Case(399, 8, dk=True), Case(200, 3, K=1), Case(200, 3, K=8), Case(399, 8, K=1), Case(399, 8, K=8), Case(200, 3, x0=0),
    Case(257, 4, kernel="fbm", dk=True))
EDGE_N, EDGE_T = (1, 2, 15, 16, 17, 31, 33, 129), (1, 2, 3, 17, 63, 64)
EDGE_CASES = tuple(Case(N, T) for N in EDGE_N for T in EDGE_T)
Q_CASES = tuple(Case(33, 3, Q=Q) for Q in (1, 20, 75))
W_CASE = Case(129, 3, w_ell=0.37, w_kl=2.5)
# "clamp": tril(Lx) x CLAMP_FACTOR, so that the nodes reach far enough down for sum_k a_k softplus(b_k f + c_k) <= 1e-3;
# "floor": every third row of Lx x 1e-4 and row 1 of Lt x 1e-4 -- rows of Lx floored at every t, task 1 floored at every n
CLAMP_FACTOR = 10.0
CLAMP_CASE, FLOOR_CASE = Case(200, 3, clamp="clamp", seed=41), Case(200, 3, clamp="floor", seed=41)
ALL_CASES = STEP_CASES + EDGE_CASES + Q_CASES + (W_CASE, CLAMP_CASE, FLOOR_CASE)
# both sides of the reduction's staging edge: cv_abc_reduce_kernel's 256 threads take the 256 / 257 workgroup partials
REDUCE_CASES = (Case(4096, 2), Case(4112, 2))


NEAR_CLAMP = 4e-3                   # the floor case puts the scale of its floored rows here: 4 x MIN_SCALE, every node live


def _solve_scale(raws, target):
    """f_t with scale_t(f_t) = target, by bisection (scale_t is increasing: a, b > 0)."""
    a, b, c = CV.constrain(*(raws[k] for k in RAW_KEYS))
    lo, hi = torch.full((a.shape[0],), -60.0, dtype=a.dtype), torch.full((a.shape[0],), 20.0, dtype=a.dtype)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        up = warp(mid, a, b, c) < target
        lo, hi = torch.where(up, mid, lo), torch.where(up, hi, mid)
    return 0.5 * (lo + hi)


@functools.lru_cache(maxsize=None)
def make(cs):
    """The inputs of a Case: p, x, y, K, raws (fp64), and the keywords (Q, w_ell, w_kl) of the reference.  R.case draws the
    tasks alike; here task t's data is scaled by 0.5 (1 + t mod 4) and its mean shifted by 0.5 (t mod 3 - 1), and the warps
    differ from task to task (``draw_raws``), so that a task evaluated with its neighbour's warp shows in the totals."""
    seed = 100 + cs.N + cs.T if cs.seed is None else cs.seed
    p, x, y = R.case(cs.N, cs.T, seed=seed, x0=cs.x0)
    t = torch.arange(cs.T)
    y = y * (0.5 * (1 + t % 4)).to(y.dtype)
    p["m"] = p["m"] + 0.5 * (t % 3 - 1).to(y.dtype)
    raws = draw_raws(cs.T, cs.K, seed + 1)
    if cs.clamp:
        low, junk = p["Lx"].tril(), p["Lx"].triu(1)
        if cs.clamp == "clamp":
            low = low * CLAMP_FACTOR
        else:
            # rows of Lx floored at every t and task 1 floored at every n (x 2e-3: var ~ 5e-7), with the scale of the floored
            # (n, t) just above the clamp, where d ell / d var is large (y^2 / scale^2 ~ 10^4): a variance derivative let
            # through the floor then shows against the largest entry of grad_Lx and of grad_Lt
            low[::3] *= 2e-3
            p["Lt"][1, :2] *= 2e-3
            near = _solve_scale(raws, NEAR_CLAMP)
            p["m"][::3] = near
            p["m"][:, 1] = near[1]
            y[:, 1] *= 2.0
        p["Lx"] = low + junk
    return dict(p=p, x=x, y=y, K=R.data_cov(x, p["raw_vol"], cs.kernel), raws=raws,
                kw=dict(Q=cs.Q, w_ell=cs.w_ell, w_kl=cs.w_kl))


def weights(cs):
    return (1.0 / cs.N if cs.w_ell is None else cs.w_ell), (1.0 / (cs.N * cs.T) if cs.w_kl is None else cs.w_kl)


@functools.lru_cache(maxsize=None)
def reference(cs, wrong=None):
    """(terms, grads) of ``struct`` in fp64 with dF/dK and dF/d(a,b,c).  Computed once per Case."""
    c = make(cs)
    return value_and_grads(struct, c["p"], c["x"], c["y"], c["raws"], K=c["K"], wrong=wrong, **c["kw"])


def restate_f32(cs):
    """``struct`` and its autograd gradients evaluated in fp32 on the CPU: (out [13] in R.SCALAR_KEYS order, grads), fp64."""
    c = make(cs)
    f = lambda t: t.float()
    terms, grads = value_and_grads(struct, {k: f(v) for k, v in c["p"].items()}, f(c["x"]), f(c["y"]),
                                   {k: f(v) for k, v in c["raws"].items()}, K=f(c["K"]), **c["kw"])
    return torch.stack([terms[k].double() for k in R.SCALAR_KEYS]), {k: v.double() for k, v in grads.items()}


def ratios(cs, out, g, ref=None):
    """error / bound of every quantity (<= 1 passes) against ``reference(cs)`` (or ``ref``): the 13 scalars ``out`` at
    R.TOL_SCALAR max(1, |ref|); the gradients ``g`` (m, Lx, Lt, F, raw_var, c, lik_a, lik_b, lik_c and, where the case asks,
    K) at R.TOL_GRAD of the array's largest reference entry (K: R.TOL_GRAD_K; lik_*: TOL_ABC, over all tasks)."""
    terms, grads = reference(cs) if ref is None else ref
    out = out.double().reshape(-1)
    r = {k: abs(float(out[i] - terms[k])) / (R.TOL_SCALAR * max(1.0, abs(float(terms[k])))) for i, k in enumerate(R.SCALAR_KEYS)}
    for k in R.GRAD_KEYS + ABC_KEYS + (("K",) if cs.dk else ()):
        want = grads[k]
        tol = R.TOL_GRAD_K if k == "K" else TOL_ABC if k in ABC_KEYS else R.TOL_GRAD
        r["grad_" + k] = float((g[k].reshape(want.shape) - want).abs().max() / want.abs().max()) / tol
    return r


def group_max(r):
    """The largest error / bound per group: scalars, variational gradients, grad_K, likelihood gradients."""
    grp = lambda k: ("grad_K" if k == "grad_K" else "grad_abc" if k[5:] in ABC_KEYS else "grads" if k.startswith("grad_")
                     else "scalars")
    out = {}
    for k, v in r.items():
        out[grp(k)] = max(out.get(grp(k), 0.0), v) if v == v else float("nan")
    return out
