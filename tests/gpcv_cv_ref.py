"""fp64 restatement of the GPCV ELBO with the copula-process ("cv") likelihood (volatility_likelihood.py:43-51),
shared by tests/test_gpcv_cv_host.py and tests/test_gpu_gpcv_cv.py.  Not a test module.

    scale(f) = sum_k a_k log(1 + exp(b_k f + c_k)),   y_i | f ~ N(0, max(scale(f), 1e-3))
    a = softplus(raw_a),  b = 3 sigmoid(raw_b),  c = 6 sigmoid(raw_c) - 3          (:24-26)
    F = w_ell ell - w_kl KL

Everything the likelihood does not touch -- quadrature nodes, the KL and its pieces, the kernels, the running std, the
jitter ladder -- is ``oracle.gpcv_oracle``'s.  Plain torch, any float dtype, gradients by autograd."""
import math

import torch
import torch.nn.functional as Fn

from oracle import gpcv_oracle as GO

MIN_SCALE = GO.MIN_SCALE


def constrain(raw_a, raw_b, raw_c):
    return Fn.softplus(raw_a), 3.0 * torch.sigmoid(raw_b), 6.0 * torch.sigmoid(raw_c) - 3.0


def draw_raw(K, seed, dtype=torch.float64):
    """raw_a, raw_b, raw_c as VolatilityGaussianLikelihood draws them: U(0,1), 0.1 U(0,1), U(0,1)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(K, generator=g).to(dtype), (0.1 * torch.rand(K, generator=g)).to(dtype),
            torch.rand(K, generator=g).to(dtype))


def warp(f, a, b, c):
    """sum_k a_k softplus(b_k f + c_k), unclamped; f [...], a, b, c [K]."""
    return (Fn.softplus(b * f.unsqueeze(-1) + c) * a).sum(-1)


def ell(m, Lq_raw, y, a, b, c, gh_x, gh_w):
    """sum_i E_{q(f_i)} log p(y_i | f_i) by Gauss-Hermite quadrature (gh_w still to be / sqrt(pi)), and the share of
    nodes under the min_scale clamp."""
    var = Lq_raw.tril().pow(2).sum(-1).clamp_min(GO.MIN_VARIANCE)
    locs = torch.sqrt(2.0 * var).unsqueeze(0) * gh_x.unsqueeze(-1) + m.unsqueeze(0)          # [Q, N]
    s = warp(locs, a, b, c)
    scale = s.clamp(min=MIN_SCALE)
    logp = -(y.unsqueeze(0) ** 2) / (2 * scale ** 2) - scale.log() - 0.5 * math.log(2 * math.pi)
    return ((logp * gh_w.unsqueeze(-1)).sum(0) / math.sqrt(math.pi)).sum(), float((s <= MIN_SCALE).double().mean())


def elbo_terms(m, Lq_raw, const, K, y, raw_a, raw_b, raw_c, gh_x, gh_w, w_ell=None, w_kl=None):
    """The pieces of GO.elbo_terms with the "cv" likelihood term; "elbo" = w_ell ell - w_kl KL (defaults 1/N, 1/N)."""
    N = y.shape[0]
    t = GO.elbo_terms(m, Lq_raw, const, K, y, gh_x, gh_w)                 # KL and its pieces (its "ell" is the "exp" one)
    e, clamped = ell(m, Lq_raw, y, *constrain(raw_a, raw_b, raw_c), gh_x, gh_w)
    w_ell = 1.0 / N if w_ell is None else w_ell
    w_kl = 1.0 / N if w_kl is None else w_kl
    t = dict(t)
    t.update(ell=e, elbo=w_ell * e - w_kl * t["kl"], clamped=clamped)
    return t


def elbo(m, Lq_raw, const, raw_vol, raws, x, y, kernel="bm", num_gh=GO.NUM_GH):
    gh_x, gh_w = GO.gauss_hermite(num_gh, dtype=m.dtype)
    vol = torch.sigmoid(raw_vol)
    K = GO.bm_cov(x, vol) if kernel == "bm" else GO.fbm_cov(x, vol)
    return elbo_terms(m, Lq_raw, const, K, y, *raws, gh_x, gh_w)["elbo"]


def init_variational_cv(x, y, raws, vol=0.2, kernel="bm"):
    """``initialize_variational_parameters`` for param == "cv", K = 1 (single_task_variational_gp.py:204-254), quirks kept:
    the returns are replaced by the log running std, no clamp, mean = ((y/a).exp() - 1 - c)/b.
    Returns (variational_mean, chol_variational_covar, mean constant)."""
    a, b, c = constrain(*raws)
    rs = GO.running_std(y)
    yl = rs.clamp(min=1e-4).log()
    f = ((yl / a).exp() - 1 - c) / b
    sigma = warp(f, a, b, c).clamp(min=MIN_SCALE)
    scaling = ((2 + 3 * yl.pow(2.0)) * (a * b.pow(2.0) / 2)).pow(-1.0)
    ih = torch.diag_embed(scaling * sigma.pow(2.0) * (1 + torch.cosh(b * yl + c)))
    volt = torch.as_tensor(vol, dtype=x.dtype)
    kuu = GO.bm_cov(x, volt) if kernel == "bm" else GO.fbm_cov(x, volt)
    L = GO.psd_safe_cholesky(kuu)
    inner = L.mT @ ih @ L + torch.eye(x.shape[0], dtype=x.dtype)
    S = L @ torch.cholesky_solve(L.mT.contiguous(), GO.psd_safe_cholesky(inner))
    return f, GO.psd_safe_cholesky(S).tril() * 10.0, rs.mean(0).log()


def pred_scale(m, Lq_raw, eps, raws):
    """train_utils.py:60-63 with the "cv" likelihood: mean over the samples f = m + Lq eps of max(scale(f), 1e-3)."""
    f = m.unsqueeze(0) + eps @ Lq_raw.tril().mT
    return warp(f, *constrain(*raws)).clamp(min=MIN_SCALE).mean(0)


def learn(x, yy, start, raws, iters, kernel="bm", train_likelihood=True, lr=0.01):
    """fp64 Adam on -ELBO from ``start`` = (variational mean, chol factor, mean constant); raw_vol starts at logit(0.2).
    Returns (losses, [m, Lq, const, raw_vol, raw_a, raw_b, raw_c])."""
    dt = torch.float64
    ps = [t.detach().clone().to(dt).requires_grad_(True) for t in (start[0], start[1], start[2].reshape(1))]
    ps.append(torch.logit(torch.tensor([0.2], dtype=dt)).requires_grad_(True))
    rs = [r.detach().clone().to(dt).requires_grad_(bool(train_likelihood)) for r in raws]
    opt = torch.optim.Adam(ps + (rs if train_likelihood else []), lr=lr)
    rec = []
    for _ in range(iters):
        opt.zero_grad()
        loss = -elbo(ps[0], ps[1], ps[2], ps[3], rs, x.to(dt), yy.to(dt), kernel=kernel)
        loss.backward()
        rec.append(float(loss.detach()))
        opt.step()
    return rec, [p.detach() for p in ps + rs]
