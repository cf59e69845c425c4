"""fp64 restatement of the WHOLE linear-time Kronecker evaluation of MultitaskBMGP(solver="linear"): the
prologue's algebra with torch.linalg.eigh in place of the Jacobi solver, the chain recurrences of tests/bm_chain_ref.py per
eigen-direction (x, vol = 1, sigma2 = 1 / kappa_j, resid = r_j) in place of volt_bm_step_*, and the epilogue's formulas
(csrc/kron_shared.h, kron_epilogue_body) in numpy.  Shared by tests/test_multitask_linear_host.py (the restatement against
dense NT x NT fp64 autograd) and tests/test_gpu_multitask_linear.py (the split epilogue's inputs)."""
import numpy as np
import torch

import bm_chain_ref as ref

NAMES = ("raw_vol", "covar_factor", "raw_var", "raw_task_noises", "raw_noise")


def _softplus(v):
    return np.where(v > 20.0, v, np.log1p(np.exp(np.minimum(v, 20.0))))


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def prologue_ref(p, x, Y):
    """p: dict of the five raw parameters (anything np.asarray takes), x [N], Y [N,T] -> dict(vol, d, Kt, S, lam, Q, W, kappa,
    sigma2 [T], resid [T,N]) in fp64; eigenvalues ascending."""
    q = {k: np.asarray(v, np.float64).reshape(-1) for k, v in p.items()}
    x, Y = np.asarray(x, np.float64), np.asarray(Y, np.float64)
    vol = float(_sigmoid(q["raw_vol"][0]))
    f = q["covar_factor"]
    d = _softplus(q["raw_task_noises"]) + 1e-4 + float(_softplus(q["raw_noise"][0])) + 1e-4
    Kt = np.outer(f, f) + np.diag(_softplus(q["raw_var"]))
    S = Kt / np.sqrt(np.outer(d, d))
    lam, Q = torch.linalg.eigh(torch.from_numpy(S))
    lam, Q = lam.numpy(), Q.numpy()
    W = Q / np.sqrt(d)[:, None]
    kappa = vol * lam
    R = Y + 0.5 * vol * vol * x[:, None] * np.diag(Kt)[None, :]
    resid = ((R @ W) / np.sqrt(kappa)[None, :]).T.copy()
    return dict(vol=vol, d=d, Kt=Kt, S=S, lam=lam, Q=Q, W=W, kappa=kappa, sigma2=1.0 / kappa, resid=resid)


def epilogue_ref(p, x, pro, out, alpha):
    """The epilogue's formulas on the step's out [T,8] and alpha [T,N]: res [3 + 3T] = mll, d / d raw_vol, d / d raw_noise,
    d / d covar_factor [T], d / d raw_var [T], d / d raw_task_noises [T]."""
    q = {k: np.asarray(v, np.float64).reshape(-1) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    T, N = alpha.shape
    vol, lam, d, W, kap, r = pro["vol"], pro["lam"], pro["d"], pro["W"], pro["kappa"], pro["resid"]
    f = q["covar_factor"]
    sk = np.sqrt(kap)
    ar, aa, u = alpha @ r.T, alpha @ alpha.T, alpha @ x
    tau = out[:, 4] / kap
    P = ar * sk[None, :] / sk[:, None] - aa / np.outer(sk, sk)
    H = 0.25 * (P / lam[None, :] + P.T / lam[:, None]) - np.diag(0.5 * (N - tau) / lam)
    Q2 = aa / np.outer(sk, sk)
    G = W @ H @ W.T
    gd = 0.5 * np.diag(W @ Q2 @ W.T) - 0.5 * (W * W) @ tau
    ax = W @ (u / sk)
    G = G + np.diag(-0.5 * vol * vol * ax)
    scale = 1.0 / (N * T)
    logp = (N * out[:, 0] - 0.5 * N * np.log(kap) - 0.5 * N * np.log(d)).sum()
    quad = (np.diag(ar) - np.diag(aa) / kap).sum()
    tr = (N - tau).sum()
    mterm = (ax * (f * f + _softplus(q["raw_var"]))).sum()
    gvol = (0.5 * quad - 0.5 * tr) / vol - vol * mterm
    res = np.empty(3 + 3 * T)
    res[0] = logp * scale
    res[1] = gvol * vol * (1.0 - vol) * scale
    res[2] = gd.sum() * float(_sigmoid(q["raw_noise"][0])) * scale
    res[3:3 + T] = 2.0 * (G @ f) * scale
    res[3 + T:3 + 2 * T] = np.diag(G) * _sigmoid(q["raw_var"]) * scale
    res[3 + 2 * T:] = gd * _sigmoid(q["raw_task_noises"]) * scale
    return res


def kron_chain_ref(p, x, Y):
    """(mll, {name: gradient}) of the linear Kronecker evaluation, all fp64."""
    pro = prologue_ref(p, x, Y)
    T = pro["lam"].shape[0]
    out, alpha, info = ref.bm_step_ref(x, np.ones(T), pro["sigma2"], pro["resid"])
    assert not info.any(), info
    res = epilogue_ref(p, x, pro, out, alpha)
    return float(res[0]), unpack(res, T)


def unpack(res, T):
    res = np.asarray(res, np.float64)
    return {"raw_vol": res[1:2], "raw_noise": res[2:3], "covar_factor": res[3:3 + T].reshape(T, 1),
            "raw_var": res[3 + T:3 + 2 * T], "raw_task_noises": res[3 + 2 * T:]}
