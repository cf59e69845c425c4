"""fp64 restatement of the O(N^2) GPCV ELBO step for the Brownian-motion prior (csrc/gpcv_bm.hip, include/volt_hip.h:
volt_gpcv_bm_step_f32).  Shared by tests/test_gpcv_bm_host.py (the restatement against the dense oracle) and
tests/test_gpu_gpcv_bm.py (the HIP kernels against the restatement).  Not a test module.

A = v min(x, x') + j I = D^-1 T D^-T, T = L diag(d) L' (tests/bm_chain_ref.py: d_i, c_i = j / d_{i-1}); rho_i = j / d_i.
Column j of Lq is one chain solve:
    forward   z_i = (Lq_ij - Lq_{i-1,j}) + c_i z_{i-1}  from i = j;   tr(A^-1 S) = sum_j sum_{i>=j} z_ij^2 / d_i
    backward  w_i = z_i / d_i + rho_i w_{i+1},  G_ij = w_i - w_{i+1}  from N-1 down to j   (tril(G) only)
    |G|_F^2 = sum tril(G)^2 + sum_j w_jj^2 Q_j,   Q_0 = 0,  Q_{j+1} = rho_j^2 Q_j + (rho_j - 1)^2
r'A^-1 r, logdet A, tr A^-1, beta = A^-1 r and |beta|^2 are bm_chain_ref.bm_step_ref's.  The likelihood term and its
gradients are torch fp64 autograd through the definition ("exp": oracle.gpcv_oracle's; "cv": tests/gpcv_cv_ref.py's warp)."""
import math

import numpy as np
import torch

import bm_chain_ref as BM
import gpcv_cv_ref as CV

JITTER, MIN_VAR, MIN_SCALE = 1e-3, 1e-6, 1e-3


def problem(n, B, seed, x0_zero=False, irregular=True, nan_upper=True):
    """A small synthetic step: grid x [N], m, y, resid-defining mu [B,N] and Lq [B,N,N] whose strict upper triangle is NaN
    (it must never be read).  Everything fp64 but exactly representable in fp32."""
    rng = np.random.default_rng(seed)
    grid = BM.grids(n, np.random.default_rng(seed + 1))[("irregular_" if irregular else "uniform_") + ("zero" if x0_zero else "dt")]
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    x = f32(grid)
    m = f32(math.log(0.2) + 0.3 * rng.standard_normal((B, n)))
    mu = f32(np.full((B, n), math.log(0.2)) + 0.05 * rng.standard_normal((B, 1)))
    y = f32(rng.standard_normal((B, n)) * np.exp(m))
    L = 0.3 * rng.standard_normal((B, n, n)) / math.sqrt(n)
    L[:, np.arange(n), np.arange(n)] = rng.uniform(0.05, 0.4, size=(B, n))
    L = f32(np.tril(L))
    if nan_upper:
        L[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]] = np.nan
    return x, m, mu, y, L


def ell_and_grads(m, Lq, y, gh_x, gh_w, abc=None, min_var=MIN_VAR, min_scale=MIN_SCALE):
    """ell [B] and d ell / d(m, tril Lq, abc) by autograd; gh_w already / sqrt(pi).  m, y [B,N], Lq [B,N,N], abc [B,3,Kc]."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    mt, Lt = t(m).requires_grad_(True), t(np.tril(np.nan_to_num(Lq))).requires_grad_(True)
    yt, gx, gw = t(y), t(gh_x), t(gh_w)
    at = t(abc).requires_grad_(True) if abc is not None else None
    var = Lt.tril().pow(2).sum(-1).clamp_min(min_var)                                   # [B,N]
    locs = torch.sqrt(2.0 * var).unsqueeze(1) * gx.reshape(1, -1, 1) + mt.unsqueeze(1)   # [B,Q,N]
    if at is None:
        s = locs.exp()
    else:
        a, b, c = (at[:, k].reshape(at.shape[0], 1, 1, -1) for k in range(3))
        s = (torch.nn.functional.softplus(b * locs.unsqueeze(-1) + c) * a).sum(-1)
    scale = s.clamp(min=min_scale)
    logp = -(yt.unsqueeze(1) ** 2) / (2 * scale ** 2) - scale.log() - 0.5 * math.log(2 * math.pi)
    ell = (logp * gw.reshape(1, -1, 1)).sum((1, 2))
    grads = torch.autograd.grad(ell.sum(), [mt, Lt] + ([at] if at is not None else []))
    clamped = float((s <= min_scale).double().mean())
    return ell.detach().numpy(), [g.numpy() for g in grads], clamped


def kl_chain(x, vol, jitter, resid, Lq):
    """The KL's pieces by the recurrences.  Returns dict of [B] scalars, beta [B,N], tril(G) [B,N,N], info [B]."""
    vol = np.asarray(vol, np.float64).reshape(-1)
    B = vol.shape[0]
    n = len(x)
    s2 = np.full(B, float(jitter))
    d, c, s, info = BM._pivots(x, vol, s2)
    out8, beta, _ = BM.bm_step_ref(x, vol, s2, resid)
    L = np.tril(np.nan_to_num(np.asarray(Lq, np.float64).reshape(B, n, n)))
    rho = s[:, None] / d
    tr_s, gg = np.zeros(B), np.zeros(B)
    G = np.zeros((B, n, n))
    for b in range(B):
        u = np.diff(L[b], axis=0, prepend=0.0)                  # Lq_ij - Lq_{i-1,j}: zero above row j, Lq_jj at row j
        z = np.empty((n, n))
        z[0] = u[0]
        for i in range(1, n):
            z[i] = u[i] + c[b, i] * z[i - 1]
        z = np.tril(z)                                          # (the sweep of column j starts at row j)
        tr_s[b] = (z * z / d[b][:, None]).sum()
        w = np.zeros((n + 1, n))
        for i in range(n - 1, -1, -1):
            w[i] = np.where(np.arange(n) <= i, z[i] / d[b, i] + rho[b, i] * w[i + 1], 0.0)   # stops at row j
        G[b] = np.tril(w[:-1] - w[1:])                          # G_ij = w_i - w_{i+1}, i >= j
        Q = np.zeros(n)
        for j in range(n - 1):
            Q[j + 1] = rho[b, j] ** 2 * Q[j] + (rho[b, j] - 1.0) ** 2
        wd = w[np.arange(n), np.arange(n)]
        gg[b] = (G[b] ** 2).sum() + (wd * wd * Q).sum()
    lds = np.log(np.diagonal(L, axis1=1, axis2=2) ** 2).sum(1)
    quad, ldk, tr_inv, bb = out8[:, 2], out8[:, 3], out8[:, 4], out8[:, 5]
    kl = 0.5 * (tr_s + quad - n + ldk - lds)
    return dict(kl=kl, quad=quad, logdet_k=ldk, logdet_s=lds, tr_s=tr_s, tr_inv=tr_inv, gg=gg, bb=bb), beta, G, info, L


def step_ref(x, vol, resid, m, Lq, y, gh_x, gh_w, abc=None, jitter=JITTER, min_var=MIN_VAR, min_scale=MIN_SCALE, w_ell=1.0,
             w_kl=1.0):
    """What volt_gpcv_bm_step_f32 returns, in fp64: dict(out [B,12], grad_m, grad_mu, grad_Lq (zero above the diagonal),
    grad_abc or None, dvol [B] = dF/dvol, info, clamped)."""
    k, beta, G, info, L = kl_chain(x, vol, jitter, resid, Lq)
    ell, g, clamped = ell_and_grads(m, Lq, y, gh_x, gh_w, abc, min_var, min_scale)
    B, n = beta.shape
    F = w_ell * ell - w_kl * k["kl"]
    out = np.stack([ell, k["kl"], k["quad"], k["logdet_k"], k["logdet_s"], k["tr_s"], k["tr_inv"], k["gg"], k["bb"], F,
                    np.full(B, float(jitter)), np.zeros(B)], 1)
    idx = np.arange(n)
    dkl_dL = G.copy()
    dkl_dL[:, idx, idx] -= 1.0 / L[:, idx, idx]
    vol = np.asarray(vol, np.float64).reshape(-1)
    dkl_dv = 0.5 * ((n - jitter * k["tr_inv"]) - (k["tr_s"] - jitter * k["gg"]) - (k["quad"] - jitter * k["bb"])) / vol
    # the magnitude of the terms dF/dvol is a difference of (what its error is judged against)
    dv_scale = w_kl * 0.5 * (n + jitter * k["tr_inv"] + k["tr_s"] + jitter * k["gg"] + k["quad"] + jitter * k["bb"]) / vol
    return dict(out=out, grad_m=w_ell * g[0] - w_kl * beta, grad_mu=w_kl * beta, grad_Lq=w_ell * np.tril(g[1]) - w_kl * dkl_dL,
                grad_abc=w_ell * g[2] if abc is not None else None, dvol=-w_kl * dkl_dv, dvol_scale=dv_scale, info=info,
                clamped=clamped)


def out_scales(out, n, w_ell=1.0, w_kl=1.0):
    """The scale each of out[:, 0..9] is judged against: the magnitude of the terms it is a sum or a difference of."""
    a = np.abs(out)
    kl = 0.5 * (a[:, 5] + a[:, 2] + n + a[:, 3] + a[:, 4])
    return np.stack([np.maximum(a[:, 0], 1.0), kl, a[:, 2], np.maximum(a[:, 3], 1.0), np.maximum(a[:, 4], 1.0), a[:, 5], a[:, 6],
                     a[:, 7], a[:, 8], w_ell * np.maximum(a[:, 0], 1.0) + w_kl * kl], 1)
