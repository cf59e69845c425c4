"""Cases and yardsticks for the direct tests of the Kronecker multi-task step (csrc/kron.hip, csrc/kron_chain.hip,
csrc/kron_shared.h): parameter regimes that move the eigenvalues of S = D^-1/2 K_t D^-1/2 away from the O(1), all-distinct
spectrum of test_gpu_multitask.make_case, invariants that do not depend on the eigenvectors' signs or on the basis chosen
inside a tied cluster, and two fp32 references for the step -- a floor (nothing but the rounding of the interface) and a
yardstick (a vendor fp32 Cholesky in place of the step).  Host code only; shared by tests/test_kron_cases_host.py (conditions
on the references) and tests/test_gpu_kron_step.py (the kernels against them)."""
import math

import numpy as np
import torch

import bm_chain_ref as ref
import kron_chain_ref as kref
from test_gpu_multitask import make_case, oracle_mll

REGIMES = ("base", "scalar", "clusters", "correlated", "noisy", "linear_branch", "tiny_vol")
SHAPES = ((65, 3), (129, 8), (33, 63))          # (N, T) of the step tests: odd N, one / several / nearly all task slots
U32 = 2.0 ** -24                                # unit roundoff of fp32 (round to nearest)


def _inv_softplus(y):
    return math.log(math.expm1(y))


def regime(name, p, T):
    """A make_case parameter dict -> the same dict moved into regime ``name`` (dtype kept).
      base           unchanged: lambda in [0.5, 250], kappa in [0.2, 100], all distinct
      scalar         F = 0, one var, one task noise: S = c I -- no rotation in any sweep, every eigenvalue tied
      clusters       as scalar with var = softplus(-0.3) on the first T // 2 tasks and softplus(0.8) on the rest: two tied clusters
      correlated     F = 1 + 0.1 N(0,1), var = d_task = 1e-2, raw_noise = -12: one lambda ~ |F|^2 / d above T - 1 of ~1
      noisy          F x 0.05, var = 1e-3, raw_task_noises = 1: lambda ~ 1e-3, kappa ~ 2e-4 (N - tau and a'r - a'a / kappa cancel)
      linear_branch  raw_task_noises[0] = 25, raw_var[-1] = 22 (softplus's v > 20 branch), raw_vol = 3
      tiny_vol       raw_vol = -6: vol = 2.5e-3"""
    if name not in REGIMES:
        raise ValueError(name)
    dt = p["raw_vol"].dtype
    q = {k: v.detach().double().clone() for k, v in p.items()}
    if name in ("scalar", "clusters"):
        q["covar_factor"].zero_()
        q["raw_var"].fill_(-0.3)
        if name == "clusters":
            q["raw_var"][T // 2:] = 0.8
        q["raw_task_noises"].fill_(-2.0)
    elif name == "correlated":
        g = torch.Generator().manual_seed(977 + T)
        q["covar_factor"] = 1.0 + 0.1 * torch.randn(T, 1, generator=g, dtype=torch.float64)
        q["raw_var"].fill_(_inv_softplus(1e-2))
        q["raw_task_noises"].fill_(_inv_softplus(1e-2))
        q["raw_noise"].fill_(-12.0)
    elif name == "noisy":
        q["covar_factor"] *= 0.05
        q["raw_var"].fill_(_inv_softplus(1e-3))
        q["raw_task_noises"].fill_(1.0)
    elif name == "linear_branch":
        q["raw_task_noises"][0] = 25.0
        q["raw_var"][-1] = 22.0
        q["raw_vol"].fill_(3.0)
    elif name == "tiny_vol":
        q["raw_vol"].fill_(-6.0)
    return {k: v.to(dt) for k, v in q.items()}


def case(name, N, T, start, dtype=torch.float64, seed=None):
    """(p, x, Y) of make_case in regime ``name``; the seed depends on the shape and the start only, so the regimes of one
    shape share x and Y."""
    p, x, Y = make_case(N, T, start, seed=(100 * T + N + start) if seed is None else seed, dtype=dtype)
    return regime(name, p, T), x, Y


def as_numpy(p):
    return {k: v.detach().cpu().double().numpy() for k, v in p.items()}


# ------------------------------------------------------------------ invariants
def eig_checks(S, lam, Q):
    """The bounds of test_gpu_multitask.test_syev_small_eigenpairs on (lam, Q) against the fp64 S rebuilt on the host: the
    residual and the eigenvalues relative to |S| (LAPACK's own small eigenvalues are accurate to eps |S| only), orthogonality
    absolute, eigenvalues ascending.  None of them depends on signs or on the basis inside a tied cluster."""
    T = S.shape[0]
    nS = np.linalg.norm(S)
    assert np.isfinite(lam).all() and np.isfinite(Q).all()
    assert np.linalg.norm(S @ Q - Q * lam) <= 1e-12 * nS, np.linalg.norm(S @ Q - Q * lam) / nS
    assert np.linalg.norm(Q.T @ Q - np.eye(T)) <= 1e-12, np.linalg.norm(Q.T @ Q - np.eye(T))
    want = np.linalg.eigvalsh(S)
    assert np.abs(lam - want).max() <= 1e-12 * np.abs(want).max(), np.abs(lam - want).max() / np.abs(want).max()
    assert (np.diff(lam) >= 0).all()


def reconstruct_R(resid, lam, vol, Q, d):
    """R = Y - mu [N,T] back from the prologue's outputs: resid_j sqrt(vol lambda_j) = (R D^-1/2 Q)_j, so
    R = (resid_j sqrt(vol lambda_j))_j Q' D^1/2.  Q enters as Q Q' restricted to an eigenspace: eigenvector signs and rotations
    inside a tied cluster cancel."""
    resid, lam, Q, d = (np.asarray(t, np.float64) for t in (resid, lam, Q, d))
    Z = resid.T * np.sqrt(vol * lam)[None, :]
    return (Z @ Q.T) * np.sqrt(d)[None, :]


def residual_of(p, x, Y):
    """Y - mu [N,T] in fp64 from the definition (mu = -1/2 vol^2 x diag(K_t))."""
    pro = kref.prologue_ref(p, x, Y)
    x, Y = np.asarray(x, np.float64), np.asarray(Y, np.float64)
    return Y + 0.5 * pro["vol"] ** 2 * x[:, None] * np.diag(pro["Kt"])[None, :]


# ------------------------------------------------------------------ the fp32 references
def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _chain_step(x, sigma2, resid):
    out, alpha, info = ref.bm_step_ref(x, np.ones(sigma2.shape[0]), sigma2, resid)
    assert not info.any(), info
    return out, alpha


def _vendor_step(x, sigma2, resid):
    """out [T,8] (columns 0 and 4, all the epilogue reads) and alpha [T,N] from torch's fp32 Cholesky of M + sigma_j^2 I per
    direction: the "vendor" route of tests/test_gpu_lownoise.py."""
    x32 = torch.from_numpy(np.asarray(x, np.float64)).float()
    n = x32.shape[0]
    M = torch.minimum(x32[:, None], x32[None, :])
    T = sigma2.shape[0]
    out, alpha = np.zeros((T, 8)), np.empty((T, n))
    for j in range(T):
        r = torch.from_numpy(resid[j]).float()
        A = (M.double() + float(sigma2[j]) * torch.eye(n, dtype=torch.float64)).float()
        L = torch.linalg.cholesky(A)
        a = torch.cholesky_solve(r.unsqueeze(-1), L).squeeze(-1)
        z = torch.linalg.solve_triangular(L, r.unsqueeze(-1), upper=False).squeeze(-1).double()
        logdet = 2.0 * float(torch.log(torch.diagonal(L).double()).sum())
        out[j, 0] = -0.5 * (float(z @ z) + logdet + n * math.log(2.0 * math.pi)) / n
        out[j, 4] = float(torch.diagonal(torch.cholesky_inverse(L)).double().sum())
        alpha[j] = a.double().numpy()
    return out, alpha


def _through_fp32_interface(p, x, Y, step):
    """The restatement with the step's interface in fp32: resid and sigma2 rounded before the step, out and alpha after it;
    the prologue's state (vol, lambda, d, W) and the epilogue in fp64, as the kernels keep them."""
    pro = kref.prologue_ref(p, x, Y)
    pro["resid"], sigma2 = _f32(pro["resid"]), _f32(pro["sigma2"])
    out, alpha = step(np.asarray(x, np.float64), sigma2, pro["resid"])
    res = kref.epilogue_ref(p, x, pro, _f32(out), _f32(alpha))
    T = pro["lam"].shape[0]
    return float(res[0]), kref.unpack(res, T)


def interface_floor(p, x, Y):
    """(mll, {name: gradient}) of the restatement with resid, sigma2, out and alpha rounded to fp32 and everything else in
    fp64: no fp32 path can be expected to do better, so its distance to the oracle bounds the fp32 path's error from below."""
    return _through_fp32_interface(p, x, Y, _chain_step)


def yardstick(p, x, Y):
    """(mll, {name: gradient}) with the step replaced by torch's fp32 Cholesky per direction: what a vendor fp32 factorisation
    leaves on the same interface."""
    return _through_fp32_interface(p, x, Y, _vendor_step)


def rel_errors(mll, grads, ref_mll, ref_grads, floor_one=False):
    """{quantity: error / scale} against the oracle.  Scales: max(1, |mll|) for the MLL; for a gradient the project's fp32
    scale max |gradient|, or max(1, .) with ``floor_one`` (the fp64 gates) and wherever the oracle's gradient is EXACTLY zero
    (d / d covar_factor at F = 0: scalar, clusters)."""
    errs = {"mll": abs(mll - ref_mll) / max(1.0, abs(ref_mll))}
    for k in kref.NAMES:
        want = np.asarray(ref_grads[k], np.float64).reshape(-1)
        got = np.asarray(grads[k], np.float64).reshape(-1)
        scale = float(np.abs(want).max())
        if floor_one or scale == 0.0:
            scale = max(1.0, scale)
        errs[k] = float(np.abs(got - want).max()) / scale
    return errs


QUANTITIES = ("mll",) + kref.NAMES
F32_BOUND = {"mll": 5e-5, **{k: 2e-3 for k in kref.NAMES}}        # the project's fp32 bounds (tests/test_gpu_multitask.py)

_REFS = {}


def references(name, N, T, start, dtype):
    """Once per case: dict(p, x, Y, oracle=(mll, grads)) and, for fp32 cases, floor / yard = rel_errors of interface_floor /
    yardstick against the oracle.  The oracle and both references see the case's own (rounded) inputs in fp64."""
    key = (name, N, T, start, dtype)
    if key not in _REFS:
        p, x, Y = case(name, N, T, start, dtype)
        mll, g = oracle_mll(p, x.double(), Y.double())
        g = {k: v.numpy() for k, v in g.items()}
        out = dict(p=p, x=x, Y=Y, oracle=(mll, g))
        if dtype == torch.float32:
            pn, xn, Yn = as_numpy(p), x.double().numpy(), Y.double().numpy()
            out["floor"] = rel_errors(*interface_floor(pn, xn, Yn), mll, g)
            out["yard"] = rel_errors(*yardstick(pn, xn, Yn), mll, g)
        _REFS[key] = out
    return _REFS[key]
