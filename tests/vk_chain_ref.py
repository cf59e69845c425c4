"""fp64 numpy restatement of the linear-time step of the volatility-kernel data model (volt_vk_step_*, csrc/bm.hip) and the
inputs its tests share.  K_b[i,j] = V_b[min(i,j)] with V_b = CumTrapz(vol_b^2, x) is Brownian motion on the clock V_b, so per
series the step is the Brownian-motion one (tests/bm_chain_ref.py) with the grid x = V_b and vol = 1: nothing new is derived
here.  Shared by tests/test_vk_chain_host.py (restatement against dense fp64) and tests/test_gpu_vk_linear.py (the HIP kernel
against the restatement)."""
import numpy as np

import bm_chain_ref as bm

NOISES = (1.08e-4, 1e-2, 0.69)      # the likelihood's floor softplus(-inf) + 1e-4 (+ a little), a trained level, the start value
FAMILIES = ("smooth", "lognormal", "flat_zero")
DT = 1.0 / 252


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def vol_path(family, n, rng, level=0.2):
    """One vol path [n] around ``level``: a smooth random walk, i.i.d. log-normal, or a flat path with a stretch of vol = 1e-6
    (whose increments of V vanish in fp32 once V has grown: zero_increments())."""
    if family == "smooth":
        return level * np.exp(np.cumsum(rng.standard_normal(n)) * 0.02)
    if family == "lognormal":
        return level * np.exp(rng.standard_normal(n) * 0.5)
    if family == "flat_zero":
        v = np.full(n, level)
        v[n // 3:2 * n // 3] = 1e-6
        return v
    raise ValueError(family)


def int_vol(vol, dt=DT):
    """V = CumTrapz(vol^2, x) on the uniform grid x_i = i dt, rounded to fp32 once (the fp32 numbers the dense fill copies into
    K; how they were rounded does not matter to the step, which takes V as given)."""
    vol = np.asarray(vol, np.float64)
    w = np.full(vol.shape[-1], dt)
    w[0] *= 0.5
    w[-1] *= 0.5
    return f32(np.cumsum(w * vol * vol, axis=-1))


def zero_increments(V):
    return int((np.diff(np.asarray(V), axis=-1) == 0).sum())


def vk_step_ref(V, sigma2, resid):
    """What volt_vk_step_* returns with VOLT_WANT_GRAD: out [B,8], alpha [B,N], info [B], all fp64.  V [N] or [B,N]."""
    r = np.atleast_2d(np.asarray(resid, np.float64))
    B, n = r.shape
    V = np.broadcast_to(np.asarray(V, np.float64), (B, n))
    s = np.broadcast_to(np.asarray(sigma2, np.float64).reshape(-1), (B,))
    out, alpha, info = np.empty((B, 8)), np.empty((B, n)), np.empty(B, np.int32)
    for b in range(B):
        o, a, i = bm.bm_step_ref(V[b], [1.0], [s[b]], r[b][None])
        out[b], alpha[b], info[b] = o[0], a[0], i[0]
    return out, alpha, info


def dense_k(V):
    V = np.asarray(V, np.float64)
    n = V.shape[-1]
    return V[..., np.minimum.outer(np.arange(n), np.arange(n))]


def resid(B, n, rng):
    return f32(np.cumsum(rng.standard_normal((B, n)) * 0.05, axis=1) - 2.0)


def mixed_case(B, n, seed=0):
    """B series, each with its OWN grid: vol levels spread over 0.05 .. 2, the three families mixed, the noise levels cycling.
    Returns fp32-representable float64 arrays V [B,N], s2 [B], r [B,N]."""
    rng = np.random.default_rng(seed + 7 * n)
    levels = np.exp(np.linspace(np.log(0.05), np.log(2.0), B)) if B > 1 else np.array([0.2])
    levels = levels[rng.permutation(B)]
    V = np.stack([int_vol(vol_path(FAMILIES[b % 3], n, rng, levels[b])) for b in range(B)])
    s2 = f32(np.array([NOISES[b % 3] for b in range(B)]))
    return V, s2, resid(B, n, rng)
