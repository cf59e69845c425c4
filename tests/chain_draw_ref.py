"""fp64 restatement (numpy, no GPU) of the chain draws of csrc/chain_draw.hip: the joint draw
mean + chol(C + j I) z from a covariance with C_ii = c_i and C_{i+1,k} = g_i C_{i,k} (k <= i) as a two-number recursion per path,

    e_i = c_i - m_i,  d_i = sqrt(e_i + j),  y_i = mean_i + s_i + d_i z_i,
    m_{i+1} = g_i^2 (m_i + (e_i / d_i)^2),  s_{i+1} = g_i (s_i + (e_i / d_i) z_i),      m_0 = s_0 = 0,

for the Markov posterior of the vol forecaster (c = diag, g = off / diag) and for the predictive block W[min(s,t)] of the
volatility-kernel data model (c = W, g = 1).  Validated against numpy's dense Cholesky in tests/test_chain_draw_host.py; the
keyword switches are that file's negative controls, never used by a GPU test."""
import numpy as np


def chain_draw_ref(c, g, jitter, mean, z, drop_g_from_m=False, d_for_r=False):
    """c, g, mean [H] (g[H-1] is not used); z [..., H].  Returns (y like z, info): info = i + 1 at the first step whose
    e_i + j is not a positive finite number, and y is then all NaN."""
    c, g, mean, z = (np.asarray(a, dtype=np.float64) for a in (c, g, mean, z))
    H = c.shape[0]
    y = np.empty_like(z)
    m = 0.0
    s = np.zeros(z.shape[:-1])
    for i in range(H):
        e = c[i] - m
        t = e + jitter
        if not (t > 0 and np.isfinite(t)):
            return np.full_like(z, np.nan), i + 1
        d = np.sqrt(t)
        r = d if d_for_r else e / d
        y[..., i] = mean[i] + s + d * z[..., i]
        if i + 1 < H:
            m = (1.0 if drop_g_from_m else g[i] ** 2) * (m + r * r)
            s = g[i] * (s + r * z[..., i])
    return y, 0


def chain_root_ref(c, g, jitter, **kw):
    """The lower-triangular R with y = mean + R z: the chain applied to the columns of I."""
    H = len(c)
    y, info = chain_draw_ref(c, g, jitter, np.zeros(H), np.eye(H), **kw)
    assert info == 0
    return y.T


def markov_cg(diag, off):
    """(c, g) of the matrix gp._markov_cov(diag, off) builds: c = max(diag, 0); g_i = max(off_i / diag_i, 0), 0 where
    diag_i <= 0; the last entry of off is not read."""
    diag, off = np.asarray(diag, dtype=np.float64), np.asarray(off, dtype=np.float64)
    g = np.zeros_like(diag)
    pos = diag > 0
    pos[-1] = False
    g[pos] = np.maximum(off[pos] / diag[pos], 0.0)
    return np.maximum(diag, 0.0), g


def markov_draw_ref(mean, diag, off, z, jitter, exp=False, **kw):
    """ops.markov_draw for ONE series: mean, diag, off [H]; z [S,H]."""
    c, g = markov_cg(diag, off)
    y, info = chain_draw_ref(c, g, jitter, mean, z, **kw)
    return (np.exp(y) if exp else y), info


def cumtrapz_ref(y, dx, square=True, halve_last=True):
    """CumTrapz (voltron/kernels/VolKernel.py:4-10) over one uniform step: weights dx / 2 on the first and the last point,
    dx between, cumulative sum."""
    y = np.asarray(y, dtype=np.float64)
    v = y * y if square else y
    w = np.full(y.shape[-1], dx, dtype=np.float64)
    w[0] = 0.5 * dx
    if halve_last:
        w[-1] = 0.5 * dx
    return np.cumsum(w * v, axis=-1)


def vk_W_ref(pred_vol, vol_last, vlr, dx, halve_last=True):
    """W [.., H] of forecast._standard_mean_prediction_linear: (V_te - V_last) + (V_last - rho) with V_te - V_last the CumTrapz
    of [vol_last, pred_vol] less its first entry."""
    pred_vol = np.asarray(pred_vol, dtype=np.float64)
    head = np.broadcast_to(np.asarray(vol_last, dtype=np.float64), pred_vol.shape[:-1])[..., None]
    tail = cumtrapz_ref(np.concatenate([head, pred_vol], -1), dx, True, halve_last)
    return (tail[..., 1:] - tail[..., :1]) + vlr


def vk_draw_ref(pred_vol, vol_last, vlr, dx, mean, z, jitter, reps=1, halve_last=True, d_for_r=False):
    """ops.vk_draw for ONE series: pred_vol [S,H]; mean [H]; z [S*reps,H].  Returns (y like z, info [S]); the recursion of
    `chain_draw_ref` with g = 1, all paths at once, a failed path NaN."""
    pred_vol, z, mean = (np.asarray(a, dtype=np.float64) for a in (pred_vol, z, mean))
    S, H = pred_vol.shape
    W = np.repeat(vk_W_ref(pred_vol, vol_last, vlr, dx, halve_last), reps, axis=0)
    y = np.empty_like(z)
    m, s, bad = np.zeros(S * reps), np.zeros(S * reps), np.zeros(S * reps, dtype=np.int32)
    with np.errstate(all="ignore"):
        for i in range(H):
            e = W[:, i] - m
            t = e + jitter
            bad = np.where((bad == 0) & ~((t > 0) & np.isfinite(t)), i + 1, bad)
            d = np.sqrt(t)
            r = d if d_for_r else e / d
            y[:, i] = mean[i] + s + d * z[:, i]
            m, s = m + r * r, s + r * z[:, i]
    y[bad != 0] = np.nan
    return y, bad[::reps]


def chain_pivots_ref(c, g, jitter):
    """e_i + j of every step up to and including the first failed one."""
    m, out = 0.0, []
    for i in range(len(c)):
        e = c[i] - m
        t = e + jitter
        out.append(t)
        if not (t > 0 and np.isfinite(t)):
            break
        m = g[i] ** 2 * (m + e * e / t)
    return np.array(out)


def min_cov(W):
    """C[s,t] = W[min(s,t)]."""
    idx = np.arange(len(W))
    return np.asarray(W, dtype=np.float64)[np.minimum(idx[:, None], idx[None, :])]


def bm_posterior_diag_off(n, H, rng, v=0.6, s=0.05):
    """The sorted, distinct test points, the mean and the (diag, off) of a BM + noise posterior on a uniform grid of n points
    (dense fp64 linear algebra): points inside (the first one always, from H = 2 on), on and beyond the grid."""
    x = (1 + np.arange(n)) / 252.0
    k_in = max(1, H // 3) if H >= 2 else 0
    k_on = min(H // 3, n // 2)
    pts = np.concatenate([rng.uniform(x[0], x[-1], k_in), rng.choice(x, k_on, replace=False),
                          x[-1] + (1 + np.arange(H - k_in - k_on)) / 252.0])
    xs = np.sort(pts)
    y = -0.5 * v * v * x + np.sqrt(v) * np.cumsum(rng.standard_normal(n)) / np.sqrt(252.0) + np.sqrt(s) * rng.standard_normal(n)
    K = v * np.minimum(x[:, None], x[None, :]) + s * np.eye(n)
    Ks = v * np.minimum(x[:, None], xs[None, :])
    sol = np.linalg.solve(K, Ks)
    cov = v * np.minimum(xs[:, None], xs[None, :]) - Ks.T @ sol
    cov = 0.5 * (cov + cov.T)
    mean = -0.5 * v * v * xs + sol.T @ (y + 0.5 * v * v * x)
    diag = np.diagonal(cov).copy()
    off = np.concatenate([np.diagonal(cov, 1), [0.0]])
    return xs, mean, diag, off


def markov_case(G, S, H, seed=0, n=50):
    """The inputs of the Markov kernel's tests: G posteriors (vol and noise differ per series) and z [G,S,H]."""
    rng = np.random.default_rng(seed + 1000 * G + 10 * S + H)
    mean, diag, off = np.empty((G, H)), np.empty((G, H)), np.empty((G, H))
    for g in range(G):
        _, mean[g], diag[g], off[g] = bm_posterior_diag_off(n, H, rng, v=rng.uniform(0.2, 1.0), s=rng.uniform(0.01, 0.2))
    return mean, diag, off, rng.standard_normal((G, S, H))


def vk_case(G, S, H, reps=1, seed=0):
    """The inputs of the vk kernel's tests: pred_vol [G,S,H] around 0.2 (annualised), a daily step, V_last - rho of the size a
    train block of a few hundred days leaves, a mean of log-price size, z [G,S*reps,H]."""
    rng = np.random.default_rng(seed + 1000 * G + 10 * S + H + 7 * reps)
    pred_vol = 0.2 * np.exp(0.3 * rng.standard_normal((G, S, H)))
    vol_last = 0.2 * np.exp(0.3 * rng.standard_normal(G))
    vlr = rng.uniform(1e-5, 3e-4, G)
    dx = np.full(G, 1.0 / 252.0)
    mean = 4.0 + 0.01 * rng.standard_normal((G, H))
    return pred_vol, vol_last, vlr, dx, mean, rng.standard_normal((G, S * reps, H))
