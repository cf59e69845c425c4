"""The fp64 definition of volt_rollout_bordered_f32 and volt_rollout_shared_f32 (include/volt_hip.h) at the kernels' own
interface, in plain numpy: the recursion of csrc/rollout.hip's rollout_lane_kernel step for step, every operation in double.
It is the yardstick of tests/test_rollout_ref_host.py and tests/test_gpu_rollout_kernels.py; it never calls the library and
never runs on the device.  Inputs are read as the values the kernel sees (fp32 arrays cast to double; rho, tau, acc0 fp64).

The branches are the kernel's, comparison for comparison:
    pvar = kss - w's;  if !(pvar > 0): jit = jitter; at most two times jit *= 10 while !(pvar + jit > 0);
                       pvar + jit > 0 ? pvar += jit : (pvar = 0, info = -step unless info is negative already)
    d2 = U - w's;      if !(d2 > 0): (info = +step if info is still 0), d2 = max(jitter, 1e-12)
so a negative code overrides a positive one and the first negative one stays.
"""
import numpy as np

PERTURBATIONS = ("taps_shift", "kss_full_dx", "tau_prev_series", "theta_dropped", "ema_prev_stale", "ww_stale")


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def ema_tails(y, w, levels=2):
    """For y [G,n] (n >= k, the first k entries are the lead-in) the EMA and EMA(EMA) at the positions of y, in fp64:
    ema[t] = sum_j w_j y[t-k+j] (left-padded with the first value), the recursion the kernels continue.  Returns
    [y, e1, e2][:levels + 1], each [G,n]."""
    y = _f64(y)
    w = _f64(w)
    k = w.shape[0]
    out = [y]
    for _ in range(levels):
        src = out[-1]
        pad = np.concatenate([np.repeat(src[:, :1], k, axis=1), src], axis=1)
        out.append(np.stack([pad[:, t:t + k] @ w for t in range(src.shape[1])], axis=1))
    return out


class _Mean:
    """The EWMA-family mean of the appended point from the stacked histories (family_mean / the lane kernel's ring)."""

    def __init__(self, hist_y, hist_e1, hist_e2, ema_prev, mr_latent, w, S, H, k, mode, mr_theta, mean_dtype, perturb):
        self.mode, self.k, self.ft, self.perturb = mode, k, np.dtype(mean_dtype).type, perturb
        self.w = _f64(w).reshape(-1)[:k]
        G = np.asarray(hist_y).shape[0]
        self.ordered = self.ft is not np.float64

        def stack(h):
            out = np.zeros((G, S, k + H))
            out[:, :, :k] = _f64(h).reshape(G, 1, k)
            return out
        self.hy = stack(hist_y) if mode != 4 else None
        self.h1 = stack(hist_e1) if mode in (1, 2) else None
        self.h2 = stack(hist_e2) if mode == 2 else None
        self.given = _f64(hist_e1).reshape(G, 1, H) if mode == 4 else None
        if mode == 3:
            self.ema_prev = np.repeat(_f64(ema_prev).reshape(G, 1), S, axis=1)
            self.mr_latent = _f64(mr_latent).reshape(G, 1)
            self.mr_theta = self.ft(np.float32(mr_theta))

    def _dot(self, h, idx):
        win = h[:, :, idx:idx + self.k]
        if self.perturb == "taps_shift":
            win = np.roll(win, 1, axis=-1)
        if not self.ordered:
            return win @ self.w
        acc = np.zeros(win.shape[:2])                      # (the oracle's order: one tap after the other)
        for j in range(self.k):
            acc += self.w[j] * win[:, :, j]
        return acc

    def step(self, idx):
        ft = self.ft
        if self.mode == 4:
            self.ma1 = self.e2 = None
            return self.given[:, :, idx]
        ma1 = self._dot(self.hy, idx).astype(ft)
        self.ma1, self.e2 = ma1, None
        if self.mode == 0:
            m = ma1
        elif self.mode == 1:
            self.e2 = self._dot(self.h1, idx).astype(ft)
            m = ft(2) * ma1 - self.e2
        elif self.mode == 2:
            self.e2 = self._dot(self.h1, idx).astype(ft)
            m = ft(3) * ma1 - ft(3) * self.e2 + self._dot(self.h2, idx).astype(ft)
        else:
            m = ma1 - self.mr_theta * (self.ema_prev.astype(ft) - self.mr_latent.astype(ft))
        return m.astype(np.float64)

    def append(self, idx, smp):
        if self.mode == 4:
            return
        self.hy[:, :, self.k + idx] = smp
        if self.h1 is not None:
            self.h1[:, :, self.k + idx] = self.ma1
        if self.h2 is not None:
            self.h2[:, :, self.k + idx] = self.e2
        if self.mode == 3 and self.perturb != "ema_prev_stale":
            self.ema_prev = self.ma1.astype(np.float64)


def bordered_ref(rho, tau, acc0, dx, hist_y, hist_e1, hist_e2, ema_prev, mr_latent, latent, w, pred_vol, z, k, mean_mode,
                 theta, mr_theta, jitter, *, mean_dtype=np.float64, perturb=None):
    """volt_rollout_bordered_f32 in double.  rho, tau, acc0, dx, ema_prev, mr_latent, latent [G]; hist_* [G,k] (mode 4:
    hist_e1 [G,H] is the given mean); w [k]; pred_vol, z [G,S,H]; theta None = no mean reversion.
    Returns (samples [G,S,H], info [G,S] int32, trace): trace holds, per path and step [G,S,H], the quantities the branches
    test and what they did -- ``pvar`` (before the ladder), ``d2`` (before the substitution), ``rung`` (-1 no ladder, 0 / 1 / 2
    the rung that made pvar positive, 3 exhausted), ``jit`` (what was added), ``subst`` (pivot substituted), ``w`` (the entry of
    w_s the step appended, entry idx-1; 0 at step 0), ``mstar`` and ``pm`` (the mean module's value and the predictive mean).
    ``mean_dtype=np.float32`` rounds the mean module's values to fp32 where the kernel and the oracle's fp64 run both do
    (EWMA.py:37's FloatTensor); the default keeps them in double.  ``perturb``: one of PERTURBATIONS, a deliberately wrong
    variant for the negative controls."""
    assert perturb is None or perturb in PERTURBATIONS
    pv, zz = _f64(pred_vol), _f64(z)
    G, S, H = pv.shape
    rho, tau, acc0, dx = (_f64(a).reshape(G, 1) for a in (rho, tau, acc0, dx))
    if perturb == "tau_prev_series":
        tau = np.roll(tau, 1, axis=0)
    use_theta = theta is not None and perturb != "theta_dropped"
    if use_theta:
        th, lat = float(np.float32(theta)), _f64(latent).reshape(G, 1)
    jit0 = float(np.float32(jitter))
    floor = max(jit0, float(np.float32(1e-12)))
    mean = _Mean(hist_y, hist_e1, hist_e2, ema_prev, mr_latent, w, S, H, k, mean_mode, mr_theta, mean_dtype, perturb)
    hdx = (dx if perturb == "kss_full_dx" else 0.5 * dx)
    base = np.repeat(acc0 - rho, S, axis=1)
    ww = np.zeros((G, S))
    wz = np.zeros((G, S))
    u_prev = np.zeros((G, S))
    rell_prev = np.zeros((G, S))
    z_prev = np.zeros((G, S))
    prev_subst = np.zeros((G, S), dtype=bool)
    bad = np.zeros((G, S), dtype=np.int64)
    samples = np.zeros((G, S, H))
    tr = {n: np.zeros((G, S, H)) for n in ("pvar", "d2", "jit", "w", "mstar", "pm")}
    tr["rung"] = np.full((G, S, H), -1, dtype=np.int64)
    tr["subst"] = np.zeros((G, S, H), dtype=bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for idx in range(H):
            if idx >= 1:
                w_a = (u_prev - ww) * rell_prev
                tr["w"][:, :, idx] = w_a
                if perturb == "ww_stale":
                    ww = np.where(prev_subst, ww, ww + w_a * w_a)
                else:
                    ww = ww + w_a * w_a
                wz = wz + w_a * z_prev
            mstar = np.broadcast_to(mean.step(idx), (G, S))
            v2 = pv[:, :, idx] ** 2
            kss = base + hdx * v2
            pm = tau + wz + mstar
            if use_theta:
                pm = pm - th * (pm - lat)
            pvar = kss - ww
            tr["pvar"][:, :, idx], tr["mstar"][:, :, idx], tr["pm"][:, :, idx] = pvar, mstar, pm
            need = ~(pvar > 0)
            jit = np.full((G, S), jit0)
            tries = np.zeros((G, S), dtype=np.int64)
            for _ in range(2):
                more = need & ~(pvar + jit > 0)
                jit = np.where(more, jit * 10.0, jit)
                tries += more
            ok = pvar + jit > 0
            exhausted = need & ~ok
            tr["rung"][:, :, idx] = np.where(need, np.where(ok, tries, 3), -1)
            tr["jit"][:, :, idx] = np.where(need & ok, jit, 0.0)
            pvar = np.where(need, np.where(ok, pvar + jit, 0.0), pvar)
            bad = np.where(exhausted & (bad >= 0), -(idx + 1), bad)
            smp = np.sqrt(pvar) * zz[:, :, idx] + pm
            samples[:, :, idx] = smp
            base = base + dx * v2
            d2 = base - ww
            tr["d2"][:, :, idx] = d2
            subst = ~(d2 > 0)
            tr["subst"][:, :, idx] = subst
            bad = np.where(subst & (bad == 0), idx + 1, bad)
            d2 = np.where(subst, floor, d2)
            rell = 1.0 / np.sqrt(d2)
            u_prev, rell_prev, prev_subst = base, rell, subst
            z_prev = ((smp - mstar) - tau - wz) * rell
            mean.append(idx, smp)
    return samples, bad.astype(np.int32), tr


def shared_ref(hist_y, hist_e1, hist_e2, ema_prev, mr_latent, w, e, k, mean_mode, mr_theta, *, mean_dtype=np.float64,
               sample_dtype=np.float64):
    """volt_rollout_shared_f32 in double: samples[.., idx] = mean_s(idx) + e[.., idx], the mean over the path's own earlier
    values.  e [G,S,H]; the rest as in bordered_ref.  Returns samples [G,S,H].  ``sample_dtype=np.float32`` rounds every sample
    to fp32 before it enters the history -- what ANY implementation with fp32 outputs must do: the distance of that run from
    the default one is the input's own amplification of one fp32 rounding per step (the tests' conditioning check)."""
    e = _f64(e)
    G, S, H = e.shape
    mean = _Mean(hist_y, hist_e1, hist_e2, ema_prev, mr_latent, w, S, H, k, mean_mode, mr_theta, mean_dtype, None)
    samples = np.zeros((G, S, H))
    for idx in range(H):
        smp = (np.broadcast_to(mean.step(idx), (G, S)) + e[:, :, idx]).astype(sample_dtype).astype(np.float64)
        samples[:, :, idx] = smp
        mean.append(idx, smp)
    return samples


def compared_steps(info, H):
    """Mask [G,S,H] of the steps a test may compare: all of them, except after an exhausted ladder (info < 0), where only
    steps 1 .. |info| are specified -- the recursion diverges behind it (w's grows past 1e40 within six steps)."""
    info = np.asarray(info)
    last = np.where(info < 0, -info, H)
    return np.arange(H)[None, None, :] < last[:, :, None]
