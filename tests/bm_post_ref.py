"""fp64 numpy restatement of the one-sweep posterior of the Brownian-motion vol forecaster (volt_bm_post_*, csrc/bm.hip;
gp._markov_cov).  Shared by tests/test_bm_post_host.py (the restatement against dense fp64 LAPACK, with its
negative controls) and tests/test_gpu_bm_post.py (the HIP kernel and the models against the restatement).

A = v M + s I over the grid x; for a test point xi the column k = v min(x, xi) has (D k)_i = v clamp(xi - x_{i-1}, 0, delta_i);
over sorted test points the sweep forms m_h = k_h'A^-1 r, p_h = k_h'A^-1 k_h, q_h = k_h'A^-1 k_{h+1} (q_{H-1} = p_{H-1})."""
import numpy as np

import bm_chain_ref as chain


def post_forms_ref(x, vol, sigma2, resid, xs, drop_c=False):
    """What volt_bm_post_* returns: out [B,3,H] (rows m, p, q) and info [B].  x [N] or [B,N]; xs [H] ascending.
    ``drop_c``: the negative control -- the z chains of the test points without their c_i z_{i-1} term."""
    x = np.asarray(x, np.float64)
    v = np.asarray(vol, np.float64).reshape(-1)
    s = np.asarray(sigma2, np.float64).reshape(-1)
    xs = np.asarray(xs, np.float64)
    B, H = v.shape[0], xs.shape[0]
    r = np.asarray(resid, np.float64).reshape(B, -1)
    n = r.shape[1]
    out = np.full((B, 3, H), np.nan)
    info = np.zeros(B, np.int32)
    prev = np.concatenate([[0.0], xs[:-1]])
    with np.errstate(all="ignore"):
        bad = ~((xs >= prev) & np.isfinite(xs))
    if bad.any():
        info[:] = -(int(np.argmax(bad)) + 1)
        return out, info
    nxt = np.concatenate([xs[1:], xs[-1:]])
    xb = np.broadcast_to(x, (B, n))
    d = np.empty((B, n))
    c = np.empty((B, n))
    if x.ndim == 1:                                                        # the pivots: one call per grid
        d, c, _, info = chain._pivots(x, v, s)
    else:
        for k in range(B):
            dk, ck, _, ik = chain._pivots(x[k], v[k:k + 1], s[k:k + 1])
            d[k], c[k], info[k] = dk[0], ck[0], ik[0]
    delta = np.diff(xb, axis=1, prepend=0.0)
    xprev = np.concatenate([np.zeros((B, 1)), xb[:, :-1]], axis=1)
    dr = np.diff(r, axis=1, prepend=0.0)
    zr = np.zeros((B, 1))
    za, zb = np.zeros((B, H)), np.zeros((B, H))
    m, p, q = np.zeros((B, H)), np.zeros((B, H)), np.zeros((B, H))
    vv = v[:, None]
    with np.errstate(all="ignore"):
        for i in range(n):                                                 # every series and test point at once
            ci, di, dl, xp = c[:, i:i + 1], d[:, i:i + 1], delta[:, i:i + 1], xprev[:, i:i + 1]
            zr = dr[:, i:i + 1] + ci * zr
            za = vv * np.minimum(np.maximum(xs - xp, 0.0), dl) + (0.0 if drop_c else ci) * za
            zb = vv * np.minimum(np.maximum(nxt - xp, 0.0), dl) + (0.0 if drop_c else ci) * zb
            m += za * zr / di
            p += za * za / di
            q += za * zb / di
    ok = info == 0
    out[ok, 0], out[ok, 1], out[ok, 2] = m[ok], p[ok], q[ok]
    return out, info


def markov_cov_ref(diag, off, mode="logdiff"):
    """cov [H,H] of a Markov process from its diagonal and first off-diagonal (off [H], the last entry unused).
    mode "logdiff": gp._markov_cov's rule, exp(L_c - L_a) with the zeros of g counted beside L.  The negative controls:
    "cumprod" fills by ratios of cumulative products of g (0 / 0 once they underflow); "nextdiag" divides by the NEXT
    point's variance in g."""
    diag, off = np.asarray(diag, np.float64), np.asarray(off, np.float64)
    H = diag.shape[0]
    with np.errstate(all="ignore"):
        den = diag[1:] if mode == "nextdiag" else diag[:-1]
        g = np.where(den > 0, off[:-1] / np.where(den > 0, den, 1.0), 0.0)
        g = np.maximum(g, 0.0)
        cov = np.zeros((H, H))
        if mode == "cumprod":
            P = np.concatenate([[1.0], np.cumprod(g)])
            for a in range(H):
                for c in range(a, H):
                    cov[a, c] = cov[c, a] = max(diag[a], 0.0) * (P[c] / P[a])
            return cov
        zero = g <= 0
        L = np.concatenate([[0.0], np.cumsum(np.log(np.where(zero, 1.0, g)))])
        Z = np.concatenate([[0], np.cumsum(zero)])
        for a in range(H):
            for c in range(a, H):
                cov[a, c] = cov[c, a] = max(diag[a], 0.0) * np.exp(L[c] - L[a]) * (Z[c] == Z[a])
    return cov


def sweep_posterior_ref(x, v, s, y, xs, drop_c=False, mode="logdiff"):
    """The posterior of BMGP at xs [H] (any order, duplicates allowed) for ONE series by the sweep: (mean [H], cov [H,H]),
    comparable with bm_chain_ref.dense_posterior."""
    x, xs, y = (np.asarray(t, np.float64) for t in (x, xs, y))
    order = np.argsort(xs, kind="stable")
    xo = xs[order]
    out, info = post_forms_ref(x, [v], [s], (y + 0.5 * v * v * x)[None], xo, drop_c)
    assert info[0] == 0
    m, p, q = out[0]
    cov_s = markov_cov_ref(v * xo - p, v * xo - q, mode)
    mean = np.empty_like(xo)
    mean[order] = -0.5 * v * v * xo + m
    cov = np.empty_like(cov_s)
    cov[np.ix_(order, order)] = cov_s
    return mean, cov


def test_points(x, H=24, rng=None):
    """The test points of the host test (H = 24; a smaller H takes the first H kinds, a larger one adds uniform draws),
    shuffled: inside the grid, ON grid points, beyond it, xi = 0, xi = x_{N-1}, 0 < xi < x_0 (where x_0 > 0), and duplicates."""
    rng = np.random.default_rng(11) if rng is None else rng
    x = np.asarray(x, np.float64)
    n, last = x.shape[0], x[-1]
    span = last if last > 0 else 1.0 / 252
    pts = [0.0, last, last, x[n // 2], x[0], 0.5 * x[0], 0.25 * x[0]]                 # (x_0 = 0: these repeat xi = 0)
    pts += list(x[rng.integers(0, n, size=3)])                                          # on grid points
    pts += list(rng.uniform(0.0, span, size=6))                                         # inside
    pts += list(last + span * np.array([1e-9, 0.01, 0.5, 0.5, 3.0]))                    # beyond, one of them twice
    pts += [pts[11], pts[12]]                                                           # duplicates of inside points
    pts += list(rng.uniform(0.0, 1.2 * span, size=max(0, H - len(pts))))
    pts = np.array(pts[:H])
    return pts[rng.permutation(H)]


def series(x, v, s, rng):
    """One draw of y = -1/2 v^2 x + BM(v) + noise(s) on the grid: residuals of the scale the model sees."""
    x = np.asarray(x, np.float64)
    f = np.cumsum(rng.standard_normal(x.shape[0]) * np.sqrt(v * np.diff(x, prepend=0.0)))
    return -0.5 * v * v * x + f + np.sqrt(s) * rng.standard_normal(x.shape[0])
