"""fp64 numpy restatement of the linear-time Brownian-motion recurrences (csrc/bm.hip, include/volt_hip.h) and the dense
definitions they replace.  Shared by tests/test_bm_chain_host.py (restatement against dense LAPACK) and
tests/test_gpu_bm_linear.py (the HIP kernels against the restatement).

K = v M, M = min(x_i, x_k); A = v M + s I = D^-1 T D^-T with D the first-difference operator and
T = v diag(delta) + s D D' tridiagonal (delta_0 = x_0, delta_i = x_i - x_{i-1})."""
import numpy as np


def grids(n, rng=None):
    """The four grids of the tests: uniform / irregular spacing, x_0 = 0 / x_0 = 1/252."""
    rng = np.random.default_rng(5) if rng is None else rng
    dt = 1.0 / 252
    out = {}
    for name, x0 in (("zero", 0.0), ("dt", dt)):
        out["uniform_" + name] = x0 + dt * np.arange(n)
        steps = dt * rng.uniform(0.25, 4.0, size=n)
        steps[0] = x0
        out["irregular_" + name] = np.cumsum(steps)
    return out


def _pivots(x, vol, sigma2):
    """d [B,N], c [B,N] (c_0 = 0) and info [B] of T = L diag(d) L'."""
    x = np.asarray(x, np.float64)
    v = np.asarray(vol, np.float64).reshape(-1)
    s = np.asarray(sigma2, np.float64).reshape(-1)
    n, B = x.shape[0], v.shape[0]
    delta = np.diff(x, prepend=0.0)
    d = np.empty((B, n))
    c = np.zeros((B, n))
    info = np.zeros(B, np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            if i == 0:
                d[:, 0] = v * delta[0] + s
            else:
                c[:, i] = s / d[:, i - 1]
                d[:, i] = v * delta[i] + 2.0 * s - s * c[:, i]
            bad = ~((d[:, i] > 0) & np.isfinite(d[:, i]))
            info = np.where((info == 0) & bad, i + 1, info).astype(np.int32)
    return d, c, s, info


def bm_step_ref(x, vol, sigma2, resid):
    """What volt_bm_step_* returns with VOLT_WANT_GRAD: out [B,8], alpha [B,N], info [B], all fp64."""
    d, c, s, info = _pivots(x, vol, sigma2)
    B, n = d.shape
    r = np.asarray(resid, np.float64).reshape(B, n)
    with np.errstate(all="ignore"):
        u = np.diff(r, axis=1, prepend=0.0)
        z = np.empty((B, n))
        z[:, 0] = u[:, 0]
        for i in range(1, n):
            z[:, i] = u[:, i] + c[:, i] * z[:, i - 1]
        logdet = np.log(d).sum(1)
        quad = (z * z / d).sum(1)
        e = s[:, None] / d
        w = np.empty((B, n))
        g = np.empty((B, n))                       # G_ii
        go = np.zeros((B, n))                      # G_{i,i+1}
        w[:, -1] = z[:, -1] / d[:, -1]
        g[:, -1] = 1.0 / d[:, -1]
        for i in range(n - 2, -1, -1):
            w[:, i] = z[:, i] / d[:, i] + e[:, i] * w[:, i + 1]
            go[:, i] = e[:, i] * g[:, i + 1]
            g[:, i] = 1.0 / d[:, i] + e[:, i] ** 2 * g[:, i + 1]
        alpha = w.copy()
        alpha[:, :-1] -= w[:, 1:]
        mult = np.full(n, 2.0)
        mult[0] = 1.0
        tr = (mult * g).sum(1) - 2.0 * go.sum(1)
        aa = (alpha * alpha).sum(1)
        out = np.zeros((B, 8))
        out[:, 0] = -0.5 * (quad + logdet + n * np.log(2 * np.pi)) / n
        out[:, 1] = 0.5 * (aa - tr) / n
        out[:, 2], out[:, 3], out[:, 4], out[:, 5], out[:, 6] = quad, logdet, tr, aa, s
        out[:, 7] = np.asarray(vol, np.float64).reshape(-1)
        bad = info != 0
        out[bad, 0] = np.nan
        out[bad, 3] = np.nan
    return out, alpha, info


def bm_solve_ref(x, vol, sigma2, R):
    """X [B,N,H] = A_b^-1 R_b by the same two sweeps."""
    d, c, s, info = _pivots(x, vol, sigma2)
    B, n = d.shape
    R = np.asarray(R, np.float64).reshape(B, n, -1)
    u = np.diff(R, axis=1, prepend=0.0)
    z = np.empty_like(R)
    z[:, 0] = u[:, 0]
    for i in range(1, n):
        z[:, i] = u[:, i] + c[:, i, None] * z[:, i - 1]
    w = np.empty_like(R)
    w[:, -1] = z[:, -1] / d[:, -1, None]
    for i in range(n - 2, -1, -1):
        w[:, i] = z[:, i] / d[:, i, None] + (s / d[:, i])[:, None] * w[:, i + 1]
    X = w.copy()
    X[:, :-1] -= w[:, 1:]
    return X, info


def dvol_ref(out, vol, n):
    """d mll / d vol (K = vol M with the residual held fixed) from the step's scalars: the closed form of
    gp._ExactMLL.backward, a'Ma = (r'a - s a'a) / v and tr(A^-1 M) = (N - s tr A^-1) / v."""
    quad, tr, aa, s = out[:, 2], out[:, 4], out[:, 5], out[:, 6]
    return 0.5 * ((quad - s * aa) - (n - s * tr)) / (n * np.asarray(vol, np.float64).reshape(-1))


# ------------------------------------------------------------------------------------------------ the dense definitions
def dense_a(x, v, s):
    x = np.asarray(x, np.float64)
    return v * np.minimum(x[:, None], x[None, :]) + s * np.eye(x.shape[0])


def dense_step(x, vol, sigma2, resid):
    """The same eight scalars and alpha from dense fp64 LAPACK (Cholesky for logdet and the solve, inv for the trace)."""
    v = np.asarray(vol, np.float64).reshape(-1)
    s = np.asarray(sigma2, np.float64).reshape(-1)
    B, n = v.shape[0], len(x)
    r = np.asarray(resid, np.float64).reshape(B, n)
    out = np.zeros((B, 8))
    alpha = np.empty((B, n))
    for b in range(B):
        A = dense_a(x, v[b], s[b])
        L = np.linalg.cholesky(A)
        a = np.linalg.solve(L.T, np.linalg.solve(L, r[b]))
        quad, logdet = r[b] @ a, 2.0 * np.log(np.diag(L)).sum()
        tr, aa = np.trace(np.linalg.inv(A)), a @ a
        out[b, :7] = (-0.5 * (quad + logdet + n * np.log(2 * np.pi)) / n, 0.5 * (aa - tr) / n, quad, logdet, tr, aa, s[b])
        alpha[b] = a
    return out, alpha


def dense_posterior(x, v, s, y, xs):
    """Exact-GP posterior of BMGP at xs [H] for ONE series in fp64: mean -1/2 v^2 x, K = v min."""
    x, xs, y = (np.asarray(t, np.float64) for t in (x, xs, y))
    A = dense_a(x, v, s)
    Kst = v * np.minimum(xs[:, None], x[None, :])
    Kss = v * np.minimum(xs[:, None], xs[None, :])
    sol = np.linalg.solve(A, np.concatenate([(y + 0.5 * v * v * x)[:, None], Kst.T], axis=1))
    return -0.5 * v * v * xs + Kst @ sol[:, 0], Kss - Kst @ sol[:, 1:]


def out_scales(out, n):
    """The scale each of out[:, 0..5] is judged against: the magnitude of the terms it is a sum or a difference of
    (mll = -(quad + logdet + N log 2pi) / 2N and d mll / d s = (a'a - tr) / 2N cancel; the other four are plain sums)."""
    quad, logdet, tr, aa = (np.abs(out[:, k]) for k in (2, 3, 4, 5))
    return np.stack([0.5 * (quad + logdet + n * np.log(2 * np.pi)) / n, 0.5 * (aa + tr) / n, quad,
                     np.maximum(logdet, 1.0), tr, aa], axis=1)
