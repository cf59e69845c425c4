"""fp64 loop restatement of the Markov GPCV's prediction away from its grid (csrc/markov_predict.hip), the dense
definition it is checked against, and the one case list the host and the GPU tests share.  numpy only.

The restatement walks the test points ONCE in descending order with an explicit state (the knot the chain stands on, the open
interval's left knot, the anchor to the right) and emits the plan's steps one after the other; ``draw_maps`` then runs the steps
on the unit vectors, which gives the draw as an explicit linear map eps -> paths, split in its chain and its bridge columns.
``variant`` switches ONE term to a wrong form (the negative controls)."""
import numpy as np

from volt_amd.models.single_task_variational_gp import markov_startup_factor

JITTER = float(np.float32(1e-3))       # the prior's level variance as the C entry takes it: a float
DT = 1.0 / 252.0
KNOT, OPEN, POINT, CLOSE = 1, 2, 3, 4
VARIANTS = ("no_cross", "free_increment", "anchor_zero", "phi_plus")
REGIMES = ("random", "startup", "weak")
FAMILIES = ("beyond", "inside", "same", "every", "crowd", "mixed")


def f32(a):
    """fp64 values that fp32 holds exactly: the device reads the same numbers."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def make_grid(N, x0):
    rng = np.random.default_rng(1000 + N)
    x = x0 + DT * np.concatenate([[0.0], np.cumsum(0.5 + rng.random(N - 1))]) if N > 1 else np.array([x0])
    x = f32(x)
    assert N == 1 or np.all(np.diff(x) > 0)
    return x


def make_params(x, v, regime, B=1, seed=0):
    """(m, rho, gamma) [B,N] and mu [B] in fp32-exact fp64."""
    N = x.shape[0]
    rng = np.random.default_rng(7 * N + 13 * seed + REGIMES.index(regime))
    m = rng.normal(-1.0, 0.5, (B, N))
    mu = rng.normal(-0.8, 0.2, B)
    if regime == "random":
        rho, gamma = rng.normal(1.0, 0.5, (B, N)), rng.normal(-0.7, 0.3, (B, N))
    else:
        h = np.full((B, N), 1e-4) if regime == "weak" else np.exp(rng.uniform(np.log(1e-4), np.log(1000.0), (B, N)))
        rho, gamma = markov_startup_factor(x, np.full(1, float(v)), JITTER, h)
    return f32(m), f32(rho), f32(gamma), f32(mu)


def make_points(x, family, H=None, seed=0):
    """The test points of ``family`` in the caller's (shuffled) order, fp32-exact.  H: how many, where the family leaves it open
    (`same` and `every` follow the grid; `mixed` has 16 or 19 of its own and is cut or repeated to H)."""
    N = x.shape[0]
    rng = np.random.default_rng(31 * N + seed + 101 * FAMILIES.index(family))
    xl = x[-1]
    n = 15 if H is None else H
    if family == "beyond":
        xs = xl + np.sort(rng.uniform(0.0, 40 * DT, n))
    elif family == "inside":
        xs = rng.uniform(x[0], x[0] + (x[-1] - x[0]), n)
    elif family == "same":
        xs = x.copy()
    elif family == "every":
        xs = x[:-1] + rng.uniform(0.1, 0.9, N - 1) * np.diff(x) if N > 1 else np.array([x[0] + DT])
    elif family == "crowd":
        i = (N - 1) // 2
        lo, hi = (x[i], x[i + 1]) if N > 1 else (x[0], x[0] + DT)
        xs = lo + rng.uniform(0.05, 0.95, n) * (hi - lo)
    else:                                                              # mixed
        k = N // 2
        xs = [0.0, x[0], x[k], x[k], xl, xl - 0.5 * DT if N > 1 else xl, xl + 0.5 * DT, xl + 0.5 * DT, xl + 3 * DT]
        if x[0] > 0:
            xs += [0.5 * x[0], 0.25 * x[0], 0.25 * x[0]]
        xs += list(rng.uniform(0.0, xl + 2 * DT, 4))
        dup = rng.uniform(x[0], xl) if N > 1 else xl + DT
        xs += [dup, dup, dup]
        xs = np.array(xs)
        if H is not None:
            xs = np.resize(xs, H)
    xs = f32(np.maximum(xs, 0.0))
    return xs[rng.permutation(xs.shape[0])]


def dense_definition(x, xs, v, mu, m, rho, gamma, j=JITTER):
    """mean, C_q = A P^-1 A', C_p = K** - A K_uu A' for ONE series, from the N x N matrices."""
    N = x.shape[0]
    Lp = np.diag(np.exp(rho))
    for i in range(N - 1):
        Lp[i + 1, i] = gamma[i] * np.exp(rho[i])
    Li = np.linalg.solve(Lp, np.eye(N))
    S = Li.T @ Li
    k = lambda a, b: v * np.minimum.outer(a, b) + j
    Kuu, Ksu, Kss = k(x, x), k(xs, x), k(xs, xs)
    A = np.linalg.solve(Kuu, Ksu.T).T
    return mu + A @ (m - mu), A @ S @ A.T, Kss - A @ Kuu @ A.T


def plan(x, xs, v, mu, m, rho, gamma, j=JITTER, variant=None):
    """The restatement for ONE series: dict(order, mean, var_q, var_p [H] over the SORTED points, steps = [(op, h, a, b, c)])."""
    assert variant is None or variant in VARIANTS
    T = np.float64
    v, mu, j = T(v), T(mu), T(j)
    N, H = x.shape[0], xs.shape[0]
    order = np.argsort(xs, kind="stable")
    xo = xs[order]
    one = T(1)
    e2 = np.exp(-2 * rho)
    s = np.zeros(N, T)
    s[N - 1] = e2[N - 1]
    for i in range(N - 2, -1, -1):
        s[i] = e2[i] + gamma[i] * gamma[i] * s[i + 1]
    sign = one if variant == "phi_plus" else -one
    xa = T(0) if variant == "anchor_zero" else -j / v

    def travel(a, b):                      # (Phi, r) of the chain from knot b down to knot a < b
        phi, r, g2 = one, T(0), one
        for l in range(a, b):
            r = r + g2 * e2[l]
            g2 = g2 * gamma[l] * gamma[l]
            phi = phi * (sign * gamma[l])
        return phi, r

    idx = np.searchsorted(x, xo, side="right") - 1
    mean, vq, vp = np.zeros(H, T), np.zeros(H, T), np.zeros(H, T)
    for h in range(H):
        i, t = idx[h], xo[h]
        if i == N - 1:
            mean[h], vq[h], vp[h] = m[i], s[i], v * (t - x[i])
            continue
        xl, ml, sl = (x[i], m[i], s[i]) if i >= 0 else (xa, mu, T(0))
        xr = x[i + 1]
        w = (t - xl) / (xr - xl)
        mean[h] = (one - w) * ml + w * m[i + 1]
        vq[h] = (one - w) ** 2 * sl + w * w * s[i + 1]
        if i >= 0 and variant != "no_cross":
            vq[h] -= 2 * w * (one - w) * gamma[i] * s[i + 1]
        vp[h] = v * (t - xl) if variant == "free_increment" else v * (t - xl) * (xr - t) / (xr - xl)
    steps = [(KNOT, 0, T(0), T(0), np.sqrt(s[N - 1]))]
    kb, h = N - 1, H - 1
    while h >= 0:
        i = idx[h]
        if i + 1 < kb:
            phi, r = travel(i + 1, kb)
            steps.append((KNOT, h, phi, T(0), np.sqrt(r)))
            kb = i + 1
        if i == N - 1:
            steps.append((OPEN, h, one, T(0), T(0)))
        elif i >= 0:
            phi, r = travel(i, i + 1)
            steps.append((OPEN, h, phi, T(0), np.sqrt(r)))
        else:
            steps.append((OPEN, h, T(0), T(0), T(0)))
        xl = x[i] if i >= 0 else xa
        ax = x[i + 1] if i < N - 1 else None
        while h >= 0 and idx[h] == i:
            t = xo[h]
            if ax is None:
                a, b, c2 = one, T(0), v * (t - xl)
            elif t >= ax:
                a, b, c2 = T(0), one, T(0)
            else:
                w = (t - xl) / (ax - xl)
                a, b = one - w, w
                c2 = v * (t - xl) if variant == "free_increment" else v * (t - xl) * (ax - t) / (ax - xl)
            last = h == 0 or idx[h - 1] != i
            steps.append((CLOSE if last else POINT, h, a, b, np.sqrt(max(c2, T(0)))))
            ax = t
            h -= 1
        kb = max(i, 0)
    return dict(order=order, mean=mean, var_q=vq, var_p=vp, steps=steps, H=H)


def draw_maps(pl):
    """(Fk, Fb) [H,E] over the SORTED points: the paths' deviations from the mean are Fk eps (chain) + Fb eps (bridge)."""
    steps, H = pl["steps"], pl["H"]
    E = len(steps)
    T = np.float64
    Fk, Fb = np.zeros((H, E), T), np.zeros((H, E), T)
    R, L, Ak, Ab = (np.zeros(E, T) for _ in range(4))
    for e, (op, h, a, b, c) in enumerate(steps):
        unit = np.zeros(E, T)
        unit[e] = c
        if op == KNOT:
            R = a * R + unit
        elif op == OPEN:
            L = a * R + unit
            Ak, Ab = R, np.zeros(E, T)
        else:
            Ak = a * L + b * Ak
            Ab = b * Ab + unit
            Fk[h], Fb[h] = Ak, Ab
            if op == CLOSE:
                R = L
    return Fk, Fb


def draw(pl, eps, part="both", exp=False):
    """The paths [S,H] in the CALLER's order for eps [S,E'] (E' >= E), fp64."""
    Fk, Fb = draw_maps(pl)
    E = Fk.shape[1]
    F = {"both": Fk + Fb, "chain": Fk, "bridge": Fb}[part]
    y = pl["mean"][None, :] + eps[:, :E].astype(np.float64) @ F.T.astype(np.float64)
    y = np.exp(y) if exp else y
    out = np.empty_like(y)
    out[:, pl["order"]] = y
    return out


def unsort(pl, a):
    out = np.empty_like(a)
    out[pl["order"]] = a
    return out


def located(x, xs):
    """idx_h = #{x_k <= xi_h} - 1 for the points as given."""
    return np.searchsorted(x, xs, side="right") - 1


def control_can_act(variant, x, xs):
    """Whether the wrong term of ``variant`` changes a number at these inputs, and the quantity it changes.
    The cross term and Phi's sign need a point strictly inside an interval of the grid (both neighbouring knots in use); the free
    increment a point strictly inside any interval, the one before x_0 included (there its right anchor is x_0); the anchor a
    point before x_0.  True means the control MUST show; for the free increment (the draw's bridges beyond the grid) and Phi's sign
    (covariances between points on different knots) False does not mean that nothing changes."""
    idx, N = located(x, xs), x.shape[0]
    inner = (idx >= 0) & (idx < N - 1)
    strictly = inner & (xs > x[np.clip(idx, 0, N - 1)])
    before = idx < 0
    return {"no_cross": (bool(strictly.any()), "var_q"), "phi_plus": (bool(strictly.any()), "chain"),
            "free_increment": (bool((strictly | before).any()), "var_p"), "anchor_zero": (bool(before.any()), "mean")}[variant]


# ---- the ONE case list: what tests/test_gpu_markov_predict.py runs on the device is what tests/test_markov_predict_host.py
# ties to the dense definition.  ``series``: the series of the batch that are compared with the restatement.
GPU_NS, GPU_BS, GPU_SS = (1, 2, 3, 63, 64, 65, 129, 399), (1, 3, 65), (1, 63, 64, 65, 130)
GPU_EDGES = (4, 5, 255, 256, 257, 2047, 2048, 2049, 2 * 4097)       # the scan's run / wave / chunk edges
GPU_HS = (1, 2, 3, 31, 32, 33, 64, 65, 130, 300)
VS = (0.05, 0.2, 0.9)
DENSE_NMAX = 2046          # the host solves the N x N systems of the dense definition up to here (seconds and 0.5 GB each beyond)


def _case(group, N, x0, v, regime, family, B, S, H=None, exp=False, parts=("both",), series=None):
    return dict(group=group, N=N, x0=x0, v=float(f32(v)), regime=regime, family=family, B=B, S=S, H=H, exp=exp, parts=parts,
                series=tuple(range(B)) if series is None else series)


def _gpu_cases():
    out = []
    for kn, N in enumerate(GPU_NS):                                    # N x B in full; families, S, x_0, v, regime rotate inside
        for kb, B in enumerate(GPU_BS):
            for f, family in enumerate(FAMILIES):
                out.append(_case(f"shape-{N}x{B}", N, (0.0, DT)[(kn + kb + f) % 2], VS[(kn + 2 * kb + f) % 3],
                                 REGIMES[(kn + kb + 2 * f) % 3], family, B, GPU_SS[(kn + kb + f) % 5], exp=f % 2 == 1,
                                 parts=("both", "chain", "bridge") if (f + kb) % 3 == 0 else ("both",),
                                 series=None if B < 65 else (0, 31, 64)))
    for N in GPU_EDGES:
        for family in ("inside", "mixed", "beyond"):
            out.append(_case(f"edge-{N}", N, (0.0, DT)[N % 2], VS[N % 3], REGIMES[N % 3], family, 2, 5, series=(1,)))
    for k, H in enumerate(GPU_HS):
        for family in ("inside", "mixed", "crowd", "beyond"):
            out.append(_case(f"points-{H}", 65, DT, 0.2, REGIMES[k % 3], family, 3, GPU_SS[k % 5], H=H, exp=k % 2 == 0))
    return out


GPU_CASES = _gpu_cases()
GPU_GROUPS = list(dict.fromkeys(c["group"] for c in GPU_CASES))


def case_inputs(c):
    """(x, xs, v, mu [B], m, rho, gamma [B,N]) of a case, fp32-exact fp64: what the device reads."""
    x = make_grid(c["N"], c["x0"])
    m, rho, gamma, mu = make_params(x, c["v"], c["regime"], B=c["B"])
    return x, make_points(x, c["family"], H=c["H"]), c["v"], mu, m, rho, gamma


def case_eps(c, E):
    """The base samples [B,S,E] of a case (fp32)."""
    return np.random.default_rng(c["N"] + 7 * E + c["S"]).standard_normal((c["B"], c["S"], E)).astype(np.float32)


def gpu_tol(N):
    """The GPU bound on the plan's fp64 outputs, of each quantity's scale."""
    return 1e-10 if N < 4096 else 1e-8


HOST_SHAPES = [(N, x0, v) for N in (1, 2, 3, 17, 64, 65, 130, 399) for x0 in (0.0, DT) for v in (0.05, 0.2, 0.9)]


def softplus(a):
    return np.logaddexp(0.0, a)


def make_task_params(T, seed=0):
    """(Lt [T,T] lower, covar_factor f [T], raw_var [T], c [T]) of the multi-task model, fp32-exact; K_t = f f' + diag softplus(raw_var)."""
    rng = np.random.default_rng(500 + T + seed)
    Lt = np.tril(rng.normal(0.0, 0.3, (T, T))) + np.diag(0.5 + rng.random(T))
    return f32(Lt), f32(rng.normal(0.0, 0.5, T)), f32(rng.normal(-1.0, 0.5, T)), f32(rng.normal(-0.8, 0.2, T))


def mt_dense_definition(x, xs, v, c, M, rho, gamma, Lt, f, raw_var, j=JITTER):
    """mean [H,T] and the (H T) x (H T) covariance (element (h, t) at h T + t) of the multi-task prediction from the full
    Kronecker matrices: prior N(1 c', K_M (x) K_t), q(U) = N(M, P^-1 (x) Lt Lt')."""
    N, T = M.shape
    Lp = np.diag(np.exp(rho))
    for i in range(N - 1):
        Lp[i + 1, i] = gamma[i] * np.exp(rho[i])
    Li = np.linalg.solve(Lp, np.eye(N))
    Kt = np.outer(f, f) + np.diag(softplus(raw_var))
    k = lambda a, b: v * np.minimum.outer(a, b) + j
    Kuu, Ksu, Kss = np.kron(k(x, x), Kt), np.kron(k(xs, x), Kt), np.kron(k(xs, xs), Kt)
    A = np.linalg.solve(Kuu, Ksu.T).T
    mu_u, mu_s = np.tile(c, N), np.tile(c, xs.shape[0])
    mean = mu_s + A @ (M.reshape(-1) - mu_u)
    C = A @ np.kron(Li.T @ Li, Lt @ Lt.T) @ A.T + Kss - A @ Kuu @ A.T
    return mean.reshape(-1, T), C


def mt_maps(x, xs, v, c, M, rho, gamma, Lt, f, raw_var, j=JITTER):
    """The composition the model makes from the single-series restatement: mean [H,T] (column t: the plan of (M[:, t], c_t)),
    var [H,T], and the draw as maps (Gk, Gb) [H T, T E] of T rows of base samples: chain parts mixed by Lt, bridge parts by
    chol(K_t).  Caller's order."""
    T = M.shape[1]
    Kt = np.outer(f, f) + np.diag(softplus(raw_var))
    pls = [plan(x, xs, v, c[t], M[:, t], rho, gamma, j=j) for t in range(T)]
    mean = np.stack([unsort(p, p["mean"]) for p in pls], -1)
    p0 = pls[0]
    var = np.outer(unsort(p0, p0["var_q"]), np.diag(Lt @ Lt.T)) + np.outer(unsort(p0, p0["var_p"]), np.diag(Kt))
    Fk, Fb = draw_maps(p0)
    inv = np.empty_like(p0["order"])
    inv[p0["order"]] = np.arange(p0["H"])
    return mean, var, np.kron(Fk[inv], Lt), np.kron(Fb[inv], np.linalg.cholesky(Kt))


def mt_draw(maps, eps):
    """Paths [S,H,T] for eps [S,T,E'] from ``mt_maps``' result."""
    mean, _, Gk, Gb = maps
    H, T = mean.shape
    E = Gk.shape[1] // T
    e = eps[:, :, :E].astype(np.float64)                               # [S,T,E]; the maps' columns run (e, t) with t fastest
    flat = e.transpose(0, 2, 1).reshape(e.shape[0], -1)
    return mean[None] + (flat @ (Gk + Gb).T).reshape(-1, H, T)
