"""The cases of the dense GPCV ELBO step (csrc/gpcv.hip: volt_gpcv_step_f32 / volt_gpcv_cv_step_f32) at its edges, floors, clamps
and unequal weights: the case list, the inputs, the fp64 oracle per case (cached) and the ONE comparison function, shared by
tests/test_gpcv_dense_cases_host.py and tests/test_gpu_gpcv_dense_edges.py.  Not a test module.

The reference is the repository's oracle: ``oracle.gpcv_oracle.elbo_terms`` (KL and the "exp" likelihood) and
``gpcv_cv_ref.ell`` (the "cv" likelihood), fp64, gradients by autograd.  Both apply clamp_min(min_var) and clamp(min=min_scale),
so autograd gives exactly the zero gradients the kernels implement.  ``restate`` below says the same step once more with
switches -- in float32 it shows that the bounds are reachable in that precision, and with ``broken`` set it makes ONE deliberate
mistake (the negative controls of the host test).

Inputs are tests/test_gpu_gpcv.py's (``_problem`` / ``_prior``): returns of volt_amd.synthetic.sde_series on the grid
arange(n)/252, the reference's start-up values perturbed, junk above the diagonal of Lq; priors "bm", "fbm", wishart * 2^-5 and
rbf_irregular of tests/spd_families.py.  Below n = 16 the start-up recipe does not exist (its running std needs 11 points): the
inputs are the leading n points of the 16-point problem.  Everything is rounded through fp32 before the oracle sees it, so both
sides read the same numbers.

The weights are w_ell = 1/n, w_kl = 0.7/(n + 3) (unequal, as tests/gpcv_markov_ref.py has them) wherever the group WEIGHTS does
not set its own.

Bounds: the project's existing ones for this step (tests/test_gpu_gpcv.py, tests/test_gpu_gpcv_cv.py), unchanged --
out columns 0..5 and 9: 5e-5 max(1, |ref|); grad_m, grad_Lq and each row of grad_abc: 2e-3 of the reference's max per series;
sum grad_mu: 2e-3 max(1, |ref|); grad_K: 5e-3 of its max.  Where a reference gradient is exactly zero the result must be exactly
zero.  (out column 7, |K^-1 Lq|_F^2, has no bound in the project for the dense step and gets none here.)"""
import collections
import contextlib
import functools
import math

import numpy as np
import torch

import gpcv_cv_ref as CV
import spd_families
from oracle import gpcv_oracle as GO
from volt_amd.synthetic import sde_series

MIN_VAR, MIN_SCALE, JITTER = GO.MIN_VARIANCE, GO.MIN_SCALE, GO.PRIOR_JITTER
SCALAR_TOL, GRAD_TOL, GK_TOL = 5e-5, 2e-3, 5e-3
SCALARS = ((0, "ell"), (1, "kl"), (2, "quad"), (3, "logdet_k"), (4, "logdet_s"), (5, "trace"), (9, "elbo"))
QUANTITIES = ("out", "grad_m", "grad_mu", "grad_Lq", "grad_K", "grad_a", "grad_b", "grad_c")
CLAMP_MARGIN = 1e-4
MIN_N_RECIPE = 16

Case = collections.namedtuple("Case", "group n B prior Kc kind weights Q want_dk")


def _case(group, n, B, prior="bm", Kc=0, kind="plain", weights="1/n,0.7/(n+3)", Q=75, want_dk=True):
    return Case(group, n, B, prior, Kc, kind, weights, Q, want_dk)


def case_id(c):
    s = f"{c.group}-{c.B}x{c.n}-{c.prior}-K{c.Kc}"
    if c.kind != "plain":
        s += "-" + c.kind
    if c.group == "WEIGHTS":
        s += "-w" + c.weights
    if c.Q != 75:
        s += f"-Q{c.Q}"
    return s


EDGE_N = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
# every n on both sides of the transpose's 32-tile, the 128 pad and the 256-column blocks of the gradient kernels; wishart at
# the two sizes whose factor has an off-diagonal tile; (33, 65): the tile/batch decode past 64 series; "cv" at a few of them
SIZES = ([_case("SIZES", n, B) for n in EDGE_N for B in (1, 3)]
         + [_case("SIZES", n, B, "wishart") for n in (129, 257) for B in (1, 3)]
         + [_case("SIZES", 33, 65)]
         + [_case("SIZES", n, B, Kc=5) for n in (1, 4, 5, 65, 129) for B in (1, 3)])
# the second pass of cv_abc_reduce_kernel (257 row blocks) and of gpcv_scalars_kernel (17 x 17 = 289 tile sums).  In the first
# the last return is an outlier of 30 scales, so that the one row of block 256 carries a share of grad_abc the bound can see
# (tests/test_gpcv_dense_cases_host.py: leaving it out fails).  Autograd through the 2049-point oracle takes 2.3 s on 16
# cores, so that case too is compared in full
LONG = [_case("LONG", 1025, 1, Kc=5), _case("LONG", 2049, 1, want_dk=False)]
KINDS = [_case("KINDS", 130, 3, prior, Kc, kind) for kind in ("floored", "clamped", "all_clamped")
         for prior in ("bm", "wishart") for Kc in (0, 5)]
WEIGHT_PAIRS = ("1,1", "1/n,0.25/n", "0,1", "1,0")
WEIGHTS = [_case("WEIGHTS", 130, 2, Kc=Kc, weights=w) for w in WEIGHT_PAIRS for Kc in (0, 5)]
QUAD = [_case("QUAD", 33, 2, Kc=Kc, Q=Q) for Q in (1, 20, 64, 65, 128, 129, 200) for Kc in (0, 5)]
KC = [_case("KC", 33, 2, Kc=Kc) for Kc in range(1, 9)]
ALL_CASES = SIZES + LONG + KINDS + WEIGHTS + QUAD + KC
SHORT_CASES = [c for c in ALL_CASES if c.group != "LONG"]
OUTLIER, FLOOR_OUTLIER = 30.0, 300.0


def weights(c):
    """(w_ell, w_kl) as the fp32 numbers the entry receives."""
    n = c.n
    we, wk = {"1/n,0.7/(n+3)": (1.0 / n, 0.7 / (n + 3)), "1,1": (1.0, 1.0), "1/n,0.25/n": (1.0 / n, 0.25 / n), "0,1": (0.0, 1.0),
              "1,0": (1.0, 0.0)}[c.weights]
    return float(np.float32(we)), float(np.float32(wk))


def floored_rows(n):
    """The designated rows of a "floored" case: the first and last row, both sides of the 128 pad, and a row per 32-tile."""
    return sorted({0, 31, 64, 127, 128, n - 1})


def r32(t):
    return t.to(torch.float32).to(torch.float64)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _problem(n, seed):
    """test_gpu_gpcv._problem for n points (x, yy, m, Lq with junk above the diagonal, the mean constant), fp64."""
    dt = torch.float64
    F, _ = sde_series(n, seed)
    x = torch.arange(n, dtype=dt) / 252
    yy = GO.scaled_returns(x, torch.tensor(F, dtype=dt))
    f, S_root, c0 = GO.init_variational(x, yy)
    g = torch.Generator().manual_seed(seed)
    m = f + 0.1 * torch.randn(n, generator=g, dtype=dt)
    Lq = (S_root / 10 + 0.01 * torch.randn(n, n, generator=g, dtype=dt)).tril()
    Lq = Lq + torch.triu(torch.randn(n, n, generator=g, dtype=dt), 1)
    return x, yy, m, Lq, c0.reshape(1)


MIN_DIAG = 0.01


def problem(n, seed):
    """_problem, cut to its leading n points below n = 16, with every |Lq_ii| at least MIN_DIAG (the sign kept).  The recipe's
    diagonal is chol(S)_ii + 0.01 N(0,1), chol(S)_ii ~ 0.03 (1e-4 in row 0): here and there it comes out next to zero.  Such an
    entry sets the maximum of grad_Lq through 1 / Lq_ii, and every bound on that gradient is relative to its maximum -- the
    off-diagonal entries of the gradient would be out of the bound's sight (the row permutation control of the host test);
    in row 0 it also puts the variance Lq_00^2 within reach of the floor, where fp32 and fp64 may disagree about the branch."""
    x, yy, m, Lq, c = _problem(max(n, MIN_N_RECIPE), seed)
    x, yy, m, Lq = x[:n], yy[:n], m[:n], Lq[:n, :n].clone()
    d = Lq.diagonal()                                                     # (a view: written through)
    small = d.abs() < MIN_DIAG
    d[small] = MIN_DIAG * (1.0 - 2.0 * (d[small] < 0).to(d.dtype))
    return x, yy, m, Lq, c


def prior(kind, x, seed):
    """test_gpu_gpcv._prior at vol = 0.2."""
    vol = torch.tensor(0.2, dtype=torch.float64)
    if kind in ("bm", "fbm"):
        return GO.bm_cov(x, vol) if kind == "bm" else GO.fbm_cov(x, vol)
    n = x.shape[0]
    if kind == "rbf":
        return torch.as_tensor(spd_families.rbf_irregular(1, n, seed=seed)[0])
    return torch.as_tensor(spd_families.wishart(1, n, seed=seed)[0]) * 2.0 ** -5


def gauss_hermite(Q):
    """(nodes, weights / sqrt(pi)), fp64 rounded through fp32."""
    x, w = GO.gauss_hermite(Q)
    return r32(x), r32(w / math.sqrt(math.pi))


def _warp_threshold(abc):
    """f* with sum_k a_k softplus(b_k f* + c_k) = min_scale (the warp is increasing in f: a, b > 0), by bisection."""
    lo, hi = torch.tensor(-60.0, dtype=torch.float64), torch.tensor(10.0, dtype=torch.float64)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if float(CV.warp(mid, *abc)) > MIN_SCALE:
            hi = mid
        else:
            lo = mid
    return float(0.5 * (lo + hi))


def variances(Lq):
    return Lq.tril().pow(2).sum(-1)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """The B series of a case: a list of dicts of fp64 tensors that are exactly representable in fp32 -- x, y, m, Lq, c (the
    mean constant, [1]), K (no jitter), abc ([3,Kc] transformed, or None) -- plus "floored" (the designated rows).  Computed
    once, never modified."""
    with few_threads(c.n):
        return _inputs(c)


def _inputs(c):
    ghx, _ = gauss_hermite(c.Q)
    series = []
    for b in range(c.B):
        seed = 2019 + b
        x, yy, m, Lq, c0 = (t.clone() for t in problem(c.n, seed))
        abc = r32(torch.stack(CV.constrain(*CV.draw_raw(c.Kc, 7000 + 31 * b + c.Kc)))) if c.Kc else None
        Lq, m, yy, c0 = r32(Lq), r32(m), r32(yy), r32(c0)
        rows = []
        scale_at = (lambda f: f.exp()) if abc is None else (lambda f: CV.warp(f, *abc))
        if c.kind == "floored":
            # A floored row has entries below 1e-3, so what the floor removes from grad_Lq, w_ell 2 (dE/dvar) Lq_ij, is beyond
            # the bound (2e-3 of a maximum that 1 / Lq_ii of the same rows sets) unless dE/dvar ~ -(y / scale)^2 is large: the
            # returns of the designated rows are outliers of 300 scales -- in every second designated row, the others keep
            # theirs, and which ones alternates with the series
            rows = floored_rows(c.n)
            var = variances(Lq)
            for k, i in enumerate(rows):                                # the row's variance becomes min_var / 4 (junk stays junk)
                Lq[i, :i + 1] *= math.sqrt(0.25 * MIN_VAR / float(var[i]))
                if (k + b) % 2 == 0:
                    yy[i] = FLOOR_OUTLIER * scale_at(m[i]) * (1.0 if yy[i] >= 0 else -1.0)
            Lq, yy = r32(Lq), r32(yy)
        if c.kind == "clamped":
            # every mean is put where the clamp's threshold lies half way between two neighbouring nodes of its row (which pair
            # moves with the row: 27 % to 75 % of a row's nodes are clamped), so the threshold cuts through the nodes and is
            # far from all of them.  The returns and the prior's mean constant move down with the means: y / scale stays of
            # order one and m - mu ordinary, so neither y^2 / min_scale^2 nor the KL swamps what the clamp does to the gradients
            thr = math.log(MIN_SCALE) if abc is None else _warp_threshold(abc)
            sd2 = torch.sqrt(2.0 * variances(Lq).clamp_min(MIN_VAR))
            c0 = c0 + (thr - m.mean())
            for i in range(c.n):
                k = 20 + (7 * i) % 36
                yy[i] *= MIN_SCALE / scale_at(m[i])
                m[i] = thr - sd2[i] * 0.5 * (ghx[k] + ghx[k + 1])
            m, yy, c0 = r32(m), r32(yy), r32(c0)
        if c.kind == "all_clamped":
            m = torch.full_like(m, -30.0)
        if c.group == "LONG" and c.Kc:
            yy[-1] = r32(OUTLIER * scale_at(m[-1]))
        series.append(dict(x=x, y=yy, m=m, Lq=Lq, c=c0, K=r32(prior(c.prior, x, seed)), abc=abc, floored=rows))
    return series


# ------------------------------------------------------------------------------------------------ the oracle and the restatement
def node_margins(s, c):
    """(share of clamped nodes, the smallest distance of a node from the clamp in the units of CLAMP_MARGIN's condition) of
    one series in the fp64 oracle: |f - log min_scale| for "exp", |s - min_scale| / min_scale for "cv"."""
    ghx, _ = gauss_hermite(c.Q)
    var = variances(s["Lq"]).clamp_min(MIN_VAR)
    locs = torch.sqrt(2.0 * var).unsqueeze(0) * ghx.unsqueeze(-1) + s["m"].unsqueeze(0)
    if s["abc"] is None:
        return float((locs <= math.log(MIN_SCALE)).double().mean()), float((locs - math.log(MIN_SCALE)).abs().min())
    sc = CV.warp(locs, *s["abc"])
    return float((sc <= MIN_SCALE).double().mean()), float((sc - MIN_SCALE).abs().min() / MIN_SCALE)


def all_clamped_ell(s, c):
    """ell of a series whose every node is clamped: -sum_i (y_i^2 / (2 min_scale^2) + log min_scale + log sqrt(2 pi)), times
    the sum of the quadrature weights (1 + 1e-8: they are the fp32 numbers the kernel reads)."""
    per = s["y"] ** 2 / (2 * MIN_SCALE ** 2) + math.log(MIN_SCALE) + 0.5 * math.log(2 * math.pi)
    return -float(per.sum() * gauss_hermite(c.Q)[1].sum())


def _result(terms, F, leaves, names, n):
    g = torch.autograd.grad(F, leaves, allow_unused=True)
    g = {k: (torch.zeros_like(leaf) if gi is None else gi).detach().double() for k, gi, leaf in zip(names, g, leaves)}
    out = {k: float(terms[k].detach()) for _, k in SCALARS if k != "elbo"}
    out["elbo"] = float(F.detach())
    res = dict(out=out, grad_m=g["m"], grad_mu=float(g["c"].sum()), grad_Lq=g["Lq"], grad_K=g["K"])
    res["grad_abc"] = g["abc"] if "abc" in g else None
    return res


def oracle_series(s, c):
    """The fp64 reference of one series: oracle.gpcv_oracle.elbo_terms (+ gpcv_cv_ref.ell), gradients of
    F = w_ell ell - w_kl KL by autograd."""
    we, wk = weights(c)
    gx, gw = GO.gauss_hermite(c.Q)
    gx, gw = r32(gx), r32(gw / math.sqrt(math.pi)) * math.sqrt(math.pi)       # the oracle divides by sqrt(pi) itself
    names = ["m", "Lq", "c", "K"] + (["abc"] if c.Kc else [])
    leaves = [s[k].clone().requires_grad_(True) for k in names]
    m, Lq, c0, K = leaves[:4]
    terms = dict(GO.elbo_terms(m, Lq, c0, K, s["y"], gx, gw))
    if c.Kc:
        abc = leaves[4]
        terms["ell"] = CV.ell(m, Lq, s["y"], abc[0], abc[1], abc[2], gx, gw)[0]
    return _result(terms, we * terms["ell"] - wk * terms["kl"], leaves, names, c.n)


@contextlib.contextmanager
def few_threads(n):
    """Up to a few hundred points torch's thread pool costs these evaluations ten times what it saves: one thread."""
    old = torch.get_num_threads()
    if n <= 512:
        torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(old)


@functools.lru_cache(maxsize=None)
def oracle(c):
    """The references of a case's series; computed once, never modified."""
    with few_threads(c.n):
        ref = [oracle_series(s, c) for s in inputs(c)]
    if not c.want_dk:                                                     # (the step is not asked for grad_K: nothing to compare)
        for r in ref:
            r["grad_K"] = None
    return ref


def restated(c, dtype=torch.float64, broken=None):
    """``restate`` of every series of a case, stacked as ``ratios`` takes it."""
    with few_threads(c.n):
        return stack([restate(s, c, dtype, broken) for s in inputs(c)])


BROKEN = ("swap", "nofloor", "clampgrad", "logf")


def restate(s, c, dtype=torch.float64, broken=None, rows=None):
    """The step of one series said once more, in ``dtype`` (inputs, quadrature table and arithmetic), with the clamps of the
    oracle.  ``broken``: "swap" -- w_ell and w_kl exchanged; "nofloor" -- the variance floor ignored; "clampgrad" -- the
    gradient flows through clamped nodes as if they were live; "logf" -- f instead of log(min_scale) in the clamped logp of
    the "exp" likelihood.  ``rows``: the likelihood of these rows only (an index tensor)."""
    if broken is not None and broken not in BROKEN:
        raise ValueError(f"broken: one of {BROKEN} (got {broken!r})")
    we, wk = weights(c)
    if broken == "swap":
        we, wk = wk, we
    names = ["m", "Lq", "c", "K"] + (["abc"] if c.Kc else [])
    leaves = [s[k].to(dtype).clone().requires_grad_(True) for k in names]
    m, Lq_raw, c0, K = leaves[:4]
    y = s["y"].to(dtype)
    gx, gw = (t.to(dtype) for t in gauss_hermite(c.Q))
    N = c.n
    Lq = Lq_raw.tril()
    var = Lq.pow(2).sum(-1)
    if broken != "nofloor":
        var = var.clamp_min(MIN_VAR)
    locs = torch.sqrt(2.0 * var).unsqueeze(0) * gx.unsqueeze(-1) + m.unsqueeze(0)                   # [Q, N]
    raw = locs.exp() if not c.Kc else CV.warp(locs, leaves[4][0], leaves[4][1], leaves[4][2])
    scale = raw.clamp(min=MIN_SCALE)
    if broken == "clampgrad":
        scale = raw + (scale - raw).detach()
    logscale = scale.log()
    if broken == "logf":
        logscale = torch.where(raw > MIN_SCALE, logscale, locs)
    logp = -(y.unsqueeze(0) ** 2) / (2 * scale ** 2) - logscale - math.log(math.sqrt(2 * math.pi))
    per_row = (logp * gw.unsqueeze(-1)).sum(0)
    ell = per_row.sum() if rows is None else per_row[rows].sum()
    Kj = K + JITTER * torch.eye(N, dtype=dtype)
    Lk = torch.linalg.cholesky(Kj)
    T = torch.linalg.solve_triangular(Lk, Lq, upper=False)
    z = torch.linalg.solve_triangular(Lk, (m - c0).unsqueeze(-1), upper=False)
    trace, quad = T.pow(2).sum(), z.pow(2).sum()
    logdet_k = 2.0 * Lk.diagonal().log().sum()
    logdet_s = Lq.diagonal().pow(2).log().sum()
    kl = 0.5 * (trace + quad - N + logdet_k - logdet_s)
    terms = dict(ell=ell, kl=kl, quad=quad, logdet_k=logdet_k, logdet_s=logdet_s, trace=trace)
    return _result(terms, we * ell - wk * kl, leaves, names, N)


# ------------------------------------------------------------------------------------------------ the comparison
def _zero_or(err, scale, tol):
    """error / bound; a reference that is exactly zero asks for exactly zero."""
    if scale == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / (tol * scale)


def ratios(got, ref):
    """error / bound per quantity, the worst over the series (<= 1 passes).  ``got``: dict of arrays with a leading batch
    dimension -- out [B,12], grad_m, grad_mu [B,n], grad_Lq, grad_K [B,n,n] (or None), grad_abc [B,3,Kc] (or None); ``ref``:
    the list ``oracle`` returns.  A quantity the reference does not have (None) is not compared; one the reference has must
    be there."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    r = dict.fromkeys(QUANTITIES, 0.0)
    worst = lambda k, v: r.__setitem__(k, max(r[k], float("inf") if math.isnan(v) else v))
    for b, want in enumerate(ref):
        out = t(got["out"])[b]
        for col, key in SCALARS:
            worst("out", abs(float(out[col]) - want["out"][key]) / (SCALAR_TOL * max(1.0, abs(want["out"][key]))))
        for k, tol in (("grad_m", GRAD_TOL), ("grad_Lq", GRAD_TOL), ("grad_K", GK_TOL)):
            if want[k] is not None:
                worst(k, _zero_or(float((t(got[k])[b] - want[k]).abs().max()), float(want[k].abs().max()), tol))
        if want["grad_mu"] is not None:
            gmu = t(got["grad_mu"])[b]
            if want["grad_mu"] == 0.0:
                worst("grad_mu", 0.0 if not gmu.any() else float("inf"))
            else:
                worst("grad_mu", abs(float(gmu.sum()) - want["grad_mu"]) / (GRAD_TOL * max(1.0, abs(want["grad_mu"]))))
        if want["grad_abc"] is not None:
            for i, k in enumerate(("grad_a", "grad_b", "grad_c")):
                w = want["grad_abc"][i]
                worst(k, _zero_or(float((t(got["grad_abc"])[b, i] - w).abs().max()), float(w.abs().max()), GRAD_TOL))
    return r


def passes(r):
    """The existing tests ask scalars <= their bound and gradients < theirs."""
    return r["out"] <= 1.0 and all(v < 1.0 for k, v in r.items() if k != "out")


def stack(results):
    """Per-series results of ``oracle`` / ``restate`` as the batched arrays ``ratios`` takes for ``got`` (grad_mu spread as
    the constant's gradient in entry 0)."""
    n = results[0]["grad_m"].shape[0]
    out = torch.zeros(len(results), 12, dtype=torch.float64)
    for b, r in enumerate(results):
        for col, key in SCALARS:
            out[b, col] = r["out"][key]
    gmu = torch.zeros(len(results), n, dtype=torch.float64)
    if results[0]["grad_mu"] is not None:
        gmu[:, 0] = torch.tensor([r["grad_mu"] for r in results])
    st = lambda k: None if results[0][k] is None else torch.stack([r[k] for r in results])
    return dict(out=out, grad_m=st("grad_m"), grad_mu=gmu, grad_Lq=st("grad_Lq"), grad_K=st("grad_K"), grad_abc=st("grad_abc"))


def fmt(r):
    return " ".join(f"{k}={v:.2e}" for k, v in r.items())
