"""The O(N^2) GPCV ELBO step for the Brownian-motion prior (csrc/gpcv_bm.hip, SingleTaskVariationalGP(prior_solver="linear")) on
the MI355X: against its fp64 restatement (tests/gpcv_bm_ref.py, validated against the dense oracle in
tests/test_gpcv_bm_host.py), side by side with the dense step, and through the model, the trainers and the stocks driver.

Tolerances are the dense step's (tests/test_gpu_gpcv.py, tests/test_gpu_gpcv_cv.py): scalars and F 5e-5 max(1, |ref|); grad_m,
grad_Lq, grad_mu and grad_abc 2e-3 of the gradient's max per series, d/dvol 2e-3 |ref| per series (one stated floor, at N = 1 on
a grid starting at 0, where that gradient is exactly zero: ratios()).  Every parity test prints its largest error RATIO (error /
tolerance) per quantity."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch

import gpcv_bm_ref as ref
from oracle import gpcv_oracle as GO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("ell", "kl", "quad", "logdet_k", "logdet_s", "tr_s", "tr_inv", "gg", "bb", "F")
VOLS = np.array([0.2, 0.05, 0.9, 0.4, 0.11, 0.6, 0.3, 0.75], np.float32).astype(np.float64)


def _gh():
    gh_x, gh_w = GO.gauss_hermite(75)
    return gh_x.numpy(), (gh_w / math.sqrt(math.pi)).numpy()


def _abc(B, Kc, seed=7000):
    import gpcv_cv_ref as CV
    abc = torch.stack([torch.stack(CV.constrain(*CV.draw_raw(Kc, seed + 31 * b + Kc))) for b in range(B)])
    return abc.to(torch.float32).double().numpy()                                            # [B,3,Kc], fp32-representable


@functools.lru_cache(maxsize=None)
def case(n, B, Kc=0, w=None):
    """Inputs (fp32-representable fp64 numpy) and the fp64 restatement's outputs for one shape; computed once, never modified.
    The grid starts at x_0 = 0 for odd n + B and at 1/252 otherwise; Lq is NaN above the diagonal."""
    x, m, mu, y, L = ref.problem(n, B, 100 + n + B, x0_zero=bool((n + B) % 2))
    vol = VOLS[:B]
    abc = _abc(B, Kc) if Kc else None
    we, wk = (1.0 / n, 1.0 / n) if w is None else w
    jit = float(np.float32(ref.JITTER))                                                      # the fp32 value the entry receives
    want = ref.step_ref(x, vol, m - mu, m, L, y, *_gh(), abc=abc, jitter=jit, w_ell=float(np.float32(we)),
                        w_kl=float(np.float32(wk)))
    return dict(x=x, vol=vol, m=m, mu=mu, y=y, L=L, abc=abc, we=we, wk=wk, n=n, B=B, Kc=Kc), want


def dev(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).to(DEV)


def run(c, ws=None, **kw):
    from volt_amd import ops
    ghx, ghw = _gh()
    ws = ops.gpcv_bm_step(dev(c["x"]), dev(c["vol"]), dev(c["m"] - c["mu"]), dev(c["m"]), dev(c["L"]), dev(c["y"]), dev(ghx),
                          dev(ghw), ws, abc=dev(c["abc"]) if c["abc"] is not None else None,
                          **{**dict(w_ell=c["we"], w_kl=c["wk"]), **kw})
    torch.cuda.synchronize()
    return ws


def dvol_of(ws, c):
    from volt_amd.variational import _dkl_dscale_grad
    return _dkl_dscale_grad(ws.out[:, 2:9].double(), dev(c["vol"]).double(), c["n"], float(np.float32(c["wk"])),
                            torch.ones(c["B"], dtype=torch.float64, device=DEV)).cpu().numpy()


def errors(ws, c, want):
    """Absolute errors per quantity: scalars [B,10]; gradients the per-series max."""
    host = lambda t: t.double().cpu().numpy()
    e = dict(out=np.abs(host(ws.out)[:, :10] - want["out"][:, :10]))
    for k in ("grad_m", "grad_mu", "grad_Lq") + (("grad_abc",) if c["Kc"] else ()):
        e[k] = np.abs(host(getattr(ws, k)) - want[k]).reshape(c["B"], -1).max(1)
    e["dvol"] = np.abs(dvol_of(ws, c) - want["dvol"])
    return e


def ratios(ws, c, want):
    """error / tolerance per quantity (<= 1 passes)."""
    e = errors(ws, c, want)
    r = {NAMES[k]: float((e["out"][:, k] / (5e-5 * np.maximum(1.0, np.abs(want["out"][:, k])))).max()) for k in range(10)}
    for k in ("grad_m", "grad_mu", "grad_Lq") + (("grad_abc",) if c["Kc"] else ()):
        r[k] = float((e[k] / (2e-3 * np.abs(want[k]).reshape(c["B"], -1).max(1))).max())
    # d/dvol per series, 2e-3 |ref_b|.  The one exception is N = 1 on a grid that starts at 0 (case (1, 8)): K = v min(0, 0) = 0
    # does not depend on vol, the gradient is exactly zero, and what is left to bound is the rounding of the fp32 scalars
    # out[2:9] it is a difference of: one rounding of each term, 2^-23 of the terms' magnitude
    tol = 2e-3 * np.abs(want["dvol"])
    if c["n"] == 1 and c["x"][0] == 0.0:
        tol = 2.0 ** -23 * want["dvol_scale"]
    r["dvol"] = float((e["dvol"] / tol).max())
    return r


def check(ws, c, want, label):
    assert ws.info.tolist() == [0] * c["B"]
    r = ratios(ws, c, want)
    print("GPCVBM", label, " ".join(f"{k}={v:.2e}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    assert float(ws.out[:, 10].double().sub(ref.JITTER).abs().max()) < 1e-9 and not ws.out[:, 11].any()
    assert not torch.triu(ws.grad_Lq, 1).any()                                               # exactly zero above the diagonal


# ------------------------------------------------------------------------------------------------ parity with the restatement
SHAPES = [(n, B) for n in (1, 2, 3, 63, 64, 65, 129, 399) for B in (1, 3, 8)] + [(1024, 2)]


@pytest.mark.parametrize("n,B", SHAPES)
def test_exp_step_matches_the_restatement(n, B):
    c, want = case(n, B)
    check(run(c), c, want, f"exp {B} x {n}")


@pytest.mark.parametrize("Kc", [1, 5, 8])
@pytest.mark.parametrize("n,B", [(65, 3), (129, 8), (399, 1)])
def test_cv_step_matches_the_restatement(n, B, Kc):
    c, want = case(n, B, Kc)
    check(run(c), c, want, f"cv K={Kc} {B} x {n}")


def test_weights_other_than_one_over_n():
    c, want = case(129, 3, 5, w=(0.75, 2.5))
    check(run(c), c, want, "cv K=5 3 x 129, w_ell 0.75 w_kl 2.5")
    c, want = case(65, 3, 0, w=(1.0, 1.0))
    check(run(c), c, want, "exp 3 x 65, w_ell 1 w_kl 1")


def test_cv_step_with_a_sizeable_share_of_clamped_nodes():
    """tests/test_gpu_gpcv_cv.py's clamped case (covariance root x 10, n = 399, B = 3, Kc = 5: 39 % of the nodes under the
    min_scale clamp) on the new path, against that test's own dense fp64 reference."""
    from test_gpu_gpcv_cv import _reference
    from volt_amd import ops
    n, B, Kc = 399, 3, 5
    series, gh_x, gh_w = _reference(n, B, "bm", Kc, root_scale=10.0)
    assert min(s["clamped"] for s in series) > 0.05, [s["clamped"] for s in series]
    f32 = lambda key: torch.stack([s[key].to(torch.float32) for s in series]).to(DEV)
    m, Lq, y, abc = f32("m"), f32("Lq"), f32("yy"), f32("abc")
    mu = torch.stack([s["c"].to(torch.float32).expand(n) for s in series]).to(DEV)
    x = (torch.arange(n, dtype=torch.float64) / 252).to(DEV)
    ws = ops.gpcv_bm_step(x, torch.full((B,), 0.2, device=DEV), m - mu, m, Lq, y, gh_x.to(DEV), (gh_w / math.sqrt(math.pi)).to(DEV),
                          abc=abc, w_ell=1.0 / n, w_kl=1.0 / n)
    torch.cuda.synchronize()
    assert ws.info.tolist() == [0] * B
    out = ws.out.double().cpu()
    worst = dict(scal=0.0, gm=0.0, gL=0.0, gmu=0.0, ga=0.0, gb=0.0, gc=0.0)
    rel = lambda a, r: float((a.double().cpu() - r).abs().max() / r.abs().max())
    for b, s in enumerate(series):
        t = s["terms"]
        for col, key in ((0, "ell"), (1, "kl"), (2, "quad"), (3, "logdet_k"), (4, "logdet_s"), (5, "trace"), (9, "elbo")):
            worst["scal"] = max(worst["scal"], abs(float(out[b, col]) - t[key]) / max(1.0, abs(t[key])))
        gm, gL, gc_, gabc, _ = s["grads"]
        worst["gm"] = max(worst["gm"], rel(ws.grad_m[b], gm))
        worst["gL"] = max(worst["gL"], rel(ws.grad_Lq[b], gL.tril()))
        worst["gmu"] = max(worst["gmu"], abs(float(ws.grad_mu[b].sum()) - float(gc_)) / max(1.0, abs(float(gc_))))
        for i, key in enumerate(("ga", "gb", "gc")):
            worst[key] = max(worst[key], rel(ws.grad_abc[b, i], gabc[i]))
    print("GPCVBM clamped %.3f" % max(s["clamped"] for s in series), " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert worst["scal"] <= 5e-5, worst
    assert max(worst[k] for k in ("gm", "gL", "gmu", "ga", "gb", "gc")) < 2e-3, worst


# ------------------------------------------------------------------------------------------------ robustness
@pytest.mark.parametrize("n,B,Kc", [(1, 1, 0), (65, 3, 5), (399, 1, 0), (129, 8, 0)])
def test_step_writes_nothing_past_its_buffers_and_repeats_bitwise(n, B, Kc):
    """Lq is NaN everywhere above the diagonal (case()); NaN sentinels behind every output and 0xFF bytes around the workspace
    survive; ten runs with the reused workspace agree bit for bit."""
    from volt_amd import _lib, ops
    c, want = case(n, B, Kc)
    assert n == 1 or np.isnan(c["L"][:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]]).all()
    ws = ops.GpcvBmWorkspace(B, n, DEV, Kc)
    nbytes = int(_lib.lib().volt_gpcv_bm_workspace_bytes(B, n, Kc))
    ws.buf.fill_(0xFF)
    guard = 64
    sizes = dict(out=(B, 12), grad_m=(B, n), grad_mu=(B, n), grad_Lq=(B, n, n))
    if Kc:
        sizes["grad_abc"] = (B, 3, Kc)
    bufs = {}
    for k, shape in sizes.items():
        bufs[k] = torch.full((int(np.prod(shape)) + guard,), float("nan"), device=DEV)
        setattr(ws, k, bufs[k][:int(np.prod(shape))].view(shape))
    ibuf = torch.full((B + guard,), -77, dtype=torch.int32, device=DEV)
    ws.info = ibuf[:B]
    got = run(c, ws)
    assert got is ws and ws.out.data_ptr() == bufs["out"].data_ptr()
    check(ws, c, want, f"sentinels {B} x {n} K={Kc}")
    first = {k: getattr(ws, k).clone() for k in list(sizes) + ["info"]}
    for _ in range(9):
        for k, shape in sizes.items():
            bufs[k][:int(np.prod(shape))].fill_(float("nan"))
        run(c, ws)
        for k, v in first.items():
            assert torch.equal(getattr(ws, k), v), k
    for k, shape in sizes.items():
        assert torch.isnan(bufs[k][int(np.prod(shape)):]).all(), k
    assert bool((ibuf[B:] == -77).all())
    off = ws.ptr - ws.buf.data_ptr()
    assert bool((ws.buf[off + nbytes:] == 0xFF).all()) and bool((ws.buf[:off] == 0xFF).all())


# ------------------------------------------------------------------------------------------------ side by side with the dense step
@pytest.mark.parametrize("B,n", [(1, 399), (8, 399), (2, 1024)])
def test_linear_step_is_at_least_as_accurate_as_the_dense_step(B, n):
    """ops.gpcv_step and ops.gpcv_bm_step on the same fp32 inputs: for each scalar and gradient the linear step's error against
    the fp64 restatement is at most the larger of the dense fp32 step's own error (margin 1: the chains are fp64) and one
    output rounding, 2^-23 |ref| (for a gradient: of its max)."""
    from volt_amd import ops
    c, want = case(n, B)
    L0 = np.tril(np.nan_to_num(c["L"]))                                                       # the dense step gets zeros above
    xt = dev(c["x"])
    K = dev(c["vol"]).reshape(B, 1, 1) * torch.minimum(xt[:, None], xt[None, :])
    ghx, ghw = _gh()
    wd = ops.gpcv_step(K, dev(c["m"] - c["mu"]), dev(c["m"]), dev(L0), dev(c["y"]), dev(ghx), dev(ghw), w_ell=c["we"], w_kl=c["wk"])
    torch.cuda.synchronize()
    assert not wd.info.any()
    wl = run(c)
    assert not wl.info.any()
    el, ed = errors(wl, c, want), errors(wd, c, want)
    bad = []
    for k in range(10):
        a, d, r = el["out"][:, k].max(), ed["out"][:, k].max(), np.abs(want["out"][:, k])
        ok = bool((el["out"][:, k] <= np.maximum(ed["out"][:, k], 2.0 ** -23 * r)).all())
        print(f"{B} x {n} {NAMES[k]:9s}: linear {a:.3e}  dense fp32 {d:.3e}  (|ref| {r.max():.3e}){'' if ok else '  <-- worse'}")
        if not ok:
            bad.append(NAMES[k])
    for k in ("grad_m", "grad_mu", "grad_Lq", "dvol"):
        r = np.abs(want[k]).reshape(B, -1).max(1) if k != "dvol" else np.abs(want[k])
        ok = bool((el[k] <= np.maximum(ed[k], 2.0 ** -23 * r)).all())
        print(f"{B} x {n} {k:9s}: linear {el[k].max():.3e}  dense fp32 {ed[k].max():.3e}  (|ref| {r.max():.3e}){'' if ok else '  <-- worse'}")
        if not ok:
            bad.append(k)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ info and errors
def test_info_reports_per_series():
    c, _ = case(65, 3)                                              # n + B even: x_0 = 1/252
    vn = c["vol"].copy()
    vn[1] = np.nan
    ws = run({**c, "vol": vn})
    assert ws.info.tolist() == [0, 1, 0]
    assert torch.isfinite(ws.out[[0, 2], :10]).all() and torch.isnan(ws.out[1, 9])
    assert torch.isfinite(ws.grad_Lq[[0, 2]]).all() and torch.isfinite(ws.grad_m[[0, 2]]).all()


def _model(x, yy, solver, param="exp", K=1, batch=None, seed=5):
    from volt_amd import gp
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import SingleTaskVariationalGP
    kw = {"batch_shape": torch.Size([batch])} if batch else {}
    torch.manual_seed(seed)
    lh = VolatilityGaussianLikelihood(param="exp") if param == "exp" else VolatilityGaussianLikelihood(K=K, param=param, **kw).to(DEV)
    model = SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=lh, use_piv_chol_init=False,
                                    mean_module=gp.ConstantMean(**kw), covar_module=BMKernel(**kw),
                                    learn_inducing_locations=False, use_whitened_var_strat=False, prior_solver=solver).to(DEV)
    n = x.shape[0]
    g = torch.Generator().manual_seed(seed)
    d = model.variational_strategy._variational_distribution
    shape = (batch,) if batch else ()
    with torch.no_grad():
        d.variational_mean.data = (math.log(0.2) + 0.3 * torch.randn(*shape, n, generator=g)).to(DEV)     # (batched: [T,N])
        L = (0.3 * torch.randn(*shape, n, n, generator=g) / math.sqrt(n)).tril(-1)
        d.chol_variational_covar.data = (L + torch.diag_embed(0.05 + 0.3 * torch.rand(*shape, n, generator=g))).to(DEV)
        model.mean_module.constant.fill_(math.log(0.2))
    return model, lh


def _elbo_and_grads(model, lh, x, yy):
    from volt_amd.variational import VariationalELBO, num_gauss_hermite_locs
    elbo = VariationalELBO(lh, model, yy.shape[-1])
    ps = list(model.parameters())
    ps += [q for q in lh.parameters() if all(q is not p for p in ps)]
    for p in ps:
        p.requires_grad_(True)
        p.grad = None
    with num_gauss_hermite_locs(75):
        val = elbo(model(x), yy)
    (val.sum() if val.ndim else val).backward()
    return val.detach(), {id(p): p.grad.clone() for p in ps if p.grad is not None}, ps


def test_zero_jitter_at_x0_zero_is_not_psd(monkeypatch):
    """jitter = 0 on a grid that starts at 0: d_0 = 0, info = 1, and VariationalELBO raises NotPSDError."""
    from volt_amd import variational
    from volt_amd.gp import NotPSDError
    c, _ = case(64, 1)                                              # n + B odd: x_0 = 0
    assert c["x"][0] == 0.0
    ws = run(c, jitter=0.0)
    assert ws.info.tolist() == [1]
    x = dev(c["x"])
    model, lh = _model(x, None, "linear")
    monkeypatch.setattr(variational, "PRIOR_JITTER", 0.0)
    with pytest.raises(NotPSDError):
        _elbo_and_grads(model, lh, x, dev(c["y"][0]))


# ------------------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize("param,K", [("exp", 1), ("cv", 5)])
def test_elbo_linear_against_dense(param, K):
    """VariationalELBO with prior_solver="linear" against "dense" on the same parameters: value and every parameter gradient
    within the step's tolerances (5e-5 max(1, |value|); 2e-3 of each gradient's max)."""
    n = 130
    x = (torch.arange(n, dtype=torch.float32) / 252).to(DEV)
    yy = dev(np.random.default_rng(4).standard_normal(n) * 0.2)
    res = {}
    for solver in ("dense", "linear"):
        model, lh = _model(x, yy, solver, param, K)
        val, grads, ps = _elbo_and_grads(model, lh, x, yy)
        res[solver] = (val, [grads.get(id(p)) for p in ps], [n_ for n_, _ in model.named_parameters()])
    vd, gd, names = res["dense"]
    vl, gl, _ = res["linear"]
    print(f"ELBO {param}: dense {float(vd):.8f} linear {float(vl):.8f}")
    assert abs(float(vd) - float(vl)) <= 5e-5 * max(1.0, abs(float(vd)))
    assert len(gd) == len(gl) and all((a is None) == (b is None) for a, b in zip(gd, gl))
    for i, (a, b) in enumerate(zip(gd, gl)):
        if a is None:
            continue
        err = float((a - b).abs().max() / a.abs().max())
        print(f"  grad {names[i] if i < len(names) else 'likelihood'}: {err:.2e}")
        assert err < 2e-3, (i, err)


def test_elbo_batched_equals_per_series():
    """A batched model's ELBO [T] equals the T separate models': value bitwise, gradients 1e-6 (of their max)."""
    n, T = 130, 3
    x = (torch.arange(n, dtype=torch.float32) / 252).to(DEV)
    yy = dev(np.random.default_rng(4).standard_normal((T, n)) * 0.2)
    mb, lb = _model(x, yy, "linear", batch=T)
    with torch.no_grad():
        mb.covar_module.raw_vol.copy_(torch.logit(torch.tensor([[0.2], [0.5], [0.1]])))
    vb, gb, pb = _elbo_and_grads(mb, lb, x, yy)
    for i in range(T):
        mi, li = _model(x, yy[i], "linear")
        with torch.no_grad():
            for (_, p), (_, q) in zip(mi.named_parameters(), mb.named_parameters()):
                p.copy_(q[i].reshape(p.shape))
        vi, gi, pi = _elbo_and_grads(mi, li, x, yy[i])
        assert torch.equal(vi, vb[i])
        for p, q in zip(pi, pb):
            a, b = gi[id(p)], gb[id(q)][i].reshape(p.shape)
            assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), float((a - b).abs().max() / b.abs().max())


def _prices(n, seed):
    from volt_amd.synthetic import sde_series
    return torch.tensor(sde_series(n, seed)[0])


@functools.lru_cache(maxsize=None)
def _fit_reference(n, T, iters=40):
    """Start-up values from the HIP path (as test_learn_gpcv_tracks_oracle takes them) and the fp64 oracle's 40 Adam iterations
    from them, per series."""
    from volt_amd.train_utils import FitGPCV
    F = torch.stack([_prices(n, 2021 + i) for i in range(T)])
    x = torch.arange(n, dtype=torch.float32) / 252
    eps = torch.randn(10, n, generator=torch.Generator().manual_seed(7))
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(T):
            m0, _, _ = FitGPCV(x.to(DEV), F[i].to(DEV), train_iters=0)
            d0 = m0.variational_strategy._variational_distribution
            init = (d0.variational_mean.detach().cpu(), d0.chol_variational_covar.detach().cpu(),
                    m0.mean_module.constant.detach().cpu().reshape(()))
            rec = []
            readout, ps = GO.learn_gpcv(x, F[i], train_iters=iters, eps=eps.double(), dtype=torch.float64, record=rec, init=init)
            out.append((rec, ps, readout))
    return x, F, eps, out


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("n,T", [(399, 1), (130, 3)])
def test_fit_gpcv_linear_tracks_oracle(n, T, graph):
    """FitGPCV(solver="linear") for 40 Adam iterations against oracle.gpcv_oracle.learn_gpcv in fp64, with the bounds of
    test_learn_gpcv_tracks_oracle: losses 5e-4 (the first 1e-4), variational mean, raw_vol and the constant 5e-3, readout 3e-2.
    A captured fit returns its last loss only."""
    from volt_amd.train_utils import FitGPCV
    iters = 40
    x, F, eps, want = _fit_reference(n, T)
    prices = F[0] if T == 1 else F
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model, lh, losses = FitGPCV(x.to(DEV), prices.to(DEV), train_iters=iters, solver="linear", graph=graph)
    assert model.prior_solver == "linear"
    got = torch.stack(losses).cpu().double().reshape(len(losses), -1)     # eager: [iters, T];  captured: the last summed loss
    d = model.variational_strategy._variational_distribution
    for i in range(T):
        rec, ps, readout = want[i]
        w = torch.tensor(rec, dtype=torch.float64)
        if not graph:
            assert float(((got[:, i] - w).abs() / w.abs().clamp_min(1.0)).max()) < 5e-4
            assert abs(float(got[0, i] - w[0])) < 1e-4 * abs(float(w[0]))
        vm = d.variational_mean.detach().cpu().double().reshape(T, n)[i]
        assert float((vm - ps[0]).abs().max()) < 5e-3
        assert abs(float(model.covar_module.raw_vol.detach().reshape(-1)[i]) - float(ps[3])) < 5e-3
        assert abs(float(model.mean_module.constant.detach().reshape(-1)[i]) - float(ps[2])) < 5e-3
    if graph:
        last = sum(want[i][0][-1] for i in range(T))
        assert got.numel() == 1 and abs(float(got) - last) < 5e-4 * max(1.0, abs(last))
    if T == 1:
        f = model(x.to(DEV)).rsample(base_samples=eps.to(DEV))
        vol = lh(f).scale.mean(0).cpu().double()
        assert float((vol - want[0][2]).abs().max() / want[0][2].abs().max()) < 3e-2


def test_learn_gpcv_linear_against_dense():
    """LearnGPCV(solver="linear") against LearnGPCV() with the same normal draws: 2e-3 of the max."""
    from volt_amd.train_utils import LearnGPCV
    n, iters = 200, 15
    x = (torch.arange(n, dtype=torch.float32) / 252).to(DEV)
    F = _prices(n, 2019).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(3)
        vd = LearnGPCV(x, F, train_iters=iters)
        torch.manual_seed(3)
        vl = LearnGPCV(x, F, train_iters=iters, solver="linear")
    assert vd.shape == vl.shape == (n,)
    err = float((vd - vl).abs().max() / vd.abs().max())
    print(f"LearnGPCV linear vs dense: {err:.2e}")
    assert err < 2e-3


# ------------------------------------------------------------------------------------------------ driver
def test_stocks_driver_with_the_linear_gpcv_solver_writes_reference_layout(tmp_path):
    from volt_amd.forecast import GenerateStockPredictionsBatch
    from volt_amd.synthetic import sde_batch
    B, T, ntrain, H, S = 3, 70, 64, 4, 5
    _, F, _ = sde_batch(B, T - 1, seed=77)
    closes = torch.as_tensor(np.asarray(F)).to(DEV)
    g = torch.Generator(device="cuda").manual_seed(1)
    out = GenerateStockPredictionsBatch(["AAA", "BBB", "CCC"], closes, forecast_horizon=H, train_iters=3, nsample=S,
                                        ntrain=ntrain, mean="ewma", save=True, k=10, ntimes=2, vol_iters=2,
                                        par_dir=str(tmp_path), generator=g, gpcv_solver="linear")
    assert tuple(out.shape) == (B, S, H) and torch.isfinite(out).all()
    files = sorted(p.name for p in (tmp_path / "BBB").iterdir())
    assert len(files) == 2 and all(f.startswith("volt_ewma10_") and f.endswith(".pt") for f in files)
    saved = torch.load(tmp_path / "CCC" / files[-1])
    assert tuple(saved.shape) == (S, H) and torch.equal(saved, out[2])
