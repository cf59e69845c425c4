"""CPU checks of the multi-task GPCV step for the Markov variational family: the loop restatement
tests/mt_gpcv_markov_ref.py against the structured and dense oracles, the single-task restatement at T = 1, its negative
controls and its fp32 evaluation against the GPU tests' bounds, the conditions that keep the floored / clamped GPU cases from
being vacuous, the O(N T) start-up values, and the interface.  No device is needed."""
import inspect
import math
import os
import re
import subprocess
import sys
import tracemalloc

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gpcv_markov_ref as MR  # noqa: E402
import mt_gpcv_cv_ref as MC  # noqa: E402
import mt_gpcv_markov_ref as MM  # noqa: E402
import mt_gpcv_ref as R  # noqa: E402

J = MM.J
ORACLE_N, ORACLE_T, ORACLE_V = (1, 2, 3, 17, 64, 65, 129), (1, 2, 3, 16, 17, 64), (0.05, 0.2, 0.9)


def _oracle(p, w_ell, w_kl, dense=False):
    """F, its pieces and autograd gradients from mt_gpcv_ref.struct (the "cv" likelihood: mt_gpcv_cv_ref.ell_abc in the
    place of its likelihood term) through the DENSE Lx = chol(P^-1) and K = K_M - j I -- struct's own + j I then yields K_M.
    ``dense``: F, ell, KL of mt_gpcv_ref.dense (the NT x NT definition) besides."""
    dt = torch.float64
    t = lambda a: torch.tensor(np.asarray(a), dtype=dt, requires_grad=True)
    x = torch.tensor(p["x"], dtype=dt)
    M, rho, gam, Lt, c, f, rv, v = (t(p[k]) for k in ("M", "rho", "gam", "Lt", "c", "f", "raw_var", "v"))
    n, T = M.shape
    d = rho.exp()
    Lp = torch.diag_embed(d)
    if n > 1:
        Lp = Lp + torch.diag_embed(gam[:-1] * d[:-1], offset=-1)
    S = torch.linalg.inv(Lp @ Lp.mT)
    Lx = torch.linalg.cholesky(0.5 * (S + S.mT))
    K = v * torch.minimum(x[:, None], x[None, :]) + J - J * torch.eye(n, dtype=dt)
    q = dict(m=M, Lx=Lx, Lt=Lt, c=c, F=f.reshape(T, 1), raw_var=rv, raw_vol=torch.zeros(1, dtype=dt))
    y = torch.tensor(p["y"], dtype=dt)
    terms = dict(R.struct(q, x, y, K=K, w_ell=w_ell, w_kl=w_kl))
    leaves = [M, c, rho, gam, Lt, f, rv, v]
    if p["abc"] is not None:
        abc = [t(a) for a in p["abc"]]
        terms["ell"] = MC.ell_abc(q, y, abc)[0]
        terms["F"] = w_ell * terms["ell"] - w_kl * terms["kl"]
        leaves += abc
    grads = torch.autograd.grad(terms["F"], leaves, allow_unused=True)
    grads = [torch.zeros_like(leaf) if g is None else g for g, leaf in zip(grads, leaves)]     # (N = 1: gamma is unused)
    o = {k: float(terms[s].detach()) for k, s in (("ell", "ell"), ("kl", "kl"), ("quad", "q"), ("logdet_km", "ld_k"),
                                                   ("logdet_kt", "ld_kt"), ("logdet_sx", "ld_sx"), ("logdet_st", "ld_st"),
                                                   ("tau_x", "tau_x"), ("tau_t", "tau_t"), ("F", "F"))}
    o.update(dFdv=float(grads[7]), s=S.diagonal().detach().numpy(), grad_M=grads[0].numpy(), grad_c=grads[1].numpy(),
             grad_rho=grads[2].numpy(), grad_gamma=grads[3].numpy(), grad_Lt=grads[4].numpy(), grad_f=grads[5].numpy(),
             grad_raw_var=grads[6].numpy())
    if p["abc"] is not None:
        o["grad_abc"] = np.stack([g.numpy() for g in grads[8:]], 1)                            # [T,3,K]
    if dense:
        with torch.no_grad():
            dd = R.dense({k: a.detach() for k, a in q.items()}, x, y, K=K.detach(), w_ell=w_ell, w_kl=w_kl)
        o["dense"] = {"kl": float(dd["kl"]), "ell": float(dd["ell"]), "F": float(dd["F"])}
    return o


def _deviations(o, ref, n):
    """Largest deviation relative to each quantity's scale: max(1, |ref|) for a scalar, the largest entry for a gradient."""
    devs = {k: abs(o[k] - ref[k]) / max(1.0, abs(ref[k])) for k in MM.SCALARS}
    rel = lambda a, b: float(np.abs(np.asarray(a) - b).max() / max(np.abs(b).max(), 1e-300))
    devs["s"] = rel(o["s"], ref["s"])
    for k in MM.GRADS + (("grad_abc",) if ref.get("grad_abc") is not None else ()):
        if k == "grad_gamma":
            if n > 1:
                devs[k] = rel(o[k][:-1], ref[k][:-1])
            continue
        devs[k] = rel(o[k], ref[k])
    return devs


@pytest.mark.parametrize("like", ["exp", "cv"])
def test_restatement_matches_the_oracles(like):
    """Every scalar and every gradient of the restatement within 1e-10 of the quantity's scale of mt_gpcv_ref.struct's
    autograd ("cv": mt_gpcv_cv_ref's likelihood term), and of mt_gpcv_ref.dense where N T <= 600."""
    worst = ("", 0.0)
    for iN, n in enumerate(ORACLE_N):
        for iT, T in enumerate(ORACLE_T):
            for x0_zero in (False, True):
                v = ORACLE_V[(iN + iT + x0_zero) % 3]
                if like == "cv" and n * T > 2200 and x0_zero:
                    continue                                               # (the largest shapes once per likelihood: time)
                p = MM.make_inputs(n, T, 31 * n + T, x0_zero=x0_zero, v=v, Kc=3 if like == "cv" else 0)
                w_ell, w_kl = 0.37, 2.5 / (n * T)
                o = MM.step_of(p, w_ell, w_kl)
                small = like == "exp" and n * T <= 600
                ref = _oracle(p, w_ell, w_kl, dense=small)
                for k, dev in _deviations(o, ref, n).items():
                    assert dev <= 1e-10, (n, T, x0_zero, v, k, dev)
                    if dev > worst[1]:
                        worst = (f"N={n} T={T} x0_zero={x0_zero} v={v} {k}", dev)
                if small:
                    for k, want in ref["dense"].items():
                        assert abs(o[k] - want) <= 1e-10 * max(1.0, abs(want)), (n, T, x0_zero, k)
    print(f"restatement vs the oracles ({like}): largest relative deviation {worst[1]:.2e} at {worst[0]}")


def test_oracle_inputs_cover_every_vol_and_grid_start():
    seen_n, seen_t = {}, {}
    for iN, n in enumerate(ORACLE_N):
        for iT, T in enumerate(ORACLE_T):
            for x0_zero in (False, True):
                v = ORACLE_V[(iN + iT + x0_zero) % 3]
                seen_n.setdefault(n, set()).add((x0_zero, v))
                seen_t.setdefault(T, set()).add((x0_zero, v))
    assert all(len(s) == 6 for s in seen_n.values()) and all(len(s) == 6 for s in seen_t.values())


def test_one_task_with_unit_task_covariances_is_the_single_task_step():
    """T = 1, K_t = S_t = 1 (f = 0, raw_var = log(e - 1), Lt = 1): the restatement equals gpcv_markov_ref.step to 1e-12."""
    ghx, ghw = MR.gauss_hermite(75)
    for n, x0_zero, Kc in ((1, True, 0), (2, False, 0), (65, True, 0), (399, False, 0), (130, False, 3)):
        p = MR.make_inputs(n, 50 + n, x0_zero=x0_zero)
        abc1 = MR.make_abc(Kc, n) if Kc else None
        we, wk = 1.0 / n, 0.7 / (n + 3)
        one = MR.step(p["x"], p["v"], J, p["mu"], p["m"], p["rho"], p["gam"], p["y"], ghx, ghw, we, wk, abc=abc1)
        o = MM.step(p["x"], p["v"], J, np.array([p["mu"]]), p["m"][:, None], p["rho"], p["gam"], np.ones((1, 1)), np.zeros(1),
                    np.array([math.log(math.e - 1.0)]), p["y"][:, None], ghx, ghw, we, wk,
                    abc=None if abc1 is None else tuple(a[None, :] for a in abc1))
        close = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-12 * max(1.0, np.abs(np.asarray(b)).max())
        for k, k1 in (("ell", "ell"), ("kl", "kl"), ("quad", "quad"), ("logdet_km", "logdet_k"), ("logdet_sx", "logdet_s"),
                      ("tau_x", "trace"), ("dFdv", "dFdv"), ("F", "F"), ("s", "s"), ("grad_rho", "grad_rho"),
                      ("grad_gamma", "grad_gamma")):
            assert close(o[k], one[k1]), (n, k)
        assert close(o["grad_M"][:, 0], one["grad_m"]) and close(o["grad_c"][0], one["grad_mu"].sum()), n
        assert abs(o["tau_t"] - 1.0) <= 1e-14 and abs(o["logdet_kt"]) <= 1e-14 and o["logdet_st"] == 0.0
        if Kc:
            assert close(o["grad_abc"][0], one["grad_abc"])


BROKEN = ("tau_t", "rho_T", "g2", "st_next")


@pytest.mark.parametrize("broken", BROKEN)
def test_negative_controls_miss_a_gpu_bound(broken):
    """A restatement with ONE mistake that only this step can make, at EVERY input the GPU tests run with T >= 2 and N >= 2:
    some quantity misses its GPU bound (error / bound > 1)."""
    least = (float("inf"), None)
    for c in MM.ALL_CASES:
        n, T, Kc, kind = c
        if n < 2 or T < 2:
            continue
        p, ref, we, wk = MM.case(*c)
        with np.errstate(all="ignore"):
            bad = MM.step_of(p, we, wk, broken=broken)
        ex = max(MM.bound_excess(bad, ref, n).values())
        assert ex > 1.0, (c, ex)
        if ex < least[0]:
            least = (ex, c)
    print(f"broken={broken}: the smallest miss over every GPU input with N, T >= 2 is {least[0]:.1f} x a bound, at {least[1]}")


@pytest.mark.parametrize("cases", [MM.EXP_CASES + MM.KIND_CASES, MM.CV_CASES], ids=["exp-and-kinds", "cv"])
def test_fp32_evaluation_within_half_of_every_gpu_bound(cases):
    """The fp32 evaluation of the restatement (inputs, quadrature nodes and outputs in fp32, recurrences and sums in fp64:
    what the kernels do) at EVERY input the GPU tests run: each quantity within half of its GPU bound."""
    worst = {}
    for c in cases:
        p, ref, we, wk = MM.case(*c)
        o32 = MM.step_of(p, we, wk, dtype=np.float32)
        for k, e in MM.bound_excess(o32, ref, c[0]).items():
            worst[k] = max(worst.get(k, 0.0), e)
            assert e <= 0.5, (c, k, e)
    print("fp32 evaluation, largest error / GPU bound:", {k: f"{e:.4f}" for k, e in worst.items()})


@pytest.mark.parametrize("case", MM.KIND_CASES, ids=lambda c: f"{c[0]}x{c[1]}-K{c[2]}-{c[3]}")
def test_floored_and_clamped_cases_are_not_vacuous(case):
    """At least a third of the (n, t) floored / at least 10 % of the nodes clamped, and nothing so close to a threshold that
    fp32 and fp64 could take different branches: no variance within 0.1 % of min_var, no node within 1e-5 of log min_scale."""
    n, T, Kc, kind = case
    p, _, _, _ = MM.case(*case)
    ghx, _ = MR.gauss_hermite(75)
    s = MR.variances(p["rho"], p["gam"])
    st = (np.tril(p["Lt"]) ** 2).sum(1)
    var = s[:, None] * st[None, :]
    f = p["M"][:, :, None] + np.sqrt(2.0 * np.maximum(var, 1e-6))[:, :, None] * ghx[None, None, :]
    if Kc:
        a, b, c = (t[None, :, None, :] for t in p["abc"])
        scale = (a * np.logaddexp(0.0, b * f[..., None] + c)).sum(-1)
    else:
        scale = np.exp(f)
    floored, clamped = float((var < 1e-6).mean()), float((scale <= 1e-3).mean())
    print(f"{case}: floored {floored:.3f} of the (n, t), clamped {clamped:.3f} of the nodes")
    if kind == "floored":
        assert floored >= 1.0 / 3.0
    else:
        assert clamped >= 0.10
    assert not (np.abs(var / 1e-6 - 1.0) < 1e-3).any()
    assert not (np.abs(np.log(scale) - math.log(1e-3)) < 1e-5).any()


# ------------------------------------------------------------------------------------------------ the model's start-up values
def _model(n, T, param="exp", x0_zero=False, solver="markov"):
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import MultitaskVariationalGP
    x = (torch.arange(n, dtype=torch.float32) + (0 if x0_zero else 1)) / 252
    torch.manual_seed(11)
    lik = VolatilityGaussianLikelihood(param="exp") if param == "exp" else \
        VolatilityGaussianLikelihood(K=1, param="cv", batch_shape=torch.Size([T]))
    return MultitaskVariationalGP(x, num_tasks=T, covar_module=BMKernel(), prior_solver=solver), lik, x


def _running_std(y):
    rs = torch.full(y.shape, float("nan"), dtype=y.dtype)
    for i in range(2, y.shape[0]):
        rs[i] = y[:i].std(0)
    rs[:10] = rs[10]
    return rs


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("param", ["exp", "cv"])
def test_startup_values_equal_the_dense_formula(param, T):
    """inv(Lp Lp') of the start-up values equals 100 L (L'HL + I)^-1 L' built densely in fp64 with K_M: H the DIAGONAL of the
    mean over tasks of the inverse Hessians ("exp": each clamped to [1e-4, 1000]; the dense route's off-diagonal 1e-4 is a
    rank-one term the tridiagonal family cannot carry)."""
    n = 64
    torch.manual_seed(3)
    y = 0.3 * torch.randn(n, T)
    model, lik, x = _model(n, T, param, x0_zero=(T == 3))
    consts0 = [float(m.constant.detach()) for m in model.mean_module.base_means]
    cf0 = model.index_kernel.covar_factor.detach().clone()
    model.initialize_variational_parameters(lik, x, y=y)
    yd = y.double()
    rs = _running_std(yd)
    f = rs.clamp(min=1e-4).log()
    if param == "exp":
        h = (0.5 * yd.pow(-2.0) * (f * 2.0).exp()).clamp(min=1e-4, max=1000.0).mean(1)
        mean = f
    else:
        a, b, c = (t.detach().double().reshape(1, T) for t in (lik.trans_a, lik.trans_b, lik.trans_c))
        mean = ((f / a).exp() - 1 - c) / b
        sigma = ((b * mean + c).exp() + 1).log().mul(a).clamp(min=1e-3)
        h = (((2 + 3 * f.pow(2.0)) * (a * b.pow(2.0) / 2)).pow(-1.0) * sigma.pow(2.0) * (1 + torch.cosh(b * f + c))).mean(1)
    K = torch.tensor(MR.prior_cov(x.double().numpy(), 0.2, J))
    L = torch.linalg.cholesky(K)
    inner = L.mT @ torch.diag_embed(h) @ L + torch.eye(n, dtype=torch.float64)
    want = 100.0 * L @ torch.linalg.solve(inner, L.mT)
    Lp = torch.tensor(MR.dense_root(model.log_diag_precision_root.detach().double().numpy(),
                                    model.coupling.detach().double().numpy()))
    got = torch.linalg.inv(Lp @ Lp.mT)
    assert (got - want).abs().max() <= 5e-6 * want.abs().max()                     # (parameters are stored in fp32)
    assert (model.variational_mean.detach().double() - mean).abs().max() <= 1e-5 * mean.abs().max()
    assert float(model.coupling[-1]) == 0.0
    log_means = rs.clamp(min=1e-4).mean(0).log()
    for t, m in enumerate(model.mean_module.base_means):
        assert abs(float(m.constant.detach()) - consts0[t] - float(log_means[t])) <= 1e-5
    assert torch.equal(model.index_kernel.covar_factor.detach(), cf0 / 10.0)


def test_startup_host_memory_is_linear_at_65536_by_8():
    n, T = 65536, 8
    torch.manual_seed(4)
    y = 0.3 * torch.randn(n, T)
    model, lik, x = _model(n, T)
    tracemalloc.start()
    model.initialize_variational_parameters(lik, x, y=y)
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    assert tuple(model.coupling.shape) == (n,) and torch.isfinite(model.log_diag_precision_root).all()
    assert torch.isfinite(model.variational_mean).all() and tuple(model.variational_mean.shape) == (n, T)
    print(f"start-up values at {n} x {T}: peak traced host memory {peak / 2 ** 20:.1f} MiB")
    assert peak <= 64 * 2 ** 20                                                    # O(N T): an [N,N] fp32 tensor is 16 GiB


# ------------------------------------------------------------------------------------------------ the interface
def test_model_parameters_refusals_and_defaults():
    from volt_amd import train_utils
    from volt_amd.forecast import (GenerateStockPredictionsBatch, GenerateWindPredictionsBatch, _check_gpcv_options,
                                   _forecast_windows, _window_pass)
    from volt_amd.kernels import BMKernel, FBMKernel
    from volt_amd.models import MultitaskVariationalGP
    from volt_amd.variational import MultitaskMarkovVariationalLatent, MultitaskVariationalLatent, VariationalELBO
    from volt_amd import ops
    model, lik, x = _model(8, 3)
    assert [k for k, _ in model.named_parameters()][:4] == ["variational_mean", "log_diag_precision_root", "coupling",
                                                            "variational_task_covar_root"]
    assert "variational_covar_root" not in dict(model.named_parameters())
    assert tuple(model.log_diag_precision_root.shape) == (8,) and tuple(model.coupling.shape) == (8,)
    assert isinstance(model(x), MultitaskMarkovVariationalLatent)
    # the default path: same parameters, same randn draw order, same latent
    torch.manual_seed(11)
    dense = MultitaskVariationalGP(x, num_tasks=3, covar_module=BMKernel())
    torch.manual_seed(11)
    again = MultitaskVariationalGP(x, num_tasks=3, covar_module=BMKernel(), prior_solver="dense")
    assert [k for k, _ in dense.named_parameters()][:3] == ["variational_mean", "variational_covar_root",
                                                           "variational_task_covar_root"]
    assert all(torch.equal(a, b) for a, b in zip(dense.parameters(), again.parameters()))
    assert torch.equal(dense.variational_mean, model.variational_mean)           # (_model seeds with 11 too)
    assert torch.equal(dense.index_kernel.covar_factor, model.index_kernel.covar_factor)
    assert type(dense(x)) is MultitaskVariationalLatent
    sig = inspect.signature
    assert sig(MultitaskVariationalGP.__init__).parameters["prior_solver"].default == "dense"
    assert sig(MultitaskVariationalGP.__init__).parameters["prior_solver"].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (train_utils.FitGPCVMultitask, train_utils.LearnGPCVMultitask):
        assert sig(fn).parameters["solver"].default == "dense"
    for fn in (GenerateStockPredictionsBatch, GenerateWindPredictionsBatch, _forecast_windows, _window_pass):
        assert sig(fn).parameters["multitask_gpcv"].default is False
    assert ops.GpcvMtMarkovWorkspace in VariationalELBO._WS_ATTR and len(VariationalELBO._WS_ATTR) == 5
    with pytest.raises(ValueError, match="BMKernel"):
        MultitaskVariationalGP(x, num_tasks=3, covar_module=FBMKernel(), prior_solver="markov")
    with pytest.raises(ValueError, match="strictly increasing"):
        MultitaskVariationalGP(x.flip(0), num_tasks=3, covar_module=BMKernel(), prior_solver="markov")
    with pytest.raises(ValueError, match="x\\[0\\] >= 0"):
        MultitaskVariationalGP(x - 1, num_tasks=3, covar_module=BMKernel(), prior_solver="markov")
    with pytest.raises(ValueError, match="prior_solver must be"):
        MultitaskVariationalGP(x, num_tasks=3, covar_module=BMKernel(), prior_solver="linear")
    prices = torch.ones(3, 9)
    for fn in (train_utils.FitGPCVMultitask, train_utils.LearnGPCVMultitask):
        with pytest.raises(ValueError, match="kernel='bm'"):
            fn(x, prices, kernel="fbm", solver="markov")
        with pytest.raises(ValueError, match="solver must be"):
            fn(x, prices, solver="linear")
    with pytest.raises(ValueError, match='gpcv_solver="markov"'):
        _check_gpcv_options(None, True, "markov", 3, None)
    with pytest.raises(ValueError, match='gpcv_solver="markov"'):
        _check_gpcv_options(None, "markov", "markov", 3, None)
    with pytest.raises(ValueError, match='gpcv_solver="linear"'):
        _check_gpcv_options(None, "markov", "linear", 3, None)
    with pytest.raises(ValueError, match="multitask_gpcv must be"):
        _check_gpcv_options(None, "banded", "dense", 3, None)
    with pytest.raises(ValueError, match="at most 64"):
        _check_gpcv_options(None, "markov", "dense", 65, None)
    with pytest.raises(ValueError, match="unknown keys"):
        _check_gpcv_options({"solver": "markov"}, "markov", "dense", 3, None)
    assert _check_gpcv_options({"param": "cv"}, "markov", "dense", 3, None) == {"param": "cv"}
    with pytest.raises(ops._lib.VoltHipError):                                     # CPU tensors: no fallback
        model.kl_divergence()
    a = torch.zeros(4, 2)
    with pytest.raises(ops._lib.VoltHipError):
        ops.gpcv_mt_markov_step(torch.arange(1., 5.), torch.tensor([0.2]), a, torch.zeros(2), torch.zeros(4), torch.zeros(4),
                                torch.eye(2), torch.zeros(2), torch.zeros(2), a, torch.zeros(3), torch.zeros(3))


def test_entry_point_validates_arguments_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    assert "volt_gpcv_mt_markov_step_f32" in _lib.EXPORTS and "volt_gpcv_mt_markov_workspace_bytes" in _lib.EXPORTS
    step = L.volt_gpcv_mt_markov_step_f32
    order = ("x", "vol", "M", "c", "rho", "gamma", "Lt", "cf", "rv", "y")
    outs = ("out", "grad_M", "grad_c", "grad_rho", "grad_gamma", "grad_Lt", "grad_cf", "grad_rv")

    def call(**kw):
        a = dict({k: 1 for k in order + outs}, abc=None, Kc=0, gh_x=1, gh_w=1, Q=75, grad_abc=None, info=1, ws=256, N=5, T=3)
        a.update(kw)
        return step(a["x"], a["vol"], 1e-3, *(a[k] for k in order[2:]), a["abc"], a["Kc"], a["gh_x"], a["gh_w"], a["Q"], 1e-6,
                    1e-3, 1.0, 1.0, *(a[k] for k in outs), a["grad_abc"], a["info"], a["ws"], a["N"], a["T"], None)
    codes = dict(x=-1, vol=-2, M=-4, c=-5, rho=-6, gamma=-7, Lt=-8, cf=-9, rv=-10, y=-11, gh_x=-14, gh_w=-15, out=-21, grad_M=-22,
                 grad_c=-23, grad_rho=-24, grad_gamma=-25, grad_Lt=-26, grad_cf=-27, grad_rv=-28, info=-30, ws=-31)
    for name, code in codes.items():
        assert call(**{name: None}) == code, name
    assert call(Kc=1) == -13 and call(abc=1, Kc=0) == -13 and call(abc=1, Kc=9) == -13
    assert call(abc=1, Kc=5) == -29                                                # "cv" without grad_abc
    assert call(Q=0) == -16 and call(Q=1025) == -16
    assert call(ws=264) == -31                                                     # not 256-byte aligned
    assert call(N=0) == -32 and call(T=0) == -33 and call(T=65) == -33


def test_workspace_formula():
    from volt_amd import _lib
    L = _lib.lib()
    al = lambda b: (b + 255) // 256 * 256
    for N, T, Kc in ((1, 1, 0), (399, 8, 0), (130, 3, 5), (399, 64, 8), (4097, 3, 1), (65536, 8, 0)):
        ngh, nch = -(-N // MM.ROWS_TILE), -(-N // MM.GRAM_TILE)
        # fp64: diag P^-1, e^{-2 rho}, the x side's sums, a_n, the partials of b_t, ell and G / G2, K_t^-1, tau_t;
        # fp32: dE/dM and the "cv" parameter partials; each region 256-byte aligned
        want = (3 * al(8 * N) + 2 * al(64) + al(8 * ngh * T) + al(8 * ngh) + al(8 * nch * 2 * T * T) + al(8 * T * T)
                + al(4 * N * T) + al(4 * T * ngh * 3 * Kc))
        assert L.volt_gpcv_mt_markov_workspace_bytes(N, T, Kc) == want, (N, T, Kc)
    assert L.volt_gpcv_mt_markov_workspace_bytes(65536, 8, 0) <= 8 * 2 ** 20       # (one [N,N] fp32 array: 16 GiB)
    for bad in ((0, 3, 0), (5, 0, 0), (5, 65, 0), (5, 3, -1), (5, 3, 9)):
        assert L.volt_gpcv_mt_markov_workspace_bytes(*bad) == 0


def test_kernels_cross_compile_without_scratch_or_spills(tmp_path):
    from volt_amd.build import FLAGS, SOURCES, _hipcc
    assert "gpcv_mt_markov.hip" in SOURCES
    src = os.path.join(ROOT, "volt_amd", "csrc", "gpcv_mt_markov.hip")
    r = subprocess.run([_hipcc(), *FLAGS, "-c", src, "-o", str(tmp_path / "gpcv_mt_markov.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel, count in (("front_kernel", 1), ("rows_kernel", 9), ("task_kernel", 1), ("back_kernel", 1)):
        blocks = [b for b in r.stderr.split("Function Name: ")[1:] if kernel in b.split()[0]]
        assert len(blocks) == count, [b.split()[0] for b in blocks]               # rows: "exp" and "cv" with K = 1 .. 8
        for b in blocks:
            name = b.split()[0]
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
            assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
            assert int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, name
    with open(src) as fh:
        text = fh.read()
    assert "atomic" not in text.replace("No atomics", "").replace("no atomics", "")
