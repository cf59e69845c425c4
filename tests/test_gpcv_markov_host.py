"""CPU checks of the O(N) GPCV step for the Markov variational family: the loop restatement
tests/gpcv_markov_ref.py against the dense oracle, its negative controls, the draw, the O(N) start-up values, the interface,
and the fp32 evaluation against the GPU tests' bounds.  No device is needed."""
import math
import os
import re
import subprocess
import sys
import time
import tracemalloc

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gpcv_cv_ref as CV  # noqa: E402
import gpcv_markov_ref as MR  # noqa: E402
from oracle import gpcv_oracle as GO  # noqa: E402

J = 1e-3
# the GPU tests' bounds (tests/test_gpu_gpcv_markov.py holds the kernel to these; the project's existing GPCV bounds)
SCALAR_TOL, GRAD_TOL, DV_TOL = 5e-5, 2e-3, 2e-3


def _dense_terms(p, w_ell, w_kl, abc=None):
    """F, its pieces and autograd gradients through the DENSE S = P^-1, Lq = chol(S) and oracle.gpcv_oracle.elbo_terms.
    The oracle adds j I to the K it is given: K_M - j I makes that exactly K_M."""
    dt = torch.float64
    t = lambda a: torch.tensor(a, dtype=dt, requires_grad=True)
    x = torch.tensor(p["x"], dtype=dt)
    m, rho, gam, v, mu = t(p["m"]), t(p["rho"]), t(p["gam"]), t(p["v"]), t(p["mu"])
    n = len(p["m"])
    d = rho.exp()
    Lp = torch.diag_embed(d)
    if n > 1:
        Lp = Lp + torch.diag_embed(gam[:-1] * d[:-1], offset=-1)
    S = torch.linalg.inv(Lp @ Lp.mT)
    S = 0.5 * (S + S.mT)
    Lq = torch.linalg.cholesky(S)
    K = v * torch.minimum(x[:, None], x[None, :]) + J - J * torch.eye(n, dtype=dt)
    ghx, ghw = GO.gauss_hermite(75)
    y = torch.tensor(p["y"], dtype=dt)
    terms = dict(GO.elbo_terms(m, Lq, mu, K, y, ghx, ghw))
    leaves = [m, mu, rho, gam, v]
    if abc is not None:
        tabc = [t(a) for a in abc]
        terms["ell"] = CV.ell(m, Lq, y, *tabc, ghx, ghw)[0]
        leaves += tabc
    F = w_ell * terms["ell"] - w_kl * terms["kl"]
    grads = torch.autograd.grad(F, leaves, allow_unused=True)
    grads = [torch.zeros_like(leaf) if g is None else g for g, leaf in zip(grads, leaves)]     # (N = 1: gamma is unused)
    out = {k: float(terms[k].detach()) for k in ("ell", "kl", "quad", "logdet_k", "logdet_s", "trace")}
    out.update(F=float(F.detach()), s=S.diagonal().detach().numpy(), grad_m=grads[0].numpy(), grad_mu=float(grads[1]),
               grad_rho=grads[2].numpy(), grad_gamma=grads[3].numpy(), dFdv=float(grads[4]))
    if abc is not None:
        out["grad_abc"] = np.stack([g.numpy() for g in grads[5:]])
    return out


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _compare_to_dense(o, ref, n):
    """Largest deviation relative to each quantity's scale."""
    devs = {k: abs(o[k] - ref[k]) / max(1.0, abs(ref[k])) for k in ("ell", "kl", "quad", "logdet_k", "logdet_s", "trace", "F")}
    devs["dFdv"] = abs(o["dFdv"] - ref["dFdv"]) / max(abs(ref["dFdv"]), 1e-300) if ref["dFdv"] != 0 else abs(o["dFdv"])
    devs["s"] = _rel(o["s"], ref["s"])
    devs["grad_m"] = _rel(o["grad_m"], ref["grad_m"])
    devs["grad_mu"] = abs(o["grad_mu"].sum() - ref["grad_mu"]) / max(np.abs(o["grad_mu"]).max(), abs(ref["grad_mu"]), 1e-300)
    devs["grad_rho"] = _rel(o["grad_rho"], ref["grad_rho"])
    if n > 1:
        devs["grad_gamma"] = _rel(o["grad_gamma"][:-1], ref["grad_gamma"][:-1])
    if "grad_abc" in ref:
        devs["grad_abc"] = _rel(o["grad_abc"], ref["grad_abc"])
    return devs


@pytest.mark.parametrize("like", ["exp", "cv"])
def test_restatement_matches_the_dense_oracle(like):
    ghx, ghw = MR.gauss_hermite(75)
    worst = ("", 0.0)
    seed = 0
    for n in (1, 2, 3, 64, 65, 399):
        for x0_zero in (False, True):
            for v in (0.05, 0.2, 0.9):
                seed += 1
                p = MR.make_inputs(n, seed, x0_zero=x0_zero, v=v)
                abc = MR.make_abc(3, seed) if like == "cv" else None
                w_ell, w_kl = 1.0 / n, 0.7 / (n + 3)
                o = MR.step(p["x"], p["v"], J, p["mu"], p["m"], p["rho"], p["gam"], p["y"], ghx, ghw, w_ell, w_kl, abc=abc)
                ref = _dense_terms(p, w_ell, w_kl, abc)
                for k, dev in _compare_to_dense(o, ref, n).items():
                    assert dev <= 1e-10, (n, x0_zero, v, k, dev)
                    if dev > worst[1]:
                        worst = (f"N={n} x0_zero={x0_zero} v={v} {k}", dev)
    print(f"restatement vs dense oracle ({like}): largest relative deviation {worst[1]:.2e} at {worst[0]}")


def _gpu_bound_excess(o, ref, n):
    """Each quantity's error as a multiple of the GPU tests' bound for it."""
    ex = {k: abs(o[k] - ref[k]) / (SCALAR_TOL * max(1.0, abs(ref[k]))) for k in ("ell", "kl", "quad", "logdet_k", "logdet_s",
                                                                                  "trace", "F")}
    ex["dFdv"] = abs(o["dFdv"] - ref["dFdv"]) / (DV_TOL * abs(ref["dFdv"])) if ref["dFdv"] != 0 else float(o["dFdv"] != 0)
    for k in MR.GRADS:
        ex[k] = np.abs(o[k] - ref[k]).max() / (GRAD_TOL * max(np.abs(ref[k]).max(), 1e-300)) if n > 1 or k != "grad_gamma" else 0.0
    if ref.get("grad_abc") is not None:
        ex["grad_abc"] = np.abs(o["grad_abc"] - ref["grad_abc"]).max() / (GRAD_TOL * np.abs(ref["grad_abc"]).max())
    return ex


def _case_id(c):
    return f"{c[1]}x{c[0]}-K{c[2]}-{c[3]}"


@pytest.mark.parametrize("broken", ["e", "q0", "adjoint"])
def test_negative_controls_are_far_outside_the_gpu_bounds(broken):
    """A restatement with ONE of the three mistakes, at EVERY input the GPU tests run (MR.ALL_CASES, every series): some
    quantity misses its GPU bound by more than 10 x (a non-finite F counts: q_0 = 0 at x_0 = 0 without the level's jitter) --
      "q0"             at every input;
      "e", "adjoint"   at every input with N >= 2 except the "floored" kind.  Both mistakes act through the couplings: at N = 1
                       there is none (asserted: the broken restatement equals the right one), and the floored inputs set every
                       second coupling to 1e-4 and every second variance to 1e-7 on purpose, which all but decouples the
                       recurrences (measured there: "e" 2.4 x, "adjoint" 0.8 x of a bound); they are not claimed there."""
    least = (float("inf"), None)
    for c in MR.ALL_CASES:
        n, B, Kc, kind = c
        ps, refs, we, wk = MR.case(*c)
        for b, (p, ref) in enumerate(zip(ps, refs)):
            with np.errstate(all="ignore"):
                bad = MR.step_of(p, we, wk, broken=broken)
            if broken != "q0" and n == 1:
                assert bad["F"] == ref["F"] and all((bad[k] == ref[k]).all() for k in MR.GRADS)
                continue
            if broken != "q0" and kind == "floored":
                continue
            ex = float("inf") if not math.isfinite(bad["F"]) else max(_gpu_bound_excess(bad, ref, n).values())
            assert ex > 10.0, (c, b, ex)
            if ex < least[0]:
                least = (ex, (_case_id(c), b))
    print(f"broken={broken}: the smallest miss over every GPU input it is claimed at is {least[0]:.1f} x a bound, at {least[1]}")


@pytest.mark.parametrize("cases", [MR.EXP_CASES + MR.KIND_CASES, MR.CV_CASES], ids=["exp-and-kinds", "cv"])
def test_fp32_evaluation_within_half_of_every_gpu_bound(cases):
    """The fp32 evaluation of the restatement (inputs, quadrature and outputs in fp32, recurrences in fp64: what the kernel
    does) at EVERY input the GPU tests run, every series: each quantity within half of its GPU bound."""
    worst = {}
    for c in cases:
        n = c[0]
        ps, refs, we, wk = MR.case(*c)
        for b, (p, ref) in enumerate(zip(ps, refs)):
            o32 = MR.step_of(p, we, wk, dtype=np.float32)
            for k, e in _gpu_bound_excess(o32, ref, n).items():
                worst[k] = max(worst.get(k, 0.0), e)
                assert e <= 0.5, (c, b, k, e)
    print("fp32 evaluation, largest error / GPU bound:", {k: f"{e:.4f}" for k, e in worst.items()})


def test_draw_matches_a_triangular_solve():
    g = np.random.default_rng(5)
    for n in (1, 2, 3, 65, 399):
        p = MR.make_inputs(n, 20 + n)
        eps = g.standard_normal((4, n))
        got = MR.draw(p["m"], p["rho"], p["gam"], eps)
        Lp = torch.tensor(MR.dense_root(p["rho"], p["gam"]))
        want = p["m"] + torch.linalg.solve_triangular(Lp.mT, torch.tensor(eps).mT, upper=True).mT.numpy()
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), n
    # and its covariance is P^-1
    Lp = MR.dense_root(p["rho"], p["gam"])
    U = MR.draw(np.zeros(n), p["rho"], p["gam"], np.eye(n))             # rows: Lp^-T e_k
    assert np.abs(U.T @ U - np.linalg.inv(Lp @ Lp.T)).max() <= 1e-9 * np.abs(U.T @ U).max()
    assert np.abs(np.diag(U.T @ U) - MR.variances(p["rho"], p["gam"])).max() <= 1e-9 * np.abs(U).max() ** 2


def _model(n, solver, x0_zero=False, param="exp", batch=None):
    from volt_amd import gp
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import SingleTaskVariationalGP
    x = (torch.arange(n, dtype=torch.float32) + (0 if x0_zero else 1)) / 252
    kw = {"batch_shape": torch.Size([batch])} if batch else {}
    lik = VolatilityGaussianLikelihood(param="exp") if param == "exp" else VolatilityGaussianLikelihood(K=1, param="cv", **kw)
    model = SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=lik, use_piv_chol_init=False,
                                    mean_module=gp.ConstantMean(**kw), covar_module=BMKernel(**kw),
                                    learn_inducing_locations=False, use_whitened_var_strat=False, prior_solver=solver)
    return model, lik, x


def _startup_reference(x, h, vol=0.2):
    """chol(S^-1 / 100) of the reference's S = L (L'HL + I)^-1 L' = (K^-1 + H)^-1 with K = K_M, dense fp64."""
    K = torch.tensor(MR.prior_cov(x.double().numpy(), vol, J))
    L = torch.linalg.cholesky(K)
    n = len(x)
    H = torch.diag_embed(torch.as_tensor(h, dtype=torch.float64))
    inner = L.mT @ H @ L + torch.eye(n, dtype=torch.float64)
    S = L @ torch.linalg.solve(inner, L.mT)
    ident = (torch.linalg.inv(S) - (torch.linalg.inv(K) + H)).abs().max() / torch.linalg.inv(S).abs().max()
    return torch.linalg.cholesky(torch.linalg.inv(S) / 100.0), float(ident)


@pytest.mark.parametrize("x0_zero", [False, True])
@pytest.mark.parametrize("param", ["exp", "cv"])
def test_startup_values_equal_the_dense_formula(param, x0_zero):
    n = 60
    torch.manual_seed(3)
    y = 0.3 * torch.randn(n)
    model, lik, x = _model(n, "markov", x0_zero, param)
    model.initialize_variational_parameters(lik, x, y=y)
    dist = model.variational_strategy._variational_distribution
    # h and the mean as initialize_variational_parameters computes them, restated in fp64
    rs = GO.running_std(y.double())
    f = rs.clamp(min=1e-4).log()
    if param == "exp":
        h = (0.5 * y.double().pow(-2.0) * (f * 2.0).exp()).clamp(min=1e-4, max=1000.0)       # H's clamped diagonal only
        mean = f
    else:
        a, b, c = (t.detach().double().reshape(()) for t in (lik.trans_a, lik.trans_b, lik.trans_c))
        mean = ((f / a).exp() - 1 - c) / b
        sigma = ((b * mean + c).exp() + 1).log().mul(a).clamp(min=1e-3)
        h = ((2 + 3 * f.pow(2.0)) * (a * b.pow(2.0) / 2)).pow(-1.0) * sigma.pow(2.0) * (1 + torch.cosh(b * f + c))
    Lref, ident = _startup_reference(x, h)
    assert ident <= 1e-9                                                           # S = (K^-1 + H)^-1
    lat = model(x)
    Lp = lat.precision_root
    assert (Lp - Lref).abs().max() <= 2e-6 * Lref.abs().max()                      # (parameters are stored in fp32)
    assert (dist.variational_mean.double() - mean).abs().max() <= 1e-5 * mean.abs().max()
    assert abs(float(model.mean_module.constant) - float(rs.mean().log())) <= 1e-5
    assert float(dist.coupling[-1]) == 0.0


def test_startup_is_linear_in_n_and_allocates_nothing_square():
    n = 65536
    torch.manual_seed(4)
    y = 0.3 * torch.randn(2, n)
    model, lik, x = _model(n, "markov", batch=2)
    tracemalloc.start()
    t0 = time.perf_counter()
    model.initialize_variational_parameters(lik, x, y=y)
    dt = time.perf_counter() - t0
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    dist = model.variational_strategy._variational_distribution
    assert tuple(dist.coupling.shape) == (2, n) and torch.isfinite(dist.log_diag_precision_root).all()
    print(f"start-up values at 2 x {n}: {dt:.2f} s, peak traced host memory {peak / 2 ** 20:.1f} MiB")
    assert peak <= 64 * 2 ** 20                                                    # O(N): an [N,N] fp32 tensor is 16 GiB
    assert dt < 30.0


def test_constructor_validation_and_state_dict():
    from volt_amd import gp, train_utils
    from volt_amd.forecast import _check_gpcv_options
    from volt_amd.kernels import FBMKernel
    from volt_amd.models import SingleTaskVariationalGP
    from volt_amd.variational import MarkovVariationalDistribution, MarkovVariationalLatent
    model, lik, x = _model(8, "markov")
    names = set(model.state_dict())
    pre = "variational_strategy._variational_distribution."
    assert {pre + "variational_mean", pre + "log_diag_precision_root", pre + "coupling"} <= names
    assert pre + "chol_variational_covar" not in names
    assert isinstance(model.variational_strategy._variational_distribution, MarkovVariationalDistribution)
    assert isinstance(model(x), MarkovVariationalLatent)
    assert "markov" in SingleTaskVariationalGP.PRIOR_SOLVERS and "markov" in train_utils.GPCV_SOLVERS
    K = model.forward(model.variational_strategy.inducing_points).lazy_covariance_matrix.evaluate()
    assert torch.allclose(K.double(), torch.tensor(MR.prior_cov(x.double().numpy(), 0.2, J)), rtol=1e-5)
    kw = dict(likelihood=lik, use_piv_chol_init=False, mean_module=gp.ConstantMean(), learn_inducing_locations=False,
              use_whitened_var_strat=False, prior_solver="markov")
    with pytest.raises(ValueError, match="BMKernel"):
        SingleTaskVariationalGP(init_points=x.view(-1, 1), covar_module=FBMKernel(), **kw)
    from volt_amd.kernels import BMKernel
    with pytest.raises(ValueError, match="strictly increasing"):
        SingleTaskVariationalGP(init_points=x.flip(0).view(-1, 1), covar_module=BMKernel(), **kw)
    with pytest.raises(ValueError, match="x\\[0\\] >= 0"):
        SingleTaskVariationalGP(init_points=(x - 1).view(-1, 1), covar_module=BMKernel(), **kw)
    with pytest.raises(ValueError, match="prior_solver must be"):
        SingleTaskVariationalGP(init_points=x.view(-1, 1), covar_module=BMKernel(), **{**kw, "prior_solver": "banded"})
    with pytest.raises(ValueError, match="kernel='bm'"):
        train_utils.FitGPCV(x, torch.ones(9), kernel="fbm", solver="markov")
    with pytest.raises(ValueError, match="kernel='bm'"):
        train_utils.LearnGPCV(x, torch.ones(9), kernel="fbm", solver="markov")
    with pytest.raises(ValueError, match='gpcv_solver="markov"'):
        _check_gpcv_options(None, True, "markov", 3, None)
    assert train_utils._auto_graph(None, torch.ones(4), launch_bound=True) is False        # (a CPU target never captures)


def test_entry_points_validate_arguments_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    for name in ("volt_gpcv_markov_step_f32", "volt_gpcv_markov_workspace_bytes", "volt_markov_root_draw_f32",
                 "volt_markov_root_var_f32"):
        assert name in _lib.EXPORTS
    step = L.volt_gpcv_markov_step_f32
    # (x, vol, jitter, resid, m, rho, gamma, y, abc, Kc, gh_x, gh_w, Q, min_var, min_scale, w_ell, w_kl, out, grad_m, grad_mu,
    #  grad_rho, grad_gamma, grad_abc, info, workspace, B, N, stream)
    def call(**kw):
        a = dict(x=1, vol=1, resid=1, m=1, rho=1, gamma=1, y=1, abc=None, Kc=0, gh_x=1, gh_w=1, Q=75, out=1, grad_m=1, grad_mu=1,
                 grad_rho=1, grad_gamma=1, grad_abc=None, info=1, ws=256, B=2, N=5)
        a.update(kw)
        return step(a["x"], a["vol"], 1e-3, a["resid"], a["m"], a["rho"], a["gamma"], a["y"], a["abc"], a["Kc"], a["gh_x"],
                    a["gh_w"], a["Q"], 1e-6, 1e-3, 1.0, 1.0, a["out"], a["grad_m"], a["grad_mu"], a["grad_rho"], a["grad_gamma"],
                    a["grad_abc"], a["info"], a["ws"], a["B"], a["N"], None)
    for name, code in (("x", -1), ("vol", -2), ("resid", -4), ("m", -5), ("rho", -6), ("gamma", -7), ("y", -8), ("gh_x", -11),
                       ("gh_w", -12), ("out", -18), ("grad_m", -19), ("grad_mu", -20), ("grad_rho", -21), ("grad_gamma", -22),
                       ("info", -24), ("ws", -25)):
        assert call(**{name: None}) == code, name
    assert call(Kc=1) == -10 and call(abc=1, Kc=0) == -10 and call(abc=1, Kc=9) == -10
    assert call(abc=1, Kc=5) == -23                                               # "cv" without grad_abc
    assert call(Q=0) == -13 and call(Q=1025) == -13
    assert call(ws=264) == -25                                                     # not 256-byte aligned
    assert call(B=0) == -26 and call(B=65536) == -26 and call(N=0) == -27
    draw = L.volt_markov_root_draw_f32                                            # (m, rho, gamma, eps, out, B, reps, N, stream)
    for k in range(5):
        ptrs = [1] * 5
        ptrs[k] = None
        assert draw(*ptrs, 2, 3, 5, None) == -(k + 1)
    assert draw(*[1] * 5, 0, 3, 5, None) == -6
    assert draw(*[1] * 5, 2, 0, 5, None) == -7 and draw(*[1] * 5, 2 ** 16, 2 ** 15, 5, None) == -7
    assert draw(*[1] * 5, 2 ** 12, 2 ** 12, 5, None) == -7                         # 2^24 workgroups of 256: 2^32 threads
    assert draw(*[1] * 5, 2, 3, 0, None) == -8
    var = L.volt_markov_root_var_f32                                              # (rho, gamma, var, B, N, stream)
    for k in range(3):
        ptrs = [1] * 3
        ptrs[k] = None
        assert var(*ptrs, 2, 5, None) == -(k + 1)
    assert var(1, 1, 1, 0, 5, None) == -4 and var(1, 1, 1, 2, 0, None) == -5


def test_workspace_formula():
    from volt_amd import _lib
    L = _lib.lib()
    al = lambda b: (b + 255) // 256 * 256
    for B, N, Kc in ((1, 1, 0), (1, 399, 0), (3, 130, 5), (65, 399, 8), (2, 65536, 0)):
        # diag S and e^{-2 rho} in fp64, the rows' dE/dvar and dE/dm in fp32: 24 B N bytes, each region 256-byte aligned
        assert L.volt_gpcv_markov_workspace_bytes(B, N, Kc) == 2 * al(8 * B * N) + al(8 * B * N)
    assert L.volt_gpcv_markov_workspace_bytes(2, 65536, 0) <= 4 * 2 ** 20
    for bad in ((0, 5, 0), (2, 0, 0), (2, 5, -1), (2, 5, 9)):
        assert L.volt_gpcv_markov_workspace_bytes(*bad) == 0


def test_cpu_tensors_raise():
    from volt_amd import ops
    from volt_amd._lib import VoltHipError
    a = torch.zeros(1, 4)
    with pytest.raises(VoltHipError):
        ops.markov_root_draw(a, a, a, torch.zeros(1, 2, 4))
    with pytest.raises(VoltHipError):
        ops.markov_root_var(a, a)
    with pytest.raises(VoltHipError):
        ops.gpcv_markov_step(torch.arange(1., 5.), torch.tensor([0.2]), a, a, a, a, a, torch.zeros(3), torch.zeros(3))


def test_markov_kernels_cross_compile_without_scratch_or_spills(tmp_path):
    from volt_amd.build import FLAGS, SOURCES, _hipcc
    assert "gpcv_markov.hip" in SOURCES
    src = os.path.join(ROOT, "volt_amd", "csrc", "gpcv_markov.hip")
    r = subprocess.run([_hipcc(), *FLAGS, "-c", src, "-o", str(tmp_path / "gpcv_markov.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel, count in (("gpcv_markov_step_kernel", 9), ("markov_root_draw_kernel", 1), ("markov_root_var_kernel", 1)):
        blocks = [b for b in r.stderr.split("Function Name: ")[1:] if kernel in b.split()[0]]
        assert len(blocks) == count, [b.split()[0] for b in blocks]               # the step: "exp" and "cv" with K = 1 .. 8
        for b in blocks:
            name = b.split()[0]
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
            assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
            assert int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, name
            print(name, "VGPRs", re.search(r" VGPRs: (\d+)", b).group(1), "occupancy",
                  re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1), "static LDS",
                  re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
    for path in (src, os.path.join(ROOT, "volt_amd", "csrc", "markov_scan.h")):      # (the scan and the sums live in the header)
        with open(path) as fh:
            text = fh.read()
        assert "atomic" not in text.replace("no atomics", ""), path
    lib = os.path.join(ROOT, "volt_amd", "csrc", "libvolt_hip.so")
    from volt_amd import _lib
    _lib.lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    for name in ("volt_gpcv_markov_step_f32", "volt_gpcv_markov_workspace_bytes", "volt_markov_root_draw_f32",
                 "volt_markov_root_var_f32"):
        assert f" T {name}" in syms
