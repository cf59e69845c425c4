"""CPU checks of the natural-gradient update of the Markov variational family: the loop restatement
tests/gpcv_natgrad_ref.py against dense algebra, its fixed points under both likelihoods, its negative controls, the trainer's
restatement against fp64 Adam, the GPU tests' bounds, and the interface.  No device is needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gpcv_markov_ref as MR  # noqa: E402
import gpcv_natgrad_ref as NR  # noqa: E402

J = MR.J
GRADS = ("grad_m", "grad_rho", "grad_gamma")


def _largest_gradient(p, we, wk, names=GRADS):
    o = MR.step_of(p, we, wk)
    return max(np.abs(o[k]).max() for k in names), float(o["F"])


# ------------------------------------------------------------------------------------------------ the recurrences
@pytest.mark.parametrize("n", [1, 2, 3, 64, 399])
def test_recurrences_match_dense_algebra(n):
    """One update from random sites at beta = 0.5: Lp Lp' of the new (rho, gamma) is K_M^-1 + diag(lam2), and the new mean is
    mu + P^-1 lam1 by numpy.linalg.solve."""
    p = MR.make_inputs(n, 40 + n)
    ghx, ghw = MR.gauss_hermite(75)
    g = np.random.default_rng(n)
    u = NR.update(p["x"], p["v"], J, p["mu"], p["m"], p["rho"], p["gam"], p["y"], ghx, ghw, 1.0 / n, 0.7 / (n + 3),
                  g.standard_normal(n), g.uniform(0, 5, n), 0.5)
    diag, off = MR.prior_precision(p["x"], p["v"], J)
    P = np.diag(diag + u["lam2"]) + np.diag(off, -1) + np.diag(off, 1)
    Lp = MR.dense_root(u["rho"], u["gam"])
    assert u["gam"][-1] == 0.0
    assert np.abs(Lp @ Lp.T - P).max() <= 1e-12 * np.abs(P).max()
    want = p["mu"] + np.linalg.solve(P, u["lam1"])
    assert np.abs(u["m"] - want).max() <= 1e-10 * max(np.abs(want).max(), 1.0)
    assert (u["lam2"] >= 0).all()


# ------------------------------------------------------------------------------------------------ fixed points
@pytest.mark.parametrize("n", [3, 64, 399])
def test_exp_likelihood_reaches_the_optimum_in_ten_updates(n):
    """Step 1, hyperparameters fixed, w_ell != w_kl: the largest of the step's gradients over m, rho, gamma falls by 1e-8 (and
    more) in ten updates from q = prior's sites, and F rises."""
    ps, we, wk = MR.case_inputs(n, 1)
    assert we != wk
    g0, F0 = _largest_gradient(ps[0], we, wk)
    _, Fs, q = NR.iterate(ps[0], we, wk, 10)
    g10, F10 = _largest_gradient(q, we, wk)
    print(f"exp N = {n}: largest gradient {g0:.3e} -> {g10:.3e} (ratio {g10 / g0:.1e}); F {F0:.6f} -> {F10:.6f}; "
          f"F monotone: {bool((np.diff([F0] + Fs) >= 0).all())}")
    assert g10 <= 1e-8 * g0
    assert F10 > F0


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("n", [64, 399])
def test_cv_likelihood_reaches_the_clamped_optimum(n, K):
    """"cv" is not log-concave: sites that want a negative lam2 are clamped at 0 and the iteration converges to the optimum
    under that constraint -- grad_m -> 0 (K_M^-1 d = r gm at any fixed point), nothing is asserted of grad_rho.  The clamped
    count is the number of points with dE/ds > 0, and no site is negative."""
    ps, we, wk = MR.case_inputs(n, 1, K)
    g0, _ = _largest_gradient(ps[0], we, wk, ("grad_m",))
    u, Fs, q = NR.iterate(ps[0], we, wk, 40, beta=0.5)
    g40, _ = _largest_gradient(q, we, wk, ("grad_m",))
    o = MR.step_of(q, we, wk)
    print(f"cv K = {K} N = {n}: grad_m {g0:.3e} -> {g40:.3e}; grad_rho {np.abs(o['grad_rho']).max():.2e} grad_gamma "
          f"{np.abs(o['grad_gamma']).max():.2e}; clamped {u['clamped']}; lowest F on the way {min(Fs):.3f}")
    assert g40 <= 1e-5 * g0
    assert u["clamped"] == int((u["gv"] > 0).sum()) and u["clamped"] > 0
    assert (u["lam2"] >= 0).all()


# ------------------------------------------------------------------------------------------------ negative controls
@pytest.mark.parametrize("broken", ["t1", "r", "clamp"])
def test_negative_controls_break_a_fixed_point_check(broken):
    """Each deliberate mistake misses one of the checks above by more than 10 x its bound: "t1" (t1 without t2 d) and "r"
    (r = 1 although w_ell != w_kl) leave grad_m far from 0 under the "exp" likelihood.  "clamp" (no clamp under "cv") still
    converges on these data (a negative lam2 need not break a pivot), so it is caught by the check with bound 0, no site below
    0: it leaves more than ten sites negative, the lowest a hundred times further from 0 than a rounding of the largest."""
    if broken == "clamp":
        ps, we, wk = MR.case_inputs(64, 1, 1)
        u, _, _ = NR.iterate(ps[0], we, wk, 40, beta=0.5, broken=broken)
        print(f"{broken}: {int((u['lam2'] < 0).sum())} sites below 0, lowest {u['lam2'].min():.3e}, largest {u['lam2'].max():.3e}")
        assert (u["lam2"] < 0).sum() > 10 and u["lam2"].min() < -100 * 2.0 ** -23 * u["lam2"].max()
        return
    ps, we, wk = MR.case_inputs(64, 1)
    g0, _ = _largest_gradient(ps[0], we, wk)
    _, _, q = NR.iterate(ps[0], we, wk, 10, broken=broken)
    g10, _ = _largest_gradient(q, we, wk)
    print(f"{broken}: largest gradient {g0:.3e} -> {g10:.3e}")
    assert g10 > 10 * 1e-8 * g0


# ------------------------------------------------------------------------------------------------ the trainer's restatement
def _series(n, seed):
    """The scaled returns of a synthetic price series and the grid, as FitGPCV forms them."""
    from volt_amd.synthetic import sde_series
    F = np.asarray(sde_series(n, seed)[0], dtype=np.float64)
    x = np.arange(n) / 252.0
    return x, (F[1:] - F[:-1]) / F[:-1] / (x[1] - x[0]) ** 0.5


@pytest.mark.parametrize("n,seed,ng_it,adam_it", [(399, 2021, 50, 200), (64, 2021, 10, 50)])
def test_fit_overtakes_fp64_adam_from_the_same_start(n, seed, ng_it, adam_it):
    """``fit()`` (natural-gradient q, Adam on the constant and raw vol) against ``learn()`` (Adam on everything) from the
    same start -- the prior's q: F after ``ng_it`` iterations is at least Adam's after ``adam_it``."""
    x, yy = _series(n, seed)
    diag, off = MR.prior_precision(x, 0.2, J)
    rho, gam = MR.tridiag_root(diag, off)
    start = (np.full(n, -1.0), rho, gam, np.array([-1.0]))
    ng, _ = NR.fit(x, yy, start, ng_it)
    adam, _ = MR.learn(x, yy, start, adam_it)
    print(f"N = {n}: F after {ng_it} natural-gradient iterations {-ng[-1]:.4f}, after {adam_it} of Adam {-adam[-1]:.4f} "
          f"(margin {adam[-1] - ng[-1]:.4f})")
    assert -ng[-1] >= -adam[-1]


# ------------------------------------------------------------------------------------------------ the GPU tests' bounds
def test_gpu_bounds_and_the_clamped_count_cap():
    """Per GPU case: the effect of fp32 rows on the CPU (what the GPU bound of m, rho, gamma is made of), and the share of
    points whose clamp decision is left out of the GPU's count (gpcv_natgrad_ref.doubtful): at most 1 % over all cases."""
    worst = dict(m=0.0, rho=0.0, gam=0.0, lam1=0.0, lam2=0.0)
    left, total = 0, 0
    for n, B, Kc, kind in NR.ALL_CASES:
        ps, sites, refs, refs32, we, wk = NR.case(n, B, Kc, kind)
        scales = NR.site_scales(refs)
        for ref, r32 in zip(refs, refs32):
            for k in worst:
                worst[k] = max(worst[k], np.abs(r32[k] - ref[k]).max() / scales.get(k, max(np.abs(ref[k]).max(), 1e-300)))
            d = NR.doubtful(ref, r32)
            left, total = left + int(d.sum()), total + len(d)
            assert ((r32["gv"] > 0) == (ref["gv"] > 0))[~d].all()
    most = left / total
    assert left <= 0.01 * total, (left, total)                         # (over the points of every case, as the GPU test counts)
    print("fp32 rows against fp64, of the largest entry:", {k: f"{v:.1e}" for k, v in worst.items()},
          f"; largest share of points left out of the clamped count {most:.4f}")
    assert worst["lam1"] <= 0.1 * NR.SITE_TOL and worst["lam2"] <= 0.1 * NR.SITE_TOL


# ------------------------------------------------------------------------------------------------ the library
def test_entry_points_validate_arguments_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    assert "volt_gpcv_markov_ng_f32" in _lib.EXPORTS and "volt_gpcv_markov_ng_workspace_bytes" in _lib.EXPORTS
    assert _lib.ABI_VERSION == L.volt_abi_version()
    al = lambda b: (b + 255) // 256 * 256
    for B, N, Kc in ((1, 1, 0), (1, 399, 0), (3, 130, 5), (65, 399, 8), (2, 65536, 0)):
        assert L.volt_gpcv_markov_ng_workspace_bytes(B, N, Kc) == 4 * al(8 * B * N)
    for bad in ((0, 5, 0), (65536, 5, 0), (2, 0, 0), (2, 5, -1), (2, 5, 9)):
        assert L.volt_gpcv_markov_ng_workspace_bytes(*bad) == 0
    ng = L.volt_gpcv_markov_ng_f32

    def call(**kw):
        a = dict(x=1, vol=1, mu=1, m=1, rho=1, gamma=1, y=1, abc=None, Kc=0, gh_x=1, gh_w=1, Q=75, w_kl=1.0, step=1.0, lam1=1,
                 lam2=1, m_out=1, rho_out=1, gamma_out=1, out=1, info=1, ws=256, B=2, N=5)
        a.update(kw)
        return ng(a["x"], a["vol"], 1e-3, a["mu"], a["m"], a["rho"], a["gamma"], a["y"], a["abc"], a["Kc"], a["gh_x"], a["gh_w"],
                  a["Q"], 1e-6, 1e-3, 1.0, a["w_kl"], a["step"], a["lam1"], a["lam2"], a["m_out"], a["rho_out"], a["gamma_out"],
                  a["out"], a["info"], a["ws"], a["B"], a["N"], None)
    for name, code in (("x", -1), ("vol", -2), ("mu", -4), ("m", -5), ("rho", -6), ("gamma", -7), ("y", -8), ("gh_x", -11),
                       ("gh_w", -12), ("lam1", -19), ("lam2", -20), ("m_out", -21), ("rho_out", -22), ("gamma_out", -23),
                       ("out", -24), ("info", -25), ("ws", -26)):
        assert call(**{name: None}) == code, name
    assert call(Kc=1) == -10 and call(abc=1, Kc=0) == -10 and call(abc=1, Kc=9) == -10
    assert call(Q=0) == -13 and call(Q=1025) == -13
    assert call(w_kl=0.0) == -17 and call(w_kl=float("nan")) == -17
    assert call(step=0.0) == -18 and call(step=1.0 + 1e-12) == -18 and call(step=-0.5) == -18 and call(step=float("nan")) == -18
    assert call(ws=264) == -26                                                     # not 256-byte aligned
    assert call(B=0) == -27 and call(B=65536) == -27 and call(N=0) == -28
    assert call(x=None, N=0) == -1                                                 # (in the order of their numbers)


def _model(n, solver, batch=None):
    from volt_amd import gp
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import SingleTaskVariationalGP
    x = torch.arange(1, n + 1, dtype=torch.float32) / 252
    kw = {"batch_shape": torch.Size([batch])} if batch else {}
    lik = VolatilityGaussianLikelihood(param="exp")
    model = SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=lik, use_piv_chol_init=False,
                                    mean_module=gp.ConstantMean(**kw), covar_module=BMKernel(**kw),
                                    learn_inducing_locations=False, use_whitened_var_strat=False, prior_solver=solver)
    return model, lik, x


def test_python_refusals_and_the_sites_stay_out_of_the_state_dict():
    from volt_amd import forecast, ops, train_utils
    from volt_amd._lib import VoltHipError
    from volt_amd.models import MultitaskVariationalGP
    from volt_amd.variational import VariationalELBO
    x = torch.arange(1, 10, dtype=torch.float32) / 252
    prices = torch.ones(10)
    for fn in (train_utils.FitGPCV, train_utils.LearnGPCV):
        for solver in ("dense", "linear"):
            with pytest.raises(ValueError, match='solver="markov"'):
                fn(x, prices, solver=solver, optimizer="natgrad")
        with pytest.raises(ValueError, match="optimizer must be"):
            fn(x, prices, solver="markov", optimizer="newton")
        for bad in (0.0, 1.5, -1.0):
            with pytest.raises(ValueError, match="ng_step"):
                fn(x, prices, solver="markov", optimizer="natgrad", ng_step=bad)
    with pytest.raises(ValueError, match="natgrad"):
        train_utils.FitGPCVMultitask(x, torch.ones(2, 10), solver="markov", optimizer="natgrad")
    assert "natgrad" in train_utils.GPCV_OPTIMIZERS and {"optimizer", "ng_step"} <= set(forecast.GPCV_OPTIONS)
    with pytest.raises(ValueError, match='solver="markov"'):
        forecast._check_gpcv_options({"optimizer": "natgrad"}, False, "dense", 3, None)
    with pytest.raises(ValueError, match="multi-task"):
        forecast._check_gpcv_options({"optimizer": "natgrad"}, "markov", "dense", 3, None)
    assert forecast._check_gpcv_options({"optimizer": "natgrad", "ng_step": 0.5}, False, "markov", 3, None) == \
        {"optimizer": "natgrad", "ng_step": 0.5}
    # every other family, and the multi-task model
    for solver in ("dense", "linear"):
        model, lik, _ = _model(9, solver)
        with pytest.raises(ValueError, match='prior_solver="markov"'):
            VariationalELBO(lik, model, 9).natural_gradient_step(torch.zeros(9))
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    for solver in MultitaskVariationalGP.PRIOR_SOLVERS:
        mt = MultitaskVariationalGP(x, num_tasks=2, covar_module=BMKernel(), prior_solver=solver)
        with pytest.raises(ValueError, match='prior_solver="markov"'):
            VariationalELBO(VolatilityGaussianLikelihood(param="exp"), mt, 18).natural_gradient_step(torch.zeros(9, 2))
    # the Markov model on the CPU: no fallback; its sites are made at first use and never saved
    model, lik, _ = _model(9, "markov")
    before = set(model.state_dict())
    with pytest.raises(VoltHipError):
        VariationalELBO(lik, model, 9).natural_gradient_step(torch.zeros(9))
    dist = model.variational_strategy._variational_distribution
    assert not any("natural" in k for k, _ in dist.named_buffers())
    l1, l2 = dist.natural_sites()
    assert l1.dtype == torch.float64 and tuple(l1.shape) == (1, 9) and not l1.any() and not l2.any()
    assert dist.natural_sites()[0] is l1
    assert set(model.state_dict()) == before
    a = torch.zeros(1, 4)
    with pytest.raises(VoltHipError):
        ops.gpcv_markov_natgrad(torch.arange(1., 5.), torch.tensor([0.2]), a, a, a, a, a, torch.zeros(3), torch.zeros(3),
                                a.double(), a.double())


def test_natgrad_kernel_cross_compiles_without_scratch_or_spills(tmp_path):
    from volt_amd.build import FLAGS, SOURCES, _hipcc
    assert "gpcv_markov_ng.hip" in SOURCES
    src = os.path.join(ROOT, "volt_amd", "csrc", "gpcv_markov_ng.hip")
    r = subprocess.run([_hipcc(), *FLAGS, "-c", src, "-o", str(tmp_path / "gpcv_markov_ng.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = [b for b in r.stderr.split("Function Name: ")[1:] if "gpcv_markov_ng_kernel" in b.split()[0]]
    assert len(blocks) == 9, [b.split()[0] for b in blocks]                       # "exp" and "cv" with K = 1 .. 8
    for b in blocks:
        name = b.split()[0]
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
        assert int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, name
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 32 * 1024, name     # not sized by N
        print(name, "VGPRs", re.search(r" VGPRs: (\d+)", b).group(1), "occupancy",
              re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1), "static LDS",
              re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
    with open(src) as fh:
        assert "atomic" not in fh.read().replace("No atomics", "").replace("no atomics", "")
    from volt_amd import _lib
    _lib.lib()
    lib = os.path.join(ROOT, "volt_amd", "csrc", "libvolt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    for name in ("volt_gpcv_markov_ng_f32", "volt_gpcv_markov_ng_workspace_bytes"):
        assert f" T {name}" in syms
