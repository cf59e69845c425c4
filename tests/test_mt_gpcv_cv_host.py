"""The multi-task GPCV "cv" path without a device: the fp64 restatement (tests/mt_gpcv_cv_ref.py) against the dense
NT x NT definition, the batched likelihood on the multi-task latent, both start-ups against the reference's own code
(tests/golden/mt_gpcv_cv.npz), the refusals, the library's argument checks, the cross-compile, and -- for every input
tests/test_gpu_mt_gpcv_cv.py uses -- the fp32 CPU evaluation of the restatement within HALF of each GPU bound, with three
negative controls beyond TEN times them."""
import os
import re
import subprocess
import types
import warnings

import numpy as np
import pytest
import torch

import gpcv_cv_ref as CV
import mt_gpcv_cv_ref as C
import mt_gpcv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "mt_gpcv_cv.npz"))
TAGS = ("n60_t3", "n90_t2")


# ------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("N", [1, 2, 3, 17, 64])
def test_structured_restatement_equals_the_dense_definition(N, T):
    """Value and every gradient -- m, Lx, Lt, c, raw_vol / K, covar_factor, raw_var and the three likelihood arrays -- of
    the Kronecker-structured form against the NT x NT definition with fp64 autograd, to 1e-10 of each quantity's scale."""
    for Kc in (1, 5, 8):
        p, x, y = R.case(N, T, seed=2 + Kc)
        raws = C.draw_raws(T, Kc, seed=5 + N)
        for with_K in (False, True):
            td, gd = C.value_and_grads(C.dense, p, x, y, raws, with_K=with_K)
            ts, gs = C.value_and_grads(C.struct, p, x, y, raws, with_K=with_K)
            errs = {k: abs(float(td[k] - ts[k])) / max(1.0, abs(float(td[k]))) for k in ("F", "ell", "kl")}
            assert set(gd) == set(gs) and set(C.ABC_KEYS) <= set(gd)
            errs.update({"grad_" + k: float((gd[k] - gs[k]).abs().max() / gd[k].abs().max().clamp_min(1e-300)) for k in gd
                         if float(gd[k].abs().max()) > 0 or float(gs[k].abs().max()) > 0})
            assert max(errs.values()) < 1e-10, (Kc, with_K, errs)
        rg = C.raw_grads(p, x, y, raws)                   # the constraints' chain rule: autograd through them == Jacobian x d/d(a,b,c)
        jac = {"raw_a": torch.sigmoid(raws["raw_a"]), "raw_b": 3 * torch.sigmoid(raws["raw_b"]) * (1 - torch.sigmoid(raws["raw_b"])),
               "raw_c": 6 * torch.sigmoid(raws["raw_c"]) * (1 - torch.sigmoid(raws["raw_c"]))}
        for rk, ak in zip(C.RAW_KEYS, C.ABC_KEYS):
            assert float((rg[rk] - jac[rk] * gs[ak]).abs().max()) <= 1e-12 * max(1.0, float(rg[rk].abs().max()))


# --------------------------------------------------------------------------------------------------------- the likelihood
def _latent(N, T, seed):
    """A MultitaskVariationalLatent over a parameter holder, fp64 on the CPU (rsample factor by factor in plain torch: the
    product's goes through the HIP GEMM)."""
    from volt_amd.variational import MultitaskVariationalLatent
    p, x, y = R.case(N, T, seed=seed)
    holder = types.SimpleNamespace(variational_mean=p["m"], variational_covar_root=p["Lx"], variational_task_covar_root=p["Lt"])

    class Latent(MultitaskVariationalLatent):
        def rsample(self, sample_shape=torch.Size(), base_samples=None):
            Lx, Lt = self._roots
            return self.loc + Lx @ base_samples @ Lt.T
    return Latent(holder), p, y


@pytest.mark.parametrize("N,T", [(7, 3), (4, 4), (3, 5)])
def test_batched_likelihood_on_the_multitask_latent(N, T):
    """[T,K] parameters against the latent's [N,T] event: expected_log_prob [N,T] sums to the restatement's ell, marginal
    keeps the [...,N,T] layout with parameter set t on column t -- N != T and N = T (where a wrong axis would go unseen by
    shapes alone, not by values)."""
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.variational import num_gauss_hermite_locs
    Kc = 5
    latent, p, y = _latent(N, T, seed=3)
    raws = C.draw_raws(T, Kc, seed=9)
    lh = VolatilityGaussianLikelihood(K=Kc, batch_shape=torch.Size([T])).double()
    with torch.no_grad():
        for k in C.RAW_KEYS:
            getattr(lh, k).copy_(raws[k])
        with num_gauss_hermite_locs(75):
            elp = lh.expected_log_prob(y, latent)
    want, _ = C.ell(p, y, raws)
    assert tuple(elp.shape) == (N, T)
    assert abs(float(elp.sum() - want)) <= 1e-10 * max(1.0, abs(float(want)))
    # column t alone, against the single-task restatement with task t's parameters
    gx, gw = R.gauss_hermite(75)
    var = R._var(p).clamp_min(R.MIN_VAR)
    for t in range(T):
        f = p["m"][:, t, None] + torch.sqrt(2 * var[:, t, None]) * gx
        s = CV.warp(f, *CV.constrain(*(raws[k][t] for k in C.RAW_KEYS))).clamp(min=R.MIN_SCALE)
        lp = ((-0.5 * (y[:, t, None] / s) ** 2 - s.log() - 0.5 * np.log(2 * np.pi)) * gw).sum(-1)
        assert float((elp[:, t] - lp).abs().max()) <= 1e-10 * max(1.0, float(lp.abs().max()))
    E = torch.randn(10, N, T, dtype=torch.float64, generator=torch.Generator().manual_seed(1))

    class Fixed(type(latent)):
        def rsample(self, sample_shape=torch.Size(), base_samples=None):
            return super().rsample(base_samples=E)
    fixed = Fixed(latent.model)
    with torch.no_grad():
        scale = lh(fixed).scale
    want = C.pred_scale(p, E, raws)                                                  # [T,N], the mean over the draws
    assert tuple(scale.shape) == (10, N, T)
    assert float((scale.mean(0).T - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_forward_on_plain_tensors_keeps_its_rule():
    """[T,K] parameters against samples [...,T,N]: series t of the samples meets parameter set t (unchanged)."""
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    T, N, Kc = 3, 7, 5
    lh = VolatilityGaussianLikelihood(K=Kc, batch_shape=torch.Size([T])).double()
    f = torch.randn(4, T, N, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        got = lh(f).scale
        for t in range(T):
            want = CV.warp(f[:, t], lh.trans_a[t], lh.trans_b[t], lh.trans_c[t]).clamp(min=1e-3)
            assert torch.allclose(got[:, t], want, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------- start-ups and the fixture
def _gold(tag, key):
    return torch.tensor(GOLD[f"{tag}_{key}"])


@pytest.mark.parametrize("param", ["exp", "cv"])
@pytest.mark.parametrize("tag", TAGS)
def test_start_up_restatements_match_the_reference_code(tag, param):
    """mt_gpcv_ref.init_variational ("exp") and mt_gpcv_cv_ref.init_variational_cv against the reference class's own method,
    executed in fp64 over stand-ins (tests/golden/make_golden_mt_gpcv_cv.py)."""
    x, y = _gold(tag, "x"), _gold(tag, "y")
    raws = {k: _gold(tag, k).double() for k in C.RAW_KEYS}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f, S, c = R.init_variational(x, y) if param == "exp" else C.init_variational_cv(x, y, raws)
    mean, root, const = (_gold(tag, f"{param}_f64_{k}") for k in ("mean", "root", "const"))
    assert float((f - mean).abs().max()) <= 1e-12 and float((c - const).abs().max()) <= 1e-12
    cov, want = S @ S.T, root @ root.T
    assert float((cov - want).abs().max() / want.abs().max()) <= 1e-7          # (both take the 1e-8 rung of the jitter ladder)
    if param == "cv":
        assert not (root.tril(-1).abs().sum() == 0) and tuple(mean.shape) == tuple(y.shape)


@pytest.mark.parametrize("param", ["exp", "cv"])
@pytest.mark.parametrize("tag", TAGS)
def test_fixture_fp32_run_stays_inside_the_products_tolerance(tag, param):
    """The reference's own fp32 run against its fp64 run, inside what the product's fp32 start-up is held to on the GPU
    (test_start_up_reference_matches_the_reference_code): mean and constants 1e-5, covariance 2e-3."""
    a = {k: _gold(tag, f"{param}_f32_{k}").double() for k in ("mean", "root", "const")}
    b = {k: _gold(tag, f"{param}_f64_{k}") for k in ("mean", "root", "const")}
    assert float((a["mean"] - b["mean"]).abs().max()) < 1e-5 and float((a["const"] - b["const"]).abs().max()) < 1e-5
    ca, cb = a["root"] @ a["root"].T, b["root"] @ b["root"].T
    assert float((ca - cb).abs().max() / cb.abs().max()) < 2e-3


# -------------------------------------------------------------------------------------------------------------- refusals
def _model(T=3, N=12):
    from volt_amd.kernels import BMKernel
    from volt_amd.models import MultitaskVariationalGP
    x = torch.arange(1, N + 1, dtype=torch.float32) / 252
    return MultitaskVariationalGP(x, T, covar_module=BMKernel()), x


def test_refusals():
    from volt_amd import forecast, ops
    from volt_amd._lib import VoltHipError
    from volt_amd.likelihoods import VolatilityGaussianLikelihood as Lik
    from volt_amd.variational import VariationalELBO
    m, x = _model()
    with pytest.raises(NotImplementedError, match=r"batch_shape=\[num_tasks\]"):      # one warp shared by all tasks: not offered
        VariationalELBO(Lik(), m, 36)
    with pytest.raises(ValueError, match="num_tasks = 3"):
        VariationalELBO(Lik(batch_shape=torch.Size([4])), m, 36)
    with pytest.raises(NotImplementedError, match="1 <= K <= 8"):
        VariationalELBO(Lik(K=9, batch_shape=torch.Size([3])), m, 36)
    elbo = VariationalELBO(Lik(K=8, batch_shape=torch.Size([3])), m, 36)
    with pytest.raises(VoltHipError):                                                 # CPU tensors: no fallback
        elbo(m(x), torch.zeros(12, 3))
    with pytest.raises(VoltHipError):
        ops.gpcv_mt_step(torch.eye(4), torch.zeros(4, 2), torch.zeros(2), torch.eye(4), torch.eye(2), torch.zeros(2),
                         torch.zeros(2), torch.zeros(4, 2), torch.zeros(3), torch.zeros(3), abc=torch.ones(2, 3, 5))
    with pytest.raises(NotImplementedError, match="only works for K = 1"):
        m.initialize_variational_parameters(Lik(K=2, batch_shape=torch.Size([3])), x, y=torch.ones(12, 3))
    with pytest.raises(NotImplementedError, match=r"batch_shape=\[num_tasks\]"):
        m.initialize_variational_parameters(Lik(K=1), x, y=torch.ones(12, 3))
    closes = torch.rand(2, 40) + 1
    with pytest.raises(ValueError, match="unknown keys"):
        forecast.GenerateStockPredictionsBatch(["a", "b"], closes, ntrain=30, gpcv_options={"param": "cv", "lr": 0.1})
    with pytest.raises(ValueError, match="unknown keys"):
        forecast.GenerateWindPredictionsBatch([0, 1], closes, ntrain=30, forecast_horizon=5, n_test_times=1,
                                              multitask_gpcv=True, gpcv_options={"solver": "linear"})
    with pytest.raises(ValueError, match="linear"):
        forecast.GenerateStockPredictionsBatch(["a", "b"], closes, ntrain=30, multitask_gpcv=True, gpcv_solver="linear")
    with pytest.raises(ValueError, match="at most 64"):
        forecast.GenerateStockPredictionsBatch([str(i) for i in range(65)], torch.rand(65, 40) + 1, ntrain=30,
                                               multitask_gpcv=True)


# --------------------------------------------------------------------------------------------- the library without a device
def test_exports_workspace_and_argument_codes():
    from volt_amd import _lib
    L = _lib.lib()
    assert "volt_gpcv_mt_cv_workspace_bytes" in _lib.EXPORTS and "volt_gpcv_mt_cv_step_f32" in _lib.EXPORTS
    al = lambda b: (b + 255) // 256 * 256
    for N, T, dk, Kc in ((300, 4, 0, 5), (300, 4, 1, 1), (17, 64, 0, 8), (4112, 2, 0, 5), (1, 1, 1, 3)):
        base = L.volt_gpcv_mt_workspace_bytes(N, T, dk)
        assert L.volt_gpcv_mt_cv_workspace_bytes(N, T, dk, Kc) == base + al(T * ((N + 15) // 16) * 3 * Kc * 4)
    for bad in ((0, 4, 0, 5), (300, 0, 0, 5), (300, 65, 0, 5), (300, 4, 0, 0), (300, 4, 0, 9)):
        assert L.volt_gpcv_mt_cv_workspace_bytes(*bad) == 0
    # every argument code of the new entry, with null pointers: no launch
    tail = [75, 1e-6, 1e-3, 1.0, 1.0]

    def call(**bad):
        a = dict(K=1, ldk=8, M=1, c=1, Lx=1, Lt=1, cf=1, rv=1, y=1, abc=1, Kc=5, gx=1, gw=1, Q=75, out=1, gM=1, gc=1, gLx=1,
                 gLt=1, gcf=1, grv=1, gK=None, gabc=1, info=1, ws=256, N=8, T=2)
        a.update(bad)
        return L.volt_gpcv_mt_cv_step_f32(a["K"], a["ldk"], 1e-3, a["M"], a["c"], a["Lx"], a["Lt"], a["cf"], a["rv"], a["y"],
                                          a["abc"], a["Kc"], a["gx"], a["gw"], a["Q"], *tail[1:], a["out"], a["gM"], a["gc"],
                                          a["gLx"], a["gLt"], a["gcf"], a["grv"], a["gK"], a["gabc"], a["info"], a["ws"],
                                          a["N"], a["T"], 0, None)
    codes = {"K": -1, "M": -4, "c": -5, "Lx": -6, "Lt": -7, "cf": -8, "rv": -9, "y": -10, "abc": -11, "gx": -13, "gw": -14,
             "out": -20, "gM": -21, "gc": -22, "gLx": -23, "gLt": -24, "gcf": -25, "grv": -26, "gabc": -28, "info": -29,
             "ws": -30}
    for name, code in codes.items():
        assert call(**{name: None}) == code, name
    assert call(ldk=4) == -2 and call(Kc=0) == -12 and call(Kc=9) == -12 and call(Q=0) == -15 and call(Q=1025) == -15
    assert call(ws=100) == -30 and call(N=0) == -31 and call(T=0) == -32 and call(T=65) == -32


def test_exp_workspace_sizes_are_unchanged():
    """volt_gpcv_mt_workspace_bytes is what tests/golden/workspace_bytes.json records (the "cv" partials are appended behind
    it), and the "cv" size is that plus the partials at every recorded (N, T, want_dk)."""
    import json
    from volt_amd import _lib
    L = _lib.lib()
    with open(os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")) as fh:
        gold = json.load(fh)
    g, rows = gold["grid"], gold["full_chip"]["volt_gpcv_mt_workspace_bytes"]
    al = lambda b: (b + 255) // 256 * 256
    for i, N in enumerate(g["N"]):
        for j, T in enumerate(g["T"]):
            for dk in (0, 1):
                assert L.volt_gpcv_mt_workspace_bytes(N, T, dk) == rows[i][j][dk], (N, T, dk)
                assert L.volt_gpcv_mt_cv_workspace_bytes(N, T, dk, 8) == rows[i][j][dk] + al(T * ((N + 15) // 16) * 96)


def test_gpcv_mt_cv_hip_cross_compiles_without_scratch_or_spills(tmp_path):
    """All eight instantiations of mt_gh_cv_kernel for gfx950: no scratch, no SGPR or VGPR spills."""
    from volt_amd.build import FLAGS, SOURCES, _hipcc
    assert "gpcv_mt_cv.hip" in SOURCES
    src = os.path.join(ROOT, "volt_amd", "csrc", "gpcv_mt_cv.hip")
    r = subprocess.run([_hipcc(), *FLAGS, "-c", src, "-o", str(tmp_path / "gpcv_mt_cv.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(kernels) == 8 and all("mt_gh_cv_kernel" in k for k in kernels), kernels
    for what in (r"ScratchSize \[bytes/lane\]", "SGPRs Spill", "VGPRs Spill"):
        vals = [int(v) for v in re.findall(what + r": (\d+)", r.stderr)]
        assert vals == [0] * 8, (what, dict(zip(kernels, vals)))


# ------------------------------------------------------------------------- fp32 attainability and the negative controls
@pytest.mark.parametrize("cs", C.ALL_CASES, ids=lambda c: f"{c.N}x{c.T}-K{c.K}-{c.kernel}-x{c.x0}-Q{c.Q}-{c.clamp}-{c.w_ell}")
def test_fp32_restatement_stays_within_half_of_every_gpu_bound(cs):
    out, g = C.restate_f32(cs)
    r = C.ratios(cs, out, g)
    assert R.over(r, 0.5) == {}, cs


@pytest.mark.parametrize("cs", C.REDUCE_CASES, ids=lambda c: f"{c.N}x{c.T}")
def test_fp32_restatement_of_the_quadrature_part_at_the_reduction_edges(cs):
    c = C.make(cs)
    e, g = C.ell_and_abc_grads(c["p"], c["y"], c["raws"])
    f = lambda d: {k: v.float() for k, v in d.items()}
    e32, g32 = C.ell_and_abc_grads(f(c["p"]), c["y"].float(), f(c["raws"]))
    assert abs(float(e32) - float(e)) <= 0.5 * R.TOL_SCALAR * max(1.0, abs(float(e)))
    for k in C.ABC_KEYS:
        assert float((g32[k].double() - g[k]).abs().max() / g[k].abs().max()) <= 0.5 * C.TOL_ABC, k


CONTROL_CASES = tuple(cs for cs in C.STEP_CASES if cs.T > 1)


@pytest.mark.parametrize("cs", CONTROL_CASES, ids=lambda c: f"{c.N}x{c.T}-K{c.K}-{c.kernel}-x{c.x0}")
def test_negative_controls_next_task_and_dropped_factor(cs):
    """The mistakes this pass can make that the others cannot, at the inputs of the step test (T > 1: at T = 1 there is no
    next task): task t evaluated with the warp of task t + 1 misses ell and the three likelihood gradients, the factor f
    dropped from d/db misses grad_b -- each by more than 10 x the GPU bound."""
    c = C.make(cs)
    terms, grads = C.value_and_grads(C.struct, c["p"], c["x"], c["y"], c["raws"], K=c["K"], wrong="next_task", **c["kw"])
    r = C.ratios(cs, torch.stack([terms[k] for k in R.SCALAR_KEYS]), grads)
    assert r["ell"] > 10 and min(r["grad_" + k] for k in C.ABC_KEYS) > 10, r
    terms, grads = C.value_and_grads(C.struct, c["p"], c["x"], c["y"], c["raws"], K=c["K"], wrong="no_f", **c["kw"])
    r = C.ratios(cs, torch.stack([terms[k] for k in R.SCALAR_KEYS]), grads)
    assert r["grad_lik_b"] > 10 and max(v for k, v in r.items() if k != "grad_lik_b") < 1e-6, r


def test_negative_control_variance_derivative_through_the_floor():
    """At the floored case: letting d/dvar through where the variance is floored misses grad_Lx and grad_Lt by more than
    10 x the GPU bound, and nothing else."""
    cs = C.FLOOR_CASE
    c = C.make(cs)
    terms, grads = C.value_and_grads(C.struct, c["p"], c["x"], c["y"], c["raws"], K=c["K"], wrong="floor", **c["kw"])
    r = C.ratios(cs, torch.stack([terms[k] for k in R.SCALAR_KEYS]), grads)
    assert r["grad_Lx"] > 10 and r["grad_Lt"] > 10, r
    assert max(v for k, v in r.items() if k not in ("grad_Lx", "grad_Lt")) < 1e-6, r
