"""Host checks (no GPU) of the O(N^2) GPCV step's mathematics and plumbing.  Two kinds of test:
  * the REFERENCE validated: the fp64 restatement of the column recurrences (tests/gpcv_bm_ref.py) against the dense oracle
    (oracle/gpcv_oracle.py on bm_cov + 1e-3 I, dense inverses for the scalars the oracle does not name).  This is what entitles
    tests/test_gpu_gpcv_bm.py to use the restatement;
  * the feature: prior_solver / solver validation, the lazy prior, the workspace size and the entry's argument checks."""
import math

import numpy as np
import pytest
import torch

import bm_chain_ref as BM
import gpcv_bm_ref as ref
from oracle import gpcv_oracle as GO

TOL = 1e-10                       # relative to each quantity's scale
SIZES = (1, 2, 3, 64, 65, 399)
VOLS = (0.05, 0.2, 0.9)


@pytest.mark.parametrize("n", SIZES)
def test_restatement_matches_dense_oracle(n):
    gh_x, gh_w = GO.gauss_hermite(75)
    ghx, ghw = gh_x.numpy(), (gh_w / math.sqrt(math.pi)).numpy()
    worst = {}
    for x0_zero in (True, False):
        for irregular in (False, True):
            x, m, mu, y, L = ref.problem(n, 1, 11 + n, x0_zero, irregular)
            for v in VOLS:
                r = ref.step_ref(x, [v], m - mu, m, L, y, ghx, ghw, w_ell=1.0 / n, w_kl=1.0 / n)
                assert not r["info"].any()
                # ---- the oracle: ELBO and gradients through the dense definition
                t = lambda a: torch.as_tensor(a, dtype=torch.float64)
                Lt = t(np.nan_to_num(L[0]))
                raw_vol = torch.logit(t([v]))
                val, (gm, gL, gc, gv) = GO.elbo_and_grads(t(m[0]), Lt, t(mu[0, :1]), raw_vol, t(x), t(y[0]))
                K = GO.bm_cov(t(x), t(v))
                terms = GO.elbo_terms(t(m[0]), Lt, t(mu[0, :1]), K, t(y[0]), gh_x, gh_w)
                Ainv = np.linalg.inv(BM.dense_a(x, v, ref.JITTER))
                Gd = Ainv @ np.tril(np.nan_to_num(L[0]))
                beta = Ainv @ (m[0] - mu[0])
                want = np.array([float(terms["ell"]), float(terms["kl"]), float(terms["quad"]), float(terms["logdet_k"]),
                                 float(terms["logdet_s"]), float(terms["trace"]), np.trace(Ainv), (Gd * Gd).sum(), beta @ beta,
                                 float(val)])
                sc = ref.out_scales(want[None], n, 1.0 / n, 1.0 / n)[0]
                err = np.abs(r["out"][0, :10] - want) / sc
                names = ("ell", "kl", "quad", "logdet_k", "logdet_s", "tr_s", "tr_inv", "gg", "bb", "F")
                for k, e in zip(names, err):
                    worst[k] = max(worst.get(k, 0.0), e)
                    assert e <= TOL, (k, x0_zero, irregular, v, e)
                rel = lambda a, w: np.abs(a - w).max() / np.abs(w).max()
                e_m, e_L = rel(r["grad_m"][0], gm.numpy()), rel(r["grad_Lq"][0], np.tril(gL.numpy()))
                e_mu = max(rel(r["grad_mu"][0], beta / n),                                  # every entry: w_kl beta
                           abs(r["grad_mu"][0].sum() - float(gc)) / max(np.abs(r["grad_mu"][0]).sum(), 1e-300))
                e_v = abs(r["dvol"][0] * v * (1 - v) - float(gv)) / (r["dvol_scale"][0] * v * (1 - v))
                for k, e in (("grad_m", e_m), ("grad_Lq", e_L), ("grad_mu", e_mu), ("d/d raw_vol", e_v)):
                    worst[k] = max(worst.get(k, 0.0), e)
                    assert e <= TOL, (k, x0_zero, irregular, v, e)
                assert not np.triu(r["grad_Lq"][0], 1).any()
    print(f"N = {n}: worst error ratios against the dense oracle " + ", ".join(f"{k} {e:.1e}" for k, e in worst.items()))


def test_cv_restatement_matches_the_cv_reference():
    """The "cv" likelihood term of the restatement against tests/gpcv_cv_ref.py (itself checked against the oracle)."""
    import gpcv_cv_ref as CV
    n, Kc = 65, 5
    x, m, mu, y, L = ref.problem(n, 1, 3)
    gh_x, gh_w = GO.gauss_hermite(75)
    raws = CV.draw_raw(Kc, 7)
    abc = torch.stack(CV.constrain(*raws)).numpy()[None]
    e, g, _ = ref.ell_and_grads(m, L, y, gh_x.numpy(), (gh_w / math.sqrt(math.pi)).numpy(), abc)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    want, _ = CV.ell(t(m[0]), t(np.nan_to_num(L[0])), t(y[0]), *CV.constrain(*raws), gh_x, gh_w)
    assert abs(e[0] - float(want)) <= 1e-12 * abs(float(want))
    assert g[2].shape == (1, 3, Kc) and np.isfinite(g[2]).all()


def test_prior_solver_validation_and_lazy_prior():
    from volt_amd import gp
    from volt_amd.gp import _BrownianPrior
    from volt_amd.kernels import BMKernel, FBMKernel
    from volt_amd.models import SingleTaskVariationalGP
    x = torch.arange(1, 9, dtype=torch.float32) / 252
    mk = lambda **kw: SingleTaskVariationalGP(**{**dict(init_points=x.view(-1, 1), covar_module=BMKernel(),
                                                        mean_module=gp.ConstantMean(), learn_inducing_locations=False,
                                                        use_whitened_var_strat=False), **kw})
    assert mk().prior_solver == "dense" and mk(prior_solver="linear").prior_solver == "linear"
    assert mk(init_points=(x - x[0]).view(-1, 1), prior_solver="linear").prior_solver == "linear"     # x_0 = 0 is fine
    with pytest.raises(ValueError, match="prior_solver must be one of"):
        mk(prior_solver="banded")
    with pytest.raises(ValueError, match="BMKernel"):
        mk(covar_module=FBMKernel(), prior_solver="linear")
    with pytest.raises(ValueError, match=r"x\[0\] >= 0"):
        mk(init_points=(x - 1.0).view(-1, 1), prior_solver="linear")
    with pytest.raises(ValueError, match="strictly increasing"):
        mk(init_points=torch.cat([x[:4], x[3:7]]).view(-1, 1), prior_solver="linear")
    model = mk(prior_solver="linear")
    Z = model.variational_strategy.inducing_points
    prior = model.forward(Z)
    lazy = prior.lazy_covariance_matrix
    assert isinstance(lazy, _BrownianPrior) and lazy.shape == torch.Size((8, 8)) and torch.equal(lazy.x, x)
    assert torch.equal(lazy.evaluate(), model.covar_module(Z).evaluate())
    assert not isinstance(mk().forward(Z).lazy_covariance_matrix, _BrownianPrior)                      # the default is unchanged
    with pytest.raises(ValueError, match="inducing grid"):
        model.forward(Z + 1.0)
    batched = mk(covar_module=BMKernel(batch_shape=torch.Size([3])), mean_module=gp.ConstantMean(batch_shape=torch.Size([3])),
                 prior_solver="linear")
    assert batched.forward(Z).lazy_covariance_matrix.scale.shape == (3, 1)


def test_trainer_and_driver_solver_validation():
    import inspect
    from volt_amd import forecast
    from volt_amd.models.Volt import Volt
    from volt_amd.train_utils import FitGPCV, LearnGPCV
    x = torch.arange(12, dtype=torch.float32) / 252
    prices = torch.ones(13)
    for fn in (FitGPCV, LearnGPCV):
        assert inspect.signature(fn).parameters["solver"].default == "dense"
        with pytest.raises(ValueError, match="solver must be one of"):
            fn(x, prices, train_iters=1, solver="banded")
        with pytest.raises(ValueError, match="needs kernel='bm'"):
            fn(x, prices, train_iters=1, kernel="fbm", solver="linear")
    for fn in (forecast.GenerateStockPredictionsBatch, forecast.GenerateWindPredictionsBatch, forecast._forecast_windows,
               forecast._window_pass, Volt.Train):
        assert inspect.signature(fn).parameters["gpcv_solver"].default == "dense"
        assert fn is Volt.Train or inspect.signature(fn).parameters["vol_solver"].default == "dense"


def test_workspace_bytes_and_argument_checks_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    al = lambda b: (b + 255) // 256 * 256
    B, N = 8, 4096
    for Kc in (0, 8):
        got = L.volt_gpcv_bm_workspace_bytes(B, N, Kc)
        tri = 4 * B * N * (N + 1)
        assert tri <= got <= tri + 96 * B * N + 16 * 256, (Kc, got)          # one packed fp64 triangle per series + O(B N)
        want = (L.volt_bm_workspace_bytes(B, N, 1) + al(tri) + al(3 * B * N * 8) + al(B * 4) + al(B * 32) + al(B * N * 4)
                + al(B * N * 16) + al(2 * B * 4) + (al(B * ((N + 3) // 4) * 3 * Kc * 4) if Kc else 0))
        assert got == want
    assert L.volt_gpcv_bm_workspace_bytes(0, 4, 0) == 0 and L.volt_gpcv_bm_workspace_bytes(1, 0, 0) == 0
    assert L.volt_gpcv_bm_workspace_bytes(1, 4, 9) == 0 and L.volt_gpcv_bm_workspace_bytes(1, 4, -1) == 0
    step = L.volt_gpcv_bm_step_f32
    ok = dict(x=1, vol=1, jitter=1e-3, resid=1, m=1, Lq=1, y=1, abc=None, Kc=0, gh_x=1, gh_w=1, Q=75, min_var=1e-6,
              min_scale=1e-3, w_ell=1.0, w_kl=1.0, out=1, grad_m=1, grad_mu=1, grad_Lq=1, grad_abc=None, info=1, workspace=256,
              B=1, N=8, stream=None)
    call = lambda **kw: step(*{**ok, **kw}.values())
    for code, kw in ((-1, dict(x=None)), (-2, dict(vol=None)), (-4, dict(resid=None)), (-5, dict(m=None)), (-6, dict(Lq=None)),
                     (-7, dict(y=None)), (-9, dict(Kc=1)), (-9, dict(abc=1, Kc=0)), (-9, dict(abc=1, Kc=9)),
                     (-10, dict(gh_x=None)), (-11, dict(gh_w=None)), (-12, dict(Q=0)), (-12, dict(Q=1025)), (-17, dict(out=None)),
                     (-18, dict(grad_m=None)), (-19, dict(grad_mu=None)), (-20, dict(grad_Lq=None)), (-21, dict(abc=1, Kc=5)),
                     (-22, dict(info=None)), (-23, dict(workspace=None)), (-23, dict(workspace=8)), (-24, dict(B=0)),
                     (-24, dict(B=65536)), (-25, dict(N=0))):
        assert call(**kw) == code, (code, kw)
