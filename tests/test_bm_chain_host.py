"""Host checks (no GPU) of the linear-time Brownian-motion solver's mathematics and plumbing.  Two kinds of test:
  * the REFERENCE validated, not the feature: the fp64 restatement of the recurrences (tests/bm_chain_ref.py) against dense fp64
    LAPACK, and its closed-form gradients against torch autograd through the dense definition.  These exercise nothing of
    volt_amd and pass with or without the solver; they are what entitles tests/test_gpu_bm_linear.py to use the restatement.
  * the feature: the lazy prior, BMGP's solver / grid validation and the C entry points' argument checks."""
import numpy as np
import pytest
import torch

import bm_chain_ref as ref

TOL = 1e-10                       # the project's fp64 gate at N <= 1024 (include/volt_hip.h), relative to each quantity's scale
SIZES = (1, 2, 3, 64, 399, 1024)
NOISES = (1e-4, 1e-2, 0.69)
VOLS = np.array([0.2, 0.7])


def _resid(n, seed=0):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.standard_normal((2, n)) * 0.05, axis=1) - 2.0


@pytest.mark.parametrize("n", SIZES)
def test_restatement_matches_dense_lapack(n):
    worst = 0.0
    for gname, x in ref.grids(n).items():
        for s in NOISES:
            s2 = np.array([s, s])
            r = _resid(n)
            out, alpha, info = ref.bm_step_ref(x, VOLS, s2, r)
            dout, dalpha = ref.dense_step(x, VOLS, s2, r)
            assert not info.any()
            err = np.abs(out[:, :6] - dout[:, :6]) / ref.out_scales(dout, n)
            aerr = np.abs(alpha - dalpha).max(1) / np.abs(dalpha).max(1)
            worst = max(worst, err.max(), aerr.max())
            assert err.max() <= TOL, (gname, s, err)
            assert aerr.max() <= TOL, (gname, s, aerr)
    print(f"N = {n}: worst relative error against dense fp64 LAPACK {worst:.2e}")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("H", (1, 20))
def test_multi_rhs_solve_matches_dense_inverse(n, H):
    rng = np.random.default_rng(1)
    for gname, x in ref.grids(n).items():
        for s in NOISES:
            R = rng.standard_normal((2, n, H))
            R[1] = (VOLS[1] * x)[:, None]                                   # the forecasting case: every column of K_t* equal
            X, info = ref.bm_solve_ref(x, VOLS, np.array([s, s]), R)
            assert not info.any()
            for b in range(2):
                want = np.linalg.inv(ref.dense_a(x, VOLS[b], s)) @ R[b]
                assert np.abs(X[b] - want).max() <= TOL * np.abs(want).max(), (gname, s, b)


def test_spd_at_x0_zero_and_info_for_zero_noise():
    x = ref.grids(8)["uniform_zero"]
    out, _, info = ref.bm_step_ref(x, [0.3], [1e-4], np.ones((1, 8)))
    assert info[0] == 0 and np.isfinite(out).all()
    out, _, info = ref.bm_step_ref(x, [0.3], [0.0], np.ones((1, 8)))         # d_0 = v x_0 + s = 0
    assert info[0] == 1 and np.isnan(out[0, 0]) and np.isnan(out[0, 3])
    out, _, info = ref.bm_step_ref(x, [0.3], [1e-2], np.full((1, 8), np.nan))   # a NaN residual is not a pivot failure
    assert info[0] == 0 and np.isnan(out[0, 0]) and np.isfinite(out[0, 3])


@pytest.mark.parametrize("n", (64, 399))
@pytest.mark.parametrize("s", (1e-2, 0.69))
def test_closed_form_gradients_match_autograd(n, s):
    """d mll / d vol and d mll / d sigma2 of BMGP's marginal likelihood (mean -1/2 vol^2 x, K = vol min) from the step's
    scalars and alpha, against torch fp64 autograd through the dense definition."""
    x = ref.grids(n)["irregular_dt"]
    y = _resid(n)[0]
    xt, yt = torch.tensor(x), torch.tensor(y)
    vol = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    s2 = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    A = vol * torch.minimum(xt[:, None], xt[None, :]) + s2 * torch.eye(n, dtype=torch.float64)
    mll = torch.distributions.MultivariateNormal(-0.5 * vol ** 2 * xt, covariance_matrix=A).log_prob(yt) / n
    gv, gs = torch.autograd.grad(mll, (vol, s2))
    v = vol.item()
    out, alpha, _ = ref.bm_step_ref(x, [v], [s], (y + 0.5 * v * v * x)[None])
    d_vol = ref.dvol_ref(out, [v], n)[0] + (alpha[0] / n * (-v * x)).sum()      # + d mll / d mean . d mean / d vol
    assert abs(out[0, 0] - mll.item()) <= 1e-9 * abs(mll.item())
    assert abs(out[0, 1] - gs.item()) <= 1e-8 * max(abs(gs.item()), ref.out_scales(out, n)[0, 1])
    assert abs(d_vol - gv.item()) <= 1e-8 * max(abs(gv.item()), 1.0)


def test_lazy_prior_evaluates_to_the_dense_one():
    from volt_amd.gp import _BrownianPrior, _ScaledDense
    x = torch.tensor(ref.grids(17)["irregular_dt"], dtype=torch.float32)
    base = torch.minimum(x[:, None], x[None, :])
    for scale in (torch.tensor([0.3]), torch.tensor([[0.2], [0.7], [0.5]])):
        lazy, dense = _BrownianPrior(scale, x), _ScaledDense(scale, base)
        assert isinstance(lazy, _ScaledDense)
        assert torch.equal(lazy.evaluate(), dense.evaluate()) and torch.equal(lazy.to_dense(), dense.to_dense())
        assert torch.equal(lazy.detach(), dense.detach()) and lazy.shape == dense.shape == torch.Size((17, 17))


def test_solver_and_grid_validation():
    from volt_amd.gp import GaussianLikelihood
    from volt_amd.models import BMGP
    x = torch.arange(1, 9, dtype=torch.float32) / 252
    y = torch.zeros(8)
    lh = GaussianLikelihood()
    assert BMGP(x, y, lh).solver == "dense" and BMGP(x, y, lh, solver="linear").solver == "linear"
    assert BMGP(x - x[0], y, lh, solver="linear").solver == "linear"          # x_0 = 0 is fine
    with pytest.raises(ValueError, match="solver must be one of"):
        BMGP(x, y, lh, solver="banded")
    with pytest.raises(ValueError, match="not"):
        BMGP(x, y, lh, kernel="fbm", solver="linear")
    with pytest.raises(ValueError, match="1-D"):
        BMGP(x.reshape(-1, 1), y, lh, solver="linear")
    with pytest.raises(ValueError, match=r"x\[0\] >= 0"):
        BMGP(x - 1.0, y, lh, solver="linear")
    with pytest.raises(ValueError, match="strictly increasing"):
        BMGP(torch.cat([x[:4], x[3:7]]), y, lh, solver="linear")
    with pytest.raises(ValueError, match="strictly increasing"):
        BMGP(torch.cat([x[:4], torch.tensor([float("nan")]), x[5:]]), y, lh, solver="linear")
    BMGP(x.reshape(-1, 1) - 1.0, y, lh)                                        # the dense path validates nothing, as before


def test_entry_points_validate_arguments_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    al = lambda b: (b + 255) // 256 * 256
    assert L.volt_bm_workspace_bytes(3, 399, 1) == 2 * al(3 * 399 * 8)
    assert L.volt_bm_workspace_bytes(2, 65536, 20) == al(2 * 65536 * 8) + al(2 * 65536 * 20 * 8)     # O(B N H): 22 MB, no N^2
    assert L.volt_bm_workspace_bytes(0, 4, 1) == 0 and L.volt_bm_workspace_bytes(1, 0, 1) == 0
    for step in (L.volt_bm_step_f32, L.volt_bm_step_f64):
        assert step(None, 1, 1, 1, 1, 1, 1, 256, 1, 8, 1, None) == -1
        assert step(1, 1, 1, None, 1, 1, 1, 256, 1, 8, 1, None) == -4
        assert step(1, 1, 1, 1, 1, None, 1, 256, 1, 8, 1, None) == -6          # alpha is needed with VOLT_WANT_GRAD
        assert step(1, 1, 1, 1, 1, 1, 1, 8, 1, 8, 1, None) == -8               # workspace not 256-byte aligned
        assert step(1, 1, 1, 1, 1, 1, 1, 256, 0, 8, 1, None) == -9
        assert step(1, 1, 1, 1, 1, 1, 1, 256, 1, 0, 1, None) == -10
        assert step(1, 1, 1, 1, 1, 1, 1, 256, 1, 8, 2, None) == -11            # VOLT_WS_INITIALISED means nothing here
    for solve in (L.volt_bm_solve_f32, L.volt_bm_solve_f64):
        assert solve(1, 1, 1, None, 1, 1, 256, 1, 8, 1, None) == -4
        assert solve(1, 1, 1, 1, 1, 1, None, 1, 8, 1, None) == -7
        assert solve(1, 1, 1, 1, 1, 1, 256, 1, 8, 0, None) == -10
