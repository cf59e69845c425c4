"""Host checks (no GPU) of the one-sweep posterior of the Brownian-motion vol forecaster (posterior="sweep", volt_bm_post_*;
DESIGN 4.16).  Two kinds:
  * the REFERENCE validated, not the feature: the restatement of tests/bm_post_ref.py against dense fp64 LAPACK
    (bm_chain_ref.dense_posterior), with three negative controls that must miss the same gate by 10 x;
  * the feature's host side: gp._markov_cov against brute force, constructor / driver validation, the entry points'
    argument codes, the exports, and a cross-compile of the kernel that asserts no scratch and no spills.
The kernel itself and the models run in tests/test_gpu_bm_post.py."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bm_chain_ref as chain
import bm_post_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-10          # of the quantity's scale (max K_** for the covariance, max |r| for the mean): the restatements' gate
SIZES = (1, 2, 3, 64, 65, 399, 1024)
GRIDS = ("uniform_zero", "irregular_zero", "uniform_dt", "irregular_dt")
NOISES = (1e-3, 1e-1, 0.69)
VOLS = (0.05, 0.9)


def _errors(x, v, s, y, xs, **kw):
    """(mean error / max |r|, covariance error / max K_**) of the sweep restatement against dense LAPACK; NaN counts as inf."""
    mean, cov = ref.sweep_posterior_ref(x, v, s, y, xs, **kw)
    dmean, dcov = chain.dense_posterior(x, v, s, y, xs)
    rscale = np.abs(y + 0.5 * v * v * x).max()
    kscale = v * xs.max()
    with np.errstate(all="ignore"):
        em, ec = np.abs(mean - dmean).max() / rscale, np.abs(cov - dcov).max() / kscale
    return (np.inf if np.isnan(em) else em), (np.inf if np.isnan(ec) else ec)


def _cases(n, grid):
    rng = np.random.default_rng(1000 * n + GRIDS.index(grid))
    x = chain.grids(n, rng)[grid]
    xs = ref.test_points(x, 24, rng)
    for s in NOISES:
        for v in VOLS:
            yield x, v, s, ref.series(x, v, s, rng), xs


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", SIZES)
def test_sweep_restatement_matches_dense_lapack(n, grid):
    worst = 0.0
    for x, v, s, y, xs in _cases(n, grid):
        assert len(xs) == 24 and (xs == 0).any() and (xs > x[-1]).any() and (xs == x[-1]).any()
        assert len(np.unique(xs)) < len(xs)                                      # duplicates
        em, ec = _errors(x, v, s, y, xs)
        worst = max(worst, em, ec)
        assert em <= GATE and ec <= GATE, (n, grid, s, v, em, ec)
        _, cov = ref.sweep_posterior_ref(x, v, s, y, xs)
        assert np.array_equal(cov, cov.T)
        zero = xs == 0
        assert not cov[zero].any() and not cov[:, zero].any()                    # f(0) = 0: that row and column are zero
    print(f"sweep restatement N = {n} {grid}: largest error / gate {worst / GATE:.2e}")


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", (64, 65, 399, 1024))
def test_negative_control_dropping_the_c_term_misses(n, grid):
    """The z chains of the test points without c_i z_{i-1} (a sweep that forgets the coupling of T) must miss by >= 10 x."""
    for x, v, s, y, xs in _cases(n, grid):
        em, ec = _errors(x, v, s, y, xs, drop_c=True)
        assert em >= 10 * GATE and ec >= 10 * GATE, (n, grid, s, v, em, ec)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", (3, 64, 65, 399, 1024))
def test_negative_control_next_points_variance_in_g_misses(n, grid):
    """g_j = Sigma_{j,j+1} / Sigma_{j+1,j+1} (the wrong end of the pair) must miss by >= 10 x; the mean does not depend on it."""
    for x, v, s, y, xs in _cases(n, grid):
        _, ec = _errors(x, v, s, y, xs, mode="nextdiag")
        assert ec >= 10 * GATE, (n, grid, s, v, ec)


def test_negative_control_cumulative_product_ratios_underflow():
    """Test points 40 grid steps apart under a small noise: each g_j is ~1e-30, so a cumulative product of 23 of them is 0 and
    a ratio of two of them 0 / 0, while the true covariance of the two DUPLICATED last points is their variance.  The
    exp-of-log-differences form passes the gate on the same case."""
    rng = np.random.default_rng(3)
    x = chain.grids(1024, rng)["uniform_dt"]
    v, s = 0.9, 1e-3
    xs = np.concatenate([x[20:20 + 40 * 23:40], x[900:901]])                   # 24 points, the last one twice
    assert len(xs) == 24 and xs[-1] == xs[-2]
    y = ref.series(x, v, s, rng)
    em, ec = _errors(x, v, s, y, xs)
    assert em <= GATE and ec <= GATE, (em, ec)
    _, bad = _errors(x, v, s, y, xs, mode="cumprod")
    assert bad >= 10 * GATE, bad


def test_forms_restatement_reports_bad_test_points_and_pivots():
    x = chain.grids(9)["uniform_dt"]
    r = np.ones((2, 9))
    for xs, code in (([0.1, 0.05], -2), ([-1.0, 0.2], -1), ([0.0, np.nan, 1.0], -2), ([0.0, np.inf], -2)):
        out, info = ref.post_forms_ref(x, [0.5, 0.5], [0.1, 0.1], r, xs)
        assert (info == code).all() and np.isnan(out).all()
    out, info = ref.post_forms_ref(x, [0.5, 0.5], [0.1, -1.0], r, [0.0, 0.1])
    assert info[0] == 0 and info[1] == 1 and np.isfinite(out[0]).all() and np.isnan(out[1]).all()


# ------------------------------------------------------------------------------------------------ gp._markov_cov
def _random_markov_cov(rng, H, zero_start=False, cut=None):
    """x_0 = e_0, x_{j+1} = a_j x_j + e_{j+1}: cov = L W L' from the explicit transfer matrix (brute force)."""
    a = rng.uniform(0.2, 1.3, size=H - 1)
    if cut is not None:
        a[cut] = 0.0
    w = rng.uniform(0.1, 2.0, size=H)
    if zero_start:
        w[0] = 0.0
    L = np.eye(H)
    for c in range(H):
        for r in range(c + 1, H):
            L[r, c] = L[r - 1, c] * a[r - 1]
    return L @ np.diag(w) @ L.T


@pytest.mark.parametrize("H", (1, 2, 7, 24))
def test_markov_cov_matches_brute_force(H):
    from volt_amd.gp import _markov_cov
    rng = np.random.default_rng(H)
    covs = [_random_markov_cov(rng, H), _random_markov_cov(rng, H, zero_start=True)]
    if H > 3:
        covs.append(_random_markov_cov(rng, H, cut=2))
    C = np.stack(covs)
    diag = np.diagonal(C, axis1=1, axis2=2).copy()
    off = np.concatenate([np.diagonal(C, 1, axis1=1, axis2=2), np.zeros((len(covs), 1))], axis=1)
    got = _markov_cov(torch.tensor(diag), torch.tensor(off))
    assert got.dtype == torch.float64 and got.shape == (len(covs), H, H)
    assert torch.equal(got, got.mT)
    np.testing.assert_allclose(got.numpy(), C, rtol=1e-12, atol=1e-13 * np.abs(C).max())
    for k in range(len(covs)):                                                   # and the numpy restatement agrees with both
        np.testing.assert_allclose(ref.markov_cov_ref(diag[k], off[k]), C[k], rtol=1e-12, atol=1e-13 * np.abs(C).max())


def test_markov_cov_long_weak_chain_does_not_underflow_to_nan():
    from volt_amd.gp import _markov_cov
    H = 40
    diag = torch.ones(H, dtype=torch.float64)
    off = torch.full((H,), 1e-30, dtype=torch.float64)
    off[-2] = 1.0                                                                # the last two points are one point
    got = _markov_cov(diag, off)
    assert torch.isfinite(got).all() and got[-1, -2] == 1.0 and got[0, -1] == 0.0 and abs(got[3, 4] / 1e-30 - 1) < 1e-12


# ------------------------------------------------------------------------------------------------ validation
def test_constructors_validate_posterior():
    from volt_amd.gp import GaussianLikelihood, MultitaskGaussianLikelihood
    from volt_amd.models import BMGP, MultitaskBMGP
    x = torch.arange(1, 9, dtype=torch.float32) / 252
    y = torch.zeros(8)
    assert BMGP(x, y, GaussianLikelihood()).posterior == "solve"
    assert BMGP(x, y, GaussianLikelihood(), solver="linear").posterior == "solve"
    assert BMGP(x, y, GaussianLikelihood(), solver="linear", posterior="sweep").posterior == "sweep"
    with pytest.raises(ValueError, match="posterior"):
        BMGP(x, y, GaussianLikelihood(), solver="linear", posterior="banded")
    with pytest.raises(ValueError, match="solver='linear'"):
        BMGP(x, y, GaussianLikelihood(), posterior="sweep")
    Y = torch.zeros(8, 3)
    lh = lambda: MultitaskGaussianLikelihood(num_tasks=3)
    assert MultitaskBMGP(x, Y, lh()).posterior == "solve"
    assert MultitaskBMGP(x, Y, lh(), solver="linear", posterior="sweep").posterior == "sweep"
    with pytest.raises(ValueError, match="posterior"):
        MultitaskBMGP(x, Y, lh(), solver="linear", posterior="banded")
    with pytest.raises(ValueError, match="solver='linear'"):
        MultitaskBMGP(x, Y, lh(), solver="dense", posterior="sweep")


def test_vol_posterior_passes_through_with_unchanged_defaults():
    from volt_amd import forecast, train_utils
    from volt_amd.models import BMGP, MultitaskBMGP, VoltMagpie, VoltronGP
    from volt_amd.models.Volt import Volt
    from volt_amd.models._base import VolGP
    for fn in (train_utils.TrainVolModel, train_utils.TrainVolModelBatch, train_utils.TrainVolModelMultitask,
               VolGP._init_vol_state, Volt.__init__, VoltMagpie.__init__, VoltronGP.__init__,
               forecast.GenerateStockPredictionsBatch, forecast.GenerateWindPredictionsBatch):
        assert inspect.signature(fn).parameters["vol_posterior"].default == "solve", fn
    for cls in (BMGP, MultitaskBMGP):
        assert inspect.signature(cls.__init__).parameters["posterior"].default == "solve"

    class Stub(VoltronGP):                            # _init_vol_state alone: the constructors fill train_cov on the device
        def __init__(self, multitask, **kw):
            from volt_amd.gp import ExactGP, GaussianLikelihood
            N, T = 12, 3
            x = torch.arange(1, N + 1, dtype=torch.float32) / 252
            ExactGP.__init__(self, x, torch.zeros(T, N), GaussianLikelihood(batch_shape=torch.Size([T])))
            self._vol_prior = lambda *a: None
            self._init_vol_state(x, torch.zeros(T, N), torch.full((T, N), 0.2), multitask, data_solver="linear", **kw)

    for multitask in (False, True):
        m = Stub(multitask, vol_solver="linear", vol_posterior="sweep")
        assert m.vol_posterior == "sweep" and m.vol_model.posterior == "sweep" and m.vol_model.solver == "linear"
        m = Stub(multitask, vol_solver="linear")
        assert m.vol_posterior == "solve" and m.vol_model.posterior == "solve"
        with pytest.raises(ValueError, match="vol_posterior"):
            Stub(multitask, vol_solver="linear", vol_posterior="banded")
        with pytest.raises(ValueError, match="vol_posterior"):
            Stub(multitask, vol_posterior="sweep")                               # the dense vol solver has one posterior
    closes = torch.ones(2, 40)
    with pytest.raises(ValueError, match="posterior"):
        forecast.GenerateStockPredictionsBatch(["a", "b"], closes, ntrain=30, vol_posterior="banded")
    with pytest.raises(ValueError, match="solver='linear'"):
        forecast.GenerateWindPredictionsBatch([0, 1], closes, ntrain=30, forecast_horizon=5, vol_posterior="sweep")


def test_cpu_tensors_raise():
    from volt_amd import ops
    from volt_amd._lib import VoltHipError
    x = torch.arange(1, 10, dtype=torch.float64)
    with pytest.raises(VoltHipError):
        ops.bm_post(x, x[:3], torch.ones(2), torch.ones(2), torch.zeros(2, 9, dtype=torch.float64))


def test_bm_post_entry_points_validate_arguments_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    assert "volt_bm_post_f32" in _lib.EXPORTS and "volt_bm_post_f64" in _lib.EXPORTS
    for post in (L.volt_bm_post_f32, L.volt_bm_post_f64):
        # (x, bsx, xs, vol, sigma2, resid, out, info, B, N, H, stream)
        assert post(None, 8, 1, 1, 1, 1, 1, 1, 1, 8, 4, None) == -1
        assert post(1, 7, 1, 1, 1, 1, 1, 1, 2, 8, 4, None) == -2                 # 0 < bsx < N: rows would overlap
        assert post(1, -8, 1, 1, 1, 1, 1, 1, 2, 8, 4, None) == -2
        assert post(1, 0, None, 1, 1, 1, 1, 1, 1, 8, 4, None) == -3              # bsx = 0 (one shared grid) is legal
        assert post(1, 8, 1, None, 1, 1, 1, 1, 1, 8, 4, None) == -4
        assert post(1, 8, 1, 1, None, 1, 1, 1, 1, 8, 4, None) == -5
        assert post(1, 8, 1, 1, 1, None, 1, 1, 1, 8, 4, None) == -6
        assert post(1, 8, 1, 1, 1, 1, None, 1, 1, 8, 4, None) == -7
        assert post(1, 8, 1, 1, 1, 1, 1, None, 1, 8, 4, None) == -8
        assert post(1, 8, 1, 1, 1, 1, 1, 1, 0, 8, 4, None) == -9
        assert post(1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 4, None) == -10
        assert post(1, 8, 1, 1, 1, 1, 1, 1, 1, 8, 0, None) == -11
        assert post(1, 8, 1, 1, 1, 1, 1, 1, 1, 8, 64 * 65535 + 1, None) == -11   # beyond a grid's second dimension


def test_bm_post_kernel_cross_compiles_without_scratch_or_spills(tmp_path):
    from volt_amd.build import FLAGS, _hipcc
    src = os.path.join(ROOT, "volt_amd", "csrc", "bm.hip")
    r = subprocess.run([_hipcc(), *FLAGS, "-c", src, "-o", str(tmp_path / "bm.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = [b for b in r.stderr.split("Function Name: ")[1:] if "bm_post_kernel" in b.split()[0]]
    assert len(blocks) == 2, [b.split()[0] for b in blocks]                      # the fp32 and the fp64 instantiation
    for b in blocks:
        name = b.split()[0]
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
        assert int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, name
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) == 3 * 64 * 8, name     # the staged tile alone
        print(name, "VGPRs", re.search(r" VGPRs: (\d+)", b).group(1), "occupancy",
              re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
    lib = os.path.join(ROOT, "volt_amd", "csrc", "libvolt_hip.so")
    from volt_amd import _lib
    _lib.lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    assert " T volt_bm_post_f32" in syms and " T volt_bm_post_f64" in syms
