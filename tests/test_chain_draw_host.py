"""Host checks (no GPU) of the chain draws (posterior="chain", draw="chain"; volt_markov_draw_*, volt_vk_draw_*):
  * the REFERENCE validated, not the feature: the restatement of tests/chain_draw_ref.py against dense fp64 Cholesky on both
    covariance families, its root, the shuffled-points rule, a zero-variance point, and three negative controls that must miss
    the GPU tests' bound by more than 10 x on the GPU tests' inputs;
  * the feature's host side: gp._MarkovCov densifies only on request, option validation, the entry points' argument codes, the
    exports, and a cross-compile of the kernels that asserts no scratch and no spills.
The kernels and the models run in tests/test_gpu_chain_draw.py."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import chain_draw_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-10                      # of the draw's magnitude max |L z|: the restatement's gate and the GPU tests' fp64 bound
SIZES = (1, 2, 3, 20, 64, 65, 300)
RUNGS = (0.0, 1e-6, 1e-2)


def _markov_dense(diag, off):
    from volt_amd.gp import _markov_cov
    return _markov_cov(torch.tensor(diag), torch.tensor(off))


def _dense_draw(C, jitter, mean, z):
    L = torch.linalg.cholesky(C + jitter * torch.eye(C.shape[-1], dtype=torch.float64))
    return mean + (L @ torch.tensor(z).mT).mT.numpy(), L.numpy()


@pytest.mark.parametrize("jitter", RUNGS)
@pytest.mark.parametrize("H", SIZES)
def test_markov_restatement_matches_dense_cholesky(H, jitter):
    rng = np.random.default_rng(H)
    xs, mean, diag, off = ref.bm_posterior_diag_off(50, H, rng)
    if H >= 3:
        assert (xs < 50 / 252.0).any() and (xs > 50 / 252.0).any() and np.isin(xs, (1 + np.arange(50)) / 252.0).any()
    z = rng.standard_normal((7, H))
    C = _markov_dense(diag, off)
    want, L = _dense_draw(C, jitter, mean, z)
    got, info = ref.markov_draw_ref(mean, diag, off, z, jitter)
    assert info == 0
    scale = np.abs(want - mean).max()
    err = np.abs(got - want).max() / scale
    R = ref.chain_root_ref(*ref.markov_cg(diag, off), jitter)
    err_r = np.abs(R @ R.T - (C.numpy() + jitter * np.eye(H))).max() / np.abs(C.numpy()).max()
    print(f"markov H = {H} j = {jitter:g}: draw error / gate {err / GATE:.2e}, R R' error / gate {err_r / GATE:.2e}")
    assert err <= GATE and err_r <= GATE
    assert np.array_equal(R, np.tril(R)) and np.abs(R - L).max() <= GATE * np.abs(L).max()


@pytest.mark.parametrize("jitter", RUNGS)
@pytest.mark.parametrize("H", SIZES)
def test_vk_restatement_matches_dense_cholesky(H, jitter):
    pv, vl, vlr, dx, mean, z = ref.vk_case(1, 5, H, reps=2, seed=H)
    got, info = ref.vk_draw_ref(pv[0], vl[0], vlr[0], dx[0], mean[0], z[0], jitter, reps=2)
    assert not info.any()
    worst = 0.0
    for s in range(5):
        tail = ref.cumtrapz_ref(np.concatenate([[vl[0]], pv[0, s]]), dx[0])
        W = (tail[1:] - tail[0]) + vlr[0]
        C = torch.tensor(ref.min_cov(W))
        want, _ = _dense_draw(C, jitter, mean[0], z[0, 2 * s:2 * s + 2])
        err = np.abs(got[2 * s:2 * s + 2] - want).max() / np.abs(want - mean[0]).max()
        R = ref.chain_root_ref(W, np.ones(H), jitter)
        err_r = np.abs(R @ R.T - (C.numpy() + jitter * np.eye(H))).max() / W.max()
        worst = max(worst, err, err_r)
        assert err <= GATE and err_r <= GATE, (s, err, err_r)
    print(f"vk H = {H} j = {jitter:g}: largest error / gate {worst / GATE:.2e}")


def test_cumtrapz_restatement_is_the_kernels_weights():
    """dx / 2 on the first and the last point, dx between -- what csrc/fill.hip (ops.cumtrapz) and VolKernel.py:4-10 use."""
    y = np.array([2.0, 3.0, 5.0, 7.0])
    np.testing.assert_allclose(ref.cumtrapz_ref(y, 0.5, square=False), np.cumsum([0.5, 1.5, 2.5, 1.75]))
    np.testing.assert_allclose(ref.cumtrapz_ref(y, 0.5, square=True), np.cumsum([1.0, 4.5, 12.5, 12.25]))


@pytest.mark.parametrize("H", (2, 3, 20, 65))
def test_shuffled_points_rule(H):
    """For points in any order the chain draw is mean + P L_sorted P' z: the chain runs over the sorted points, the number at
    the caller's position i drives the point at position i.  Its covariance is the caller's (unsorted) matrix."""
    rng = np.random.default_rng(40 + H)
    _, mean_s, diag, off = ref.bm_posterior_diag_off(50, H, rng)
    order = rng.permutation(H)                     # sorted[k] = caller[order[k]]
    z = rng.standard_normal((3, H))
    y_s, _ = ref.markov_draw_ref(mean_s, diag, off, z[:, order], 0.0)
    y = np.empty_like(y_s)
    y[:, order] = y_s
    C_s = _markov_dense(diag, off).numpy()
    P = np.zeros((H, H))
    P[order, np.arange(H)] = 1.0                   # caller position order[k] <- sorted position k
    L_s = np.linalg.cholesky(C_s)
    mean = np.empty(H)
    mean[order] = mean_s
    want = mean + (P @ L_s @ P.T @ z.T).T
    assert np.abs(y - want).max() <= GATE * np.abs(want - mean).max()
    C = P @ C_s @ P.T                              # the caller's matrix: the same distribution
    Rt = P @ L_s @ P.T
    assert np.abs(Rt @ Rt.T - C).max() <= 1e-12 * np.abs(C).max()


def test_a_zero_variance_point_cuts_the_chain():
    """diag with one zero entry (f(0) = 0): that row and column of the root are zero and nothing couples across them."""
    rng = np.random.default_rng(5)
    _, mean, diag, off = ref.bm_posterior_diag_off(50, 9, rng)
    diag[4] = off[3] = 0.0                         # (a point of zero variance has zero covariance with its neighbours)
    c, g = ref.markov_cg(diag, off)
    assert g[3] == 0.0 and g[4] == 0.0
    R = ref.chain_root_ref(c, g, 1e-300)           # (the pivot of the zero point is 0: any positive rung passes it)
    assert not R[4, :4].any() and abs(R[4, 4]) < 1e-100 and not R[5:, :5].any()
    C = _markov_dense(diag, off).numpy()
    assert not C[4].any() and not C[:, 4].any() and not C[5:, :4].any()
    assert np.abs(R @ R.T - C).max() <= GATE * np.abs(C).max()
    _, info = ref.markov_draw_ref(mean, diag, off, np.zeros((1, 9)), 0.0)
    assert info == 5                               # at rung 0 it is a failed pivot, as in the dense factorisation


# ------------------------------------------------------------------------------------------------ negative controls
GPU_SHAPES = [(3, 65, H) for H in (2, 3, 4, 5, 63, 64, 65, 300, 1025)] + [(1, 5, 5), (3, 130, 65)]


def _deviation(got, want, mean):
    """Of the draw's magnitude; a control that fails a pivot (NaN) misses by inf."""
    assert np.isfinite(want).all()
    d = np.abs(got - want).max() / np.abs(want - mean).max()
    return np.inf if np.isnan(d) else d


@pytest.mark.parametrize("G,S,H", GPU_SHAPES)
def test_negative_control_g_dropped_from_m_misses(G, S, H):
    mean, diag, off, z = ref.markov_case(G, S, H)
    for g in range(G):
        want, _ = ref.markov_draw_ref(mean[g], diag[g], off[g], z[g], 1e-6)
        got, _ = ref.markov_draw_ref(mean[g], diag[g], off[g], z[g], 1e-6, drop_g_from_m=True)
        assert _deviation(got, want, mean[g][None]) > 10 * GATE, (g, H)


@pytest.mark.parametrize("G,S,H", GPU_SHAPES)
def test_negative_control_d_in_place_of_e_over_d_misses(G, S, H):
    mean, diag, off, z = ref.markov_case(G, S, H)
    pv, vl, vlr, dx, vmean, vz = ref.vk_case(G, S, H)
    for g in range(G):
        want, _ = ref.markov_draw_ref(mean[g], diag[g], off[g], z[g], 1e-6)
        got, _ = ref.markov_draw_ref(mean[g], diag[g], off[g], z[g], 1e-6, d_for_r=True)
        assert _deviation(got, want, mean[g][None]) > 10 * GATE, (g, H)
        want, _ = ref.vk_draw_ref(pv[g], vl[g], vlr[g], dx[g], vmean[g], vz[g], 1e-6)
        got, _ = ref.vk_draw_ref(pv[g], vl[g], vlr[g], dx[g], vmean[g], vz[g], 1e-6, d_for_r=True)
        assert _deviation(got, want, vmean[g][None]) > 10 * GATE, (g, H)


@pytest.mark.parametrize("G,S,H", [(3, 65, 1)] + GPU_SHAPES)
def test_negative_control_last_weight_not_halved_misses(G, S, H):
    pv, vl, vlr, dx, mean, z = ref.vk_case(G, S, H)
    for g in range(G):
        want, _ = ref.vk_draw_ref(pv[g], vl[g], vlr[g], dx[g], mean[g], z[g], 0.0)
        got, _ = ref.vk_draw_ref(pv[g], vl[g], vlr[g], dx[g], mean[g], z[g], 0.0, halve_last=False)
        assert _deviation(got, want, mean[g][None]) > 10 * GATE, (g, H)


# ------------------------------------------------------------------------------------------------ the feature's host side
def test_markov_cov_is_densified_only_on_request(monkeypatch):
    from volt_amd import gp
    calls, real = [], gp._markov_cov

    def spy(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(gp, "_markov_cov", spy)
    rng = np.random.default_rng(2)
    _, mean, diag, off = ref.bm_posterior_diag_off(50, 6, rng)
    order = torch.tensor([3, 0, 5, 1, 4, 2])
    lazy = gp._MarkovCov(torch.tensor(diag), torch.tensor(off), order, dtype=torch.float32)
    post = gp.MultivariateNormal(torch.tensor(mean, dtype=torch.float32), lazy)
    assert post.lazy_covariance_matrix is lazy and tuple(lazy.shape) == (6, 6) and post.mean.shape == (6,) and not calls
    cov = post.covariance_matrix
    assert len(calls) == 1 and cov.dtype == torch.float32 and tuple(cov.shape) == (6, 6)
    want = torch.empty(6, 6, dtype=torch.float64)
    want[order.unsqueeze(-1), order.unsqueeze(0)] = real(torch.tensor(diag), torch.tensor(off))
    assert torch.equal(cov, want.float())
    assert torch.equal(post.variance, torch.diagonal(want.float())) and len(calls) == 2
    scaled = gp._MarkovCov(torch.tensor(np.stack([diag, diag])), torch.tensor(np.stack([off, off])), None,
                           scale=torch.tensor([1.0, 2.5], dtype=torch.float64), dtype=torch.float32)
    mt = gp.MultitaskMultivariateNormal(torch.zeros(6, 2), blocks=(torch.eye(2), scaled))
    assert len(calls) == 2
    var = mt.variance
    assert len(calls) == 3 and torch.allclose(var[:, 1].double(), 2.5 * torch.tensor(diag), rtol=1e-6)
    assert tuple(mt.covariance_matrix.shape) == (12, 12) and len(calls) == 4


def test_option_validation():
    from volt_amd import forecast, rollout_utils
    from volt_amd.gp import GaussianLikelihood, MultitaskGaussianLikelihood
    from volt_amd.models import BMGP, MultitaskBMGP, VoltMagpie, VoltronGP
    from volt_amd.models.Volt import Volt
    from volt_amd.models._base import VolGP
    x = torch.arange(1, 9, dtype=torch.float32) / 252
    assert "chain" in BMGP.POSTERIORS and MultitaskBMGP.POSTERIORS == BMGP.POSTERIORS
    assert BMGP(x, torch.zeros(8), GaussianLikelihood(), solver="linear", posterior="chain").posterior == "chain"
    lh = MultitaskGaussianLikelihood(num_tasks=3)
    assert MultitaskBMGP(x, torch.zeros(8, 3), lh, solver="linear", posterior="chain").posterior == "chain"
    with pytest.raises(ValueError, match="solver='linear'"):
        BMGP(x, torch.zeros(8), GaussianLikelihood(), posterior="chain")
    with pytest.raises(ValueError, match="solver='linear'"):
        MultitaskBMGP(x, torch.zeros(8, 3), MultitaskGaussianLikelihood(num_tasks=3), posterior="chain")
    for fn in (VolGP._init_vol_state, Volt.__init__, VoltMagpie.__init__, VoltronGP.__init__,
               forecast.GenerateStockPredictionsBatch, forecast.GenerateWindPredictionsBatch, forecast._window_pass):
        assert inspect.signature(fn).parameters["predict_draw"].default == "factor", fn
    for fn in (rollout_utils._linear_draw, rollout_utils._posterior_draw_linear, forecast._standard_mean_prediction,
               forecast._standard_mean_prediction_linear):
        assert inspect.signature(fn).parameters["draw"].default == "factor", fn
    for fn in (rollout_utils.GeneratePrediction, rollout_utils.Rollouts):
        assert inspect.signature(fn).parameters["draw"].default is None, fn
    assert rollout_utils._resolve_draw(None, "dense") == "factor" and rollout_utils._resolve_draw("chain", "linear") == "chain"
    with pytest.raises(ValueError, match="draw must be"):
        rollout_utils._resolve_draw("banded", "linear")
    with pytest.raises(ValueError, match="solver='linear'"):
        rollout_utils._resolve_draw("chain", "dense")
    closes = torch.ones(2, 40)
    with pytest.raises(ValueError, match="solver='linear'"):
        forecast.GenerateStockPredictionsBatch(["a", "b"], closes, ntrain=30, predict_draw="chain")
    with pytest.raises(ValueError, match="draw must be"):
        forecast.GenerateWindPredictionsBatch([0, 1], closes, ntrain=30, forecast_horizon=5, predict_solver="linear",
                                              predict_draw="banded")
    with pytest.raises(ValueError, match="posterior"):
        forecast.GenerateStockPredictionsBatch(["a", "b"], closes, ntrain=30, vol_posterior="chain")     # needs vol_solver="linear"

    class Stub(VoltronGP):                            # _init_vol_state alone: the constructors fill train_cov on the device
        def __init__(self, **kw):
            from volt_amd.gp import ExactGP
            xx = torch.arange(1, 13, dtype=torch.float32) / 252
            ExactGP.__init__(self, xx, torch.zeros(3, 12), GaussianLikelihood(batch_shape=torch.Size([3])))
            self._vol_prior = lambda *a: None
            self._init_vol_state(xx, torch.zeros(3, 12), torch.full((3, 12), 0.2), False, data_solver="linear", **kw)

    m = Stub(vol_solver="linear", vol_posterior="chain", predict_solver="linear", predict_draw="chain")
    assert m.vol_model.posterior == "chain" and m.predict_draw == "chain"
    assert Stub().predict_draw == "factor"
    with pytest.raises(ValueError, match="solver='linear'"):
        Stub(predict_draw="chain")


def test_cpu_tensors_raise():
    from volt_amd import ops
    from volt_amd._lib import VoltHipError
    a = torch.ones(1, 4, dtype=torch.float64)
    with pytest.raises(VoltHipError):
        ops.markov_draw(a, a, a, torch.zeros(1, 2, 4))
    with pytest.raises(VoltHipError):
        ops.vk_draw(torch.ones(1, 2, 4), 0.2, 1e-4, 1 / 252, a, torch.zeros(1, 2, 4))


def test_entry_points_validate_arguments_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    for name in ("volt_markov_draw_f32", "volt_markov_draw_f64", "volt_vk_draw_f32", "volt_vk_draw_f64"):
        assert name in _lib.EXPORTS
    for draw in (L.volt_markov_draw_f32, L.volt_markov_draw_f64):
        # (mean, diag, off, z, jitter, out, info, G, S, H, flags, stream)
        for k in range(7):
            ptrs = [1] * 7
            ptrs[k] = None
            assert draw(*ptrs, 1, 2, 4, 0, None) == -(k + 1)
        assert draw(*[1] * 7, 0, 2, 4, 0, None) == -8
        assert draw(*[1] * 7, 1, 0, 4, 0, None) == -9
        assert draw(*[1] * 7, 1, 65535 * 1024 + 1, 4, 0, None) == -9              # beyond a grid's second dimension
        assert draw(*[1] * 7, 1, 2, 0, 0, None) == -10
        assert draw(*[1] * 7, 1, 2, 4, 2, None) == -11                            # an unknown flag bit
    assert "volt_markov_mix_f32" in _lib.EXPORTS
    mix = L.volt_markov_mix_f32                                                 # (lz, V, mean, out, T, S, n, stream)
    for k in range(4):
        ptrs = [1] * 4
        ptrs[k] = None
        assert mix(*ptrs, 3, 5, 7, None) == -(k + 1)
    assert mix(1, 1, 1, 1, 0, 5, 7, None) == -5
    assert mix(1, 1, 1, 1, 65, 5, 7, None) == -5                                # beyond the Kronecker path's 64 tasks
    assert mix(1, 1, 1, 1, 3, 0, 7, None) == -6
    assert mix(1, 1, 1, 1, 64, 2 ** 31 - 1, 2 ** 31 - 1, None) == -6           # more blocks than a grid holds
    assert mix(1, 1, 1, 1, 3, 5, 0, None) == -7
    for draw in (L.volt_vk_draw_f32, L.volt_vk_draw_f64):
        # (pred_vol, vol_last, vlr, dx, mean, z, jitter, out, info, G, S, H, reps, stream)
        for k in range(9):
            ptrs = [1] * 9
            ptrs[k] = None
            assert draw(*ptrs, 1, 2, 4, 1, None) == -(k + 1)
        assert draw(*[1] * 9, 0, 2, 4, 1, None) == -10
        assert draw(*[1] * 9, 1, 0, 4, 1, None) == -11
        assert draw(*[1] * 9, 1, 2, 0, 1, None) == -12
        assert draw(*[1] * 9, 1, 2, 4, 0, None) == -13
        assert draw(*[1] * 9, 2 ** 31 - 1, 2 ** 31 - 1, 4, 64, None) == -13       # more blocks than a grid holds


def test_chain_draw_kernels_cross_compile_without_scratch_or_spills(tmp_path):
    from volt_amd.build import FLAGS, SOURCES, _hipcc
    assert "chain_draw.hip" in SOURCES
    src = os.path.join(ROOT, "volt_amd", "csrc", "chain_draw.hip")
    r = subprocess.run([_hipcc(), *FLAGS, "-c", src, "-o", str(tmp_path / "chain_draw.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel in ("markov_draw_kernel", "vk_draw_kernel"):
        blocks = [b for b in r.stderr.split("Function Name: ")[1:] if kernel in b.split()[0]]
        assert len(blocks) == 4, [b.split()[0] for b in blocks]                  # fp32 / fp64 x (16-byte groups / single elements)
        for b in blocks:
            name = b.split()[0]
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
            assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
            assert int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, name
            print(name, "VGPRs", re.search(r" VGPRs: (\d+)", b).group(1), "occupancy",
                  re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1), "static LDS",
                  re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
    with open(src) as fh:
        text = fh.read()
    assert "asm" not in text and "atomic" not in text.replace("no atomics", "")
    lib = os.path.join(ROOT, "volt_amd", "csrc", "libvolt_hip.so")
    from volt_amd import _lib
    _lib.lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    for name in ("volt_markov_draw_f32", "volt_markov_draw_f64", "volt_vk_draw_f32", "volt_vk_draw_f64", "volt_markov_mix_f32"):
        assert f" T {name}" in syms
