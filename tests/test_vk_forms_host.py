"""Host checks (no GPU) of the linear-time forecast path (predict_solver="linear", volt_vk_forms_*).  Two kinds:
  * the REFERENCE validated, not the feature: the restatements of tests/vk_forms_ref.py against dense fp64 LAPACK, the closed
    form and the project's fp64 oracle, plus the negative controls that show the GPU tests' bounds can tell a wrong chain from
    a right one.  These pass with or without the feature; they are what entitles tests/test_gpu_predict_linear.py to use the
    restatements.
  * the feature: predict_solver / solver validation, the C entry points' argument checks, _lib.EXPORTS, and the cross-compile of
    csrc/bm.hip for gfx950 without scratch or spills."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import vk_chain_ref as vk
import vk_forms_ref as ref
from oracle import volt_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10                       # the project's bound for a restatement against dense fp64, of each quantity's scale
SIZES = (1, 2, 3, 64, 65, 399, 1024)
# Dense LAPACK's own error grows with cond(K + j I).  It is measured per case without the code under test -- the same four
# numbers by Cholesky and by LU, their disagreement (vk_forms_ref.dense_forms) -- and a case is admitted when the reference
# holds ADMIT of the bound itself (the idea of rollout_cases.SHARED_CONDITION); the test prints which cases that leaves out.
ADMIT = 0.5


@pytest.mark.parametrize("n", SIZES)
def test_two_chain_sweep_matches_dense_lapack(n):
    worst, left_out = 0.0, []
    for fi, family in enumerate(vk.FAMILIES):
        rng = np.random.default_rng(100 * n + fi)
        V = vk.int_vol(vk.vol_path(family, n, rng))
        assert (np.diff(V) >= 0).all() and V[0] > 0
        if family == "flat_zero" and n >= 64:
            assert vk.zero_increments(V) >= 10                                 # zero increments of V are really there (j > 0)
        r = vk.resid(1, n, rng)
        for j in ref.JITTERS:
            out, info = ref.forms_ref(V, j, r)
            assert not info.any()
            want, own = ref.dense_forms(V, j, r[0])
            scale = ref.forms_scales(V, r, out)[0]
            if (own / scale).max() > ADMIT * TOL:
                left_out.append((family, j, f"LAPACK's own {(own / scale).max():.1e}"))
                continue
            err = np.abs(out[0] - want) / scale
            worst = max(worst, err.max())
            assert err.max() <= TOL, (family, j, err)
    print(f"N = {n}: worst error / scale against dense fp64 LAPACK {worst:.2e}; left out for conditioning: {left_out}")
    assert n >= 1024 or not left_out                                           # only the largest size may lose cases
    assert len(left_out) < 9                                                   # and never all of them


@pytest.mark.parametrize("n", SIZES)
def test_at_zero_jitter_the_forms_are_the_closed_form(n):
    """j = 0: c_i = 0 and d_i = delta_i, so rho = sum delta_i = V[N-1] and tau = sum (D r)_i = r[N-1].  On a grid whose values
    are multiples of 2^-20 below 2^6 (and a residual likewise) every operation of the chain is exact: equality.  On the vol-path
    families the two sums round: N eps64 of the scale."""
    rng = np.random.default_rng(n)
    V = np.cumsum(rng.integers(1, 9, n)) * 2.0 ** -10
    r = rng.integers(-64, 64, (1, n)) * 2.0 ** -6
    out, info = ref.forms_ref(V, 0.0, r)
    assert not info.any() and out[0, 0] == V[-1] and out[0, 1] == r[0, -1]
    for fi, family in enumerate(("smooth", "lognormal")):
        rng = np.random.default_rng(100 * n + fi)
        V = vk.int_vol(vk.vol_path(family, n, rng))
        assert (np.diff(V) > 0).all()
        r = vk.resid(1, n, rng)
        out, info = ref.forms_ref(V, 0.0, r)
        assert not info.any()
        assert abs(out[0, 0] - V[-1]) <= n * 2.0 ** -52 * V[-1]
        assert abs(out[0, 1] - r[0, -1]) <= n * 2.0 ** -52 * np.abs(r).max()


@pytest.mark.parametrize("n,i", [(2, 1), (64, 17), (399, 398), (399, 200)])
def test_a_flat_step_fails_at_zero_jitter_and_succeeds_on_the_first_rung(n, i):
    rng = np.random.default_rng(3 * n + i)
    V = vk.int_vol(vk.vol_path("smooth", n, rng))
    V[i] = V[i - 1]                                                            # ONE exactly flat step: delta_i = 0
    r = vk.resid(1, n, rng)
    out, info = ref.forms_ref(V, 0.0, r)
    assert info.tolist() == [i + 1] and np.isnan(out).all()
    for j in (1e-8, 1e-6, 1e-4):                                               # the first rungs of fp64 input, fp32 input, the callers' 1e-4
        out, used = ref.safe_forms_ref(V, r, j)
        assert used == j
        want, own = ref.dense_forms(V, j, r[0])
        scale = ref.forms_scales(V, r, out)[0]
        assert (np.abs(out[0] - want) / scale <= TOL + 2 * own / scale).all(), (j, out[0], want, own)   # (cond ~ 1e9 at j = 1e-8)


def _histories(N, T, S, per_sample, rng):
    x = (np.arange(N) / 252.).astype(np.float32)
    test_x = ((np.arange(T) / 252.).astype(np.float32) + x[-1] + x[1]).astype(np.float32)
    shape = (S, N) if per_sample else (N,)
    y = (2.3 + np.cumsum(0.012 * rng.standard_normal(shape), -1)).astype(np.float32)
    lv = (np.log(0.2) + np.cumsum(0.05 * rng.standard_normal(shape), -1)).astype(np.float32)
    pv = np.exp(np.log(0.2) + np.cumsum(0.05 * rng.standard_normal((S, T)), -1)).astype(np.float32)
    z = rng.standard_normal((S, T, 1)).astype(np.float32)
    tx = np.repeat(x[None], S, 0) if per_sample else x
    return tx, y, lv, test_x, pv, z


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per_sample"])
@pytest.mark.parametrize("theta", [None, 0.3], ids=["plain", "theta"])
@pytest.mark.parametrize("N", [3, 64, 140])
@pytest.mark.parametrize("T", [1, 2, 24])
def test_linear_draw_restatement_matches_the_fp64_oracle(N, T, theta, per_sample):
    """draw_ref against oracle.generate_prediction(dtype=float64) on identical draws: 1e-9, the bound tests/rollout_ref.py
    holds against the oracle."""
    rng = np.random.default_rng(1000 * N + 10 * T + per_sample)
    tx, y, lv, test_x, pv, z = _histories(N, T, 4, per_sample, rng)
    kw = dict(latent_mean=None if theta is None else 2.25, theta=0.5 if theta is None else theta)
    want = vo.generate_prediction(tx, y, lv, test_x, pv, z, ref.linear_mean, dtype=np.float64, **kw)
    got = ref.draw_ref(tx, y, lv, test_x, pv, z, ref.linear_mean, **kw)
    err = np.abs(got - want).max()
    print(f"N = {N} T = {T} theta = {theta} per-sample = {per_sample}: max |draw_ref - oracle| = {err:.2e}")
    assert err <= 1e-9


def test_flat_step_draw_restatement_matches_the_conditional_at_its_rung():
    """The crafted case of the GPU test: vol[i] = 0 makes V[i] = V[i-1] exactly; the chain reports pivot i, the ladder's first
    rung (1e-4, GeneratePrediction's jitter) succeeds, and draw_ref equals the dense fp64 conditional at that rung to 1e-9."""
    N, T, S, i = ref.FLAT
    x, y, vol, test_x, pv, z, want = ref.flat_case()
    full_vol = np.concatenate([vol.astype(np.float64), pv[0]])
    V = vo.cumtrapz(full_vol * full_vol, np.concatenate([x, test_x]).astype(np.float64))
    assert V[i] == V[i - 1] and (np.diff(np.delete(V, i)) > 0).all()
    r = (y.astype(np.float64) - ref.linear_mean(x))[None]
    _, info = ref.forms_ref(V[:N], 0.0, r)
    assert info.tolist() == [i + 1]
    assert ref.safe_forms_ref(V[:N], r, 1e-4)[1] == 1e-4
    with np.errstate(divide="ignore"):
        got = ref.draw_ref(x, y, np.log(vol.astype(np.float64)), test_x, pv, z, ref.linear_mean)
    print(f"flat step: max |draw_ref - dense conditional at the rung| = {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() <= 1e-9


def test_train_block_of_the_stacked_path_does_not_depend_on_the_test_vols():
    rng = np.random.default_rng(0)
    x = (np.arange(50) / 252.).astype(np.float32)
    v = (0.2 * np.exp(0.3 * rng.standard_normal(50))).astype(np.float32)
    a, b = v.copy(), v.copy()
    b[40:] *= 3.0
    assert np.array_equal(vo.cumtrapz(a * a, x)[:40], vo.cumtrapz(b * b, x)[:40])


# ------------------------------------------------------------------------------------------------ negative controls
def test_dropping_the_second_chains_c_term_misses_the_gpu_bound():
    """At the inputs of the GPU test of ops.vk_forms (vk_chain_ref.mixed_case, jitter = the series' noise level) a D V chain
    without its c_i z_{i-1} term misses rho and tau by more than 10 x that test's bound (1e-10 of scale) in every series."""
    for n in (31, 399):
        V, s2, r = vk.mixed_case(6, n)
        good, _ = ref.forms_ref(V, s2, r)
        bad, _ = ref.forms_ref(V, s2, r, drop_c=True)
        miss = np.abs(bad - good) / ref.forms_scales(V, r, good)
        print(f"N = {n}: a chain without c_i misses rho by {miss[:, 0].min():.1e} .. and tau by {miss[:, 1].min():.1e} .. of scale")
        assert (miss[:, :2] > 10 * 1e-10).all(), miss
        assert (miss[:, 2:] == 0).all()                                        # the r chain and the pivots are untouched


@pytest.mark.parametrize("N,T,S", ref.DRAW_SHAPES)
def test_train_only_cumtrapz_misses_the_gpu_bound(N, T, S):
    """At the inputs of the GPU test of the draw, conditioning on the CumTrapz of the train vols alone (last TRAIN weight halved)
    moves the first predictive variance by dx vol^2 / 2.  Against the fp64 oracle that is more than 10 x the restatement's 1e-9
    and more than 10 x 2^-23 |ref|, the floor of the GPU test's comparative criterion, at the worst output (a draw with a small
    first z hides it on its own path: the statistic is the one a test fails on, the maximum); the GPU test repeats the
    control against its full criterion (dense fp32 error + 2^-23 |ref|).  It is NOT 10 x the absolute 2e-3 of README row a7 --
    at vol ~ 0.2 the miss is ~ 1e-3 -- which is why the GPU test's criterion is the comparative one."""
    x, y, vol, test_x, pv, z, want = ref.draw_case(N, T, S)
    good = ref.draw_ref(x, y, np.log(vol.astype(np.float64)), test_x, pv, z, ref.linear_mean)
    bad = ref.draw_ref(x, y, np.log(vol.astype(np.float64)), test_x, pv, z, ref.linear_mean, train_only=True)
    assert np.abs(good - want).max() <= 1e-9
    miss = np.abs(bad - want).max(1)
    print(f"N = {N} T = {T}: train-only CumTrapz misses the oracle by {miss.min():.2e} .. {miss.max():.2e} per path")
    assert miss.max() > 10 * 2.0 ** -23 * np.abs(want).max() and miss.max() > 10 * 1e-9


# ------------------------------------------------------------------------------------------------ the feature's interface
def test_predict_solver_validation():
    from volt_amd import rollout_engine, rollout_utils
    from volt_amd.forecast import (GenerateStockPredictionsBatch, GenerateWindPredictionsBatch, _forecast_windows,
                                   _standard_mean_prediction, _window_pass)
    from volt_amd.gp import GaussianLikelihood
    from volt_amd.models import VoltMagpie, VoltronGP
    from volt_amd.models.Volt import Volt
    x = torch.arange(12, dtype=torch.float32) / 252
    y = torch.zeros(12)
    vol = torch.full((12,), 0.2)
    with pytest.raises(ValueError, match="predict_solver must be one of"):
        VoltMagpie(x, y, GaussianLikelihood(), vol, k=3, predict_solver="banded")
    with pytest.raises(ValueError, match="predict_solver must be one of"):
        VoltronGP(x, y, GaussianLikelihood(), vol, predict_solver="banded")
    with pytest.raises(ValueError, match="predict_solver must be one of"):
        Volt(torch.arange(13, dtype=torch.float32) / 252, torch.zeros(13), vol_path=vol, predict_solver="banded")
    for cls in (VoltMagpie, VoltronGP, Volt):
        p = inspect.signature(cls.__init__).parameters["predict_solver"]
        assert p.default == "dense" and p.kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (_window_pass, _forecast_windows, GenerateStockPredictionsBatch, GenerateWindPredictionsBatch):
        assert inspect.signature(fn).parameters["predict_solver"].default == "dense"
    for fn in (rollout_utils.GeneratePrediction, rollout_utils.Rollouts):
        p = inspect.signature(fn).parameters["solver"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (rollout_engine.train_block_terms, rollout_engine.rollout_series, rollout_engine.rollouts_bordered):
        assert inspect.signature(fn).parameters["solve"].default == "factor"  # no default changed
    assert inspect.signature(_standard_mean_prediction).parameters["solver"].default == "dense"
    import types
    m = types.SimpleNamespace(predict_solver="linear")                        # (a model needs the device: the GPU tests build them)
    assert rollout_utils._resolve_solver(None, m) == "linear" and rollout_utils._resolve_solver("dense", m) == "dense"
    assert rollout_utils._resolve_solver(None, object()) == "dense"
    with pytest.raises(ValueError, match="solver must be one of"):
        rollout_utils._resolve_solver("banded", m)
    with pytest.raises(ValueError, match="solver must be one of"):
        rollout_utils.Rollouts(x, y.exp(), x[:2], m, nsample=2, solver="banded")
    with pytest.raises(ValueError, match="unknown train-block solve"):
        rollout_engine.train_block_terms(torch.ones(1, 4), torch.ones(1, 4), "banded")


def test_cpu_tensors_raise():
    from volt_amd import gp, ops, rollout_engine
    from volt_amd._lib import VoltHipError
    V, r = torch.rand(2, 9).cumsum(-1), torch.zeros(2, 9)
    with pytest.raises(VoltHipError):
        ops.vk_forms(V, 0.0, r)
    with pytest.raises(VoltHipError):
        gp._safe_forms(V, r, 1e-4)
    with pytest.raises(VoltHipError):
        rollout_engine.train_block_terms(V, r, "chain")


def test_vk_forms_entry_points_validate_arguments_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    assert "volt_vk_forms_f32" in _lib.EXPORTS and "volt_vk_forms_f64" in _lib.EXPORTS
    for forms in (L.volt_vk_forms_f32, L.volt_vk_forms_f64):
        # (V, bsv, jitter, resid, out, info, B, N, stream)
        assert forms(None, 8, 1, 1, 1, 1, 1, 8, None) == -1
        assert forms(1, 7, 1, 1, 1, 1, 2, 8, None) == -2                       # 0 < bsv < N: rows would overlap
        assert forms(1, -8, 1, 1, 1, 1, 2, 8, None) == -2
        assert forms(1, 0, None, 1, 1, 1, 1, 8, None) == -3                    # bsv = 0 (one shared grid) is legal
        assert forms(1, 8, 1, None, 1, 1, 1, 8, None) == -4
        assert forms(1, 8, 1, 1, None, 1, 1, 8, None) == -5
        assert forms(1, 8, 1, 1, 1, None, 1, 8, None) == -6
        assert forms(1, 8, 1, 1, 1, 1, 0, 8, None) == -7
        assert forms(1, 0, 1, 1, 1, 1, 1, 0, None) == -8


def test_bm_hip_cross_compiles_without_scratch_or_spills(tmp_path):
    from volt_amd.build import FLAGS, SOURCES, _hipcc
    assert "bm.hip" in SOURCES
    src = os.path.join(ROOT, "volt_amd", "csrc", "bm.hip")
    r = subprocess.run([_hipcc(), *FLAGS, "-c", src, "-o", str(tmp_path / "bm.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stderr.split("Function Name: ")[1:]
    forms = [b for b in blocks if "bm_forms_kernel" in b.split()[0]]
    assert len(forms) == 2, [b.split()[0] for b in blocks]                     # the fp32 and the fp64 instantiation
    for b in blocks:                                                           # every kernel of the file, the new ones included
        name = b.split()[0]
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
    for b in forms:
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 64 * 1024
    lib = os.path.join(ROOT, "volt_amd", "csrc", "libvolt_hip.so")
    from volt_amd import _lib
    _lib.lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    assert " T volt_vk_forms_f32" in syms and " T volt_vk_forms_f64" in syms
