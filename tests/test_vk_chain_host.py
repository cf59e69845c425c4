"""Host checks (no GPU) of the linear-time step of the volatility-kernel data model (data_solver="linear").  Two kinds of test:
  * the REFERENCE validated, not the feature: the restatement (tests/vk_chain_ref.py: per series the Brownian-motion
    recurrences on the grid V_b with vol = 1) against the project's fp64 oracle (oracle.volt_oracle.mll_and_grads) and dense
    fp64 LAPACK (bm_chain_ref.dense_step) on K = V[min(i,j)].  These exercise nothing of volt_amd and pass with or without the
    feature; they are what entitles tests/test_gpu_vk_linear.py to use the restatement.
  * the feature: the lazy _VolPrior, the data_solver / solver validation and the C entry points' argument checks."""
import numpy as np
import pytest
import torch

import bm_chain_ref as bm
import vk_chain_ref as ref
from oracle import volt_oracle

TOL = 1e-10                       # relative to each quantity's scale (bm_chain_ref.out_scales; max |.| for alpha)
SIZES = (1, 2, 3, 64, 65, 399, 1024)


@pytest.mark.parametrize("n", SIZES)
def test_restatement_matches_the_oracle_and_dense_lapack(n):
    worst = 0.0
    for fi, family in enumerate(ref.FAMILIES):
        rng = np.random.default_rng(100 * n + fi)
        V = ref.int_vol(ref.vol_path(family, n, rng))
        assert (np.diff(V) >= 0).all() and V[0] >= 0
        if family == "flat_zero" and n >= 64:
            assert ref.zero_increments(V) >= 10, ref.zero_increments(V)       # increments that vanish in fp32 are really there
        r = ref.resid(1, n, rng)
        K = ref.dense_k(V)
        for s in ref.NOISES:
            raw = float(np.log(np.expm1(s - 1e-4)))
            s_used = float(volt_oracle.noise_from_raw(raw))                   # what the oracle factors with
            out, alpha, info = ref.vk_step_ref(V, [s_used], r)
            assert not info.any() and out[0, 6] == s_used and out[0, 7] == 1.0
            dout, dalpha = bm.dense_step(V, [1.0], [s_used], r)
            orc = volt_oracle.mll_and_grads(K, r[0], np.zeros(n), raw)
            oout = np.array([[orc["mll"], orc["d_raw"] * (1.0 + np.exp(-raw)), orc["quad"], orc["logdet"], orc["trinv"], orc["aa"]]])
            scale = bm.out_scales(dout, n)
            for name, want, walpha in (("lapack", dout[:, :6], dalpha), ("oracle", oout, orc["alpha"][None])):
                err = np.abs(out[:, :6] - want) / scale
                aerr = np.abs(alpha - walpha).max(1) / np.abs(walpha).max(1)
                worst = max(worst, err.max(), aerr.max())
                assert err.max() <= TOL, (family, s, name, err)
                assert aerr.max() <= TOL, (family, s, name, aerr)
    print(f"N = {n}: worst relative error against the oracle / dense fp64 LAPACK {worst:.2e}")


def test_restatement_handles_per_series_grids_and_reports_pivots():
    V, s2, r = ref.mixed_case(5, 40)
    out, alpha, info = ref.vk_step_ref(V, s2, r)
    assert not info.any()
    for b in range(5):                                                        # every series against ITS grid only
        o, a, _ = bm.bm_step_ref(V[b], [1.0], [s2[b]], r[b][None])
        assert np.array_equal(out[b], o[0]) and np.array_equal(alpha[b], a[0])
    V0 = V.copy()
    V0[:, 0] = 0.0
    _, _, info = ref.vk_step_ref(V0[:2], [0.0, 1e-2], r[:2])                  # d_0 = V_0 + s = 0
    assert info.tolist() == [1, 0]
    Vn = V.copy()
    Vn[1, 7] = np.nan
    out, _, info = ref.vk_step_ref(Vn[:3], s2[:3], r[:3])
    assert info.tolist() == [0, 8, 0] and np.isfinite(out[[0, 2]]).all()


def test_vol_prior_is_lazy_and_has_the_dense_shape():
    from volt_amd import ops
    from volt_amd.gp import _Evaluated, _VolPrior, MultivariateNormal
    for shape in ((17,), (3, 17)):
        V = torch.rand(shape).cumsum(-1)
        p = _VolPrior(V)                                                      # CPU tensors: nothing has been filled, or it would have raised
        assert isinstance(p, _Evaluated) and p.x is V
        assert p.shape == torch.Size((*shape[:-1], 17, 17))
        assert MultivariateNormal(torch.zeros(shape), p).lazy_covariance_matrix is p
        for dense in (p.evaluate, p.to_dense, p.detach):
            with pytest.raises(ops._lib.VoltHipError):                        # the fill is the HIP kernel: no CPU path
                dense()


def test_data_solver_validation():
    from volt_amd import train_utils
    from volt_amd.forecast import GenerateStockPredictionsBatch, GenerateWindPredictionsBatch, _forecast_windows, _window_pass
    from volt_amd.gp import GaussianLikelihood
    from volt_amd.models import VoltMagpie, VoltronGP
    from volt_amd.models.Volt import Volt
    import inspect
    x = torch.arange(12, dtype=torch.float32) / 252
    y = torch.zeros(12)
    vol = torch.full((12,), 0.2)
    with pytest.raises(ValueError, match="data_solver must be one of"):
        VoltMagpie(x, y, GaussianLikelihood(), vol, k=3, data_solver="banded")
    with pytest.raises(ValueError, match="data_solver must be one of"):
        VoltronGP(x, y, GaussianLikelihood(), vol, data_solver="banded")
    with pytest.raises(ValueError, match="data_solver must be one of"):
        Volt(torch.arange(13, dtype=torch.float32) / 252, torch.zeros(13), vol_path=vol, data_solver="banded")
    for fn, args in ((train_utils.TrainDataModel, (x, y.exp(), None, None, vol)),
                     (train_utils.TrainVoltMagpieModel, (x, y.exp(), None, None, vol)),
                     (train_utils.TrainVoltMagpieBatch, (x, y.exp()[None], vol[None]))):
        with pytest.raises(ValueError, match="solver must be one of"):
            fn(*args, train_iters=0, solver="banded")
    for fn in (_window_pass, _forecast_windows, GenerateStockPredictionsBatch, GenerateWindPredictionsBatch):
        assert inspect.signature(fn).parameters["data_solver"].default == "dense"
    for fn in (train_utils.TrainDataModel, train_utils.TrainVoltMagpieModel, train_utils.TrainVoltMagpieBatch):
        assert inspect.signature(fn).parameters["solver"].default == "dense"


def test_vk_entry_points_validate_arguments_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    for step in (L.volt_vk_step_f32, L.volt_vk_step_f64):
        # (V, bsv, sigma2, resid, out, alpha, info, workspace, B, N, flags, stream)
        assert step(None, 8, 1, 1, 1, 1, 1, 256, 1, 8, 1, None) == -1
        assert step(1, 7, 1, 1, 1, 1, 1, 256, 2, 8, 1, None) == -2             # 0 < bsv < N: rows would overlap
        assert step(1, -8, 1, 1, 1, 1, 1, 256, 2, 8, 1, None) == -2
        assert step(1, 0, None, 1, 1, 1, 1, 256, 1, 8, 1, None) == -3          # bsv = 0 (one shared grid) is legal
        assert step(1, 8, 1, None, 1, 1, 1, 256, 1, 8, 1, None) == -4
        assert step(1, 8, 1, 1, None, 1, 1, 256, 1, 8, 1, None) == -5
        assert step(1, 8, 1, 1, 1, None, 1, 256, 1, 8, 1, None) == -6          # alpha is needed with VOLT_WANT_GRAD
        assert step(1, 8, 1, 1, 1, 1, None, 256, 1, 8, 1, None) == -7
        assert step(1, 8, 1, 1, 1, 1, 1, 8, 1, 8, 1, None) == -8               # workspace not 256-byte aligned
        assert step(1, 8, 1, 1, 1, 1, 1, None, 1, 8, 1, None) == -8
        assert step(1, 8, 1, 1, 1, 1, 1, 256, 0, 8, 1, None) == -9
        assert step(1, 0, 1, 1, 1, 1, 1, 256, 1, 0, 1, None) == -10
        assert step(1, 8, 1, 1, 1, 1, 1, 256, 1, 8, 2, None) == -11
