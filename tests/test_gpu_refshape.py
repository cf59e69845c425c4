"""Rollouts and the model-method prediction twins at the reference drivers' shapes, against the reference's own code run
in fp64 (tests/golden/rollouts_refshape.npz, tests/golden/refshape_twins.npz, written by make_golden_refshape.py).

rollouts.npz pins the engines only at N <= 120, H <= 8, k <= 25 and only to the reference's fp32 output, which at N = 399
is itself up to ~1e-3 (k = 25) off an fp64 run of the same code with the same draws.  Here: N = 399, H = 100, S = 8, every
mean family at k in {25, 100, 200, 300, 400} (k > N - 1 included; the lane engine and its wave-per-path fallback), mean
reversion, the theta branch, the weather grid (dt = 1/365, test points two steps after the last train point, an x-only
mean), S = 65 and H = 300.  The default engine is held to the fp64 run at BOUND64 = 2e-4: about 1/45 of the one-step
predictive sd (sqrt(dt/2) vol ~ 9e-3) and below the reference's own fp32 error."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND64 = 2e-4          # default (bordered) engine vs the fp64 reference run
BOUND32 = 2e-3          # any engine vs the reference's fp32 run (rollouts.npz's tolerance)
TWIN_BOUND = 1e-4       # model-method twins vs the fp64 run (fp32 reference vs fp64: <= 1.3e-5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODES = {"ewma": 0, "dewma": 1, "tewma": 2, "meanrevert": 3}


def _fx():
    return np.load(os.path.join(GOLDEN, "rollouts_refshape.npz"))


def _tw():
    return np.load(os.path.join(GOLDEN, "refshape_twins.npz"))


FX_TAGS = sorted(f[:-4] for f in np.load(os.path.join(GOLDEN, "rollouts_refshape.npz")).files if f.endswith("_s64"))
TW_TAGS = sorted(f[:-7] for f in np.load(os.path.join(GOLDEN, "refshape_twins.npz")).files if f.endswith("_raises"))


def dev(a):
    return torch.as_tensor(np.asarray(a)).cuda()


def _lane_eligible(mean, k):
    """csrc/rollout.hip: a lane per path when levels * k * 256 + 8k <= 150 KB (levels = 1, 2, 3 for ewma / dewma / tewma)."""
    levels = {"ewma": 1, "meanrevert": 1, "dewma": 2, "tewma": 3}.get(mean, 0)
    return levels * k * 256 + 8 * k <= 150 * 1024


def _case(d, tag, mean=None, k=None, theta="fixture"):
    """(model, Rollouts args, kwargs) for a fixture case, with optional deliberate changes (the negative controls)."""
    from volt_amd import means
    from volt_amd.gp import ConstantMean, GaussianLikelihood
    from volt_amd.models import VoltMagpie
    iset = str(d[f"{tag}_set"])
    mean = mean or str(d[f"{tag}_mean"])
    k = int(d[f"{tag}_k"]) if k is None else k
    th = float(d[f"{tag}_theta"])
    th = (None if np.isnan(th) else th) if theta == "fixture" else theta
    tx, ty, vol = dev(d[f"{iset}_train_x"]), dev(d[f"{iset}_train_y"]), dev(d[f"{iset}_vol"])
    model = VoltMagpie(tx, ty[1:].log(), GaussianLikelihood().cuda(), vol, k=max(k, 1))
    if mean == "const":
        model.mean_module = ConstantMean().cuda()
        with torch.no_grad():
            model.mean_module.constant.fill_(float(d["const_c"]))
    elif mean == "loglin":
        model.mean_module = means.LogLinearMean(1).cuda()
        with torch.no_grad():
            model.mean_module.weights.fill_(float(d["loglin_w"]))
            model.mean_module.bias.fill_(float(d["loglin_b"]))
    else:
        cls = {"ewma": means.EWMAMean, "dewma": means.DEWMAMean, "tewma": means.TEWMAMean,
                         "meanrevert": means.MeanRevertingEMAMean}[mean]
        model.mean_module = cls(tx, ty[1:].log(), k)
    pv, z = d[f"{iset}_pred_vol"], d[f"{iset}_z"]
    S = pv.shape[0]
    return model, (tx, ty, dev(d[f"{iset}_test_x"]), model), dict(nsample=S, theta=th, pred_vol=dev(pv), z=dev(z))


def _run(d, tag, engine=None, **kw):
    from volt_amd.gp import NumericalWarning
    from volt_amd.rollout_utils import Rollouts
    model, args, rkw = _case(d, tag, **kw)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = Rollouts(*args, engine=engine, **rkw)
    assert not [x for x in w if issubclass(x.category, NumericalWarning)], [str(x.message) for x in w]
    return model, out.numpy()


def _bound64(d, tag):
    """BOUND64 for paths at the level of the train series (|log y| <= y0 ~ 2.3), scaled by how far the reference's own
    fp64 paths wander beyond it.  Every rounding the engine makes is relative to the values it holds (fp32 samples and
    mean history, fp64 running sums), so for the same recursion the error grows with the path's magnitude: the stored
    fp32 sample alone carries ulp(|y|)/2, 1.9e-6 at |y| = 31 against 1.2e-7 at 2.3.  Only tewma at k = 25 (paths reach
    |y| = 31: a 3-level EMA at a short window feeds back with gain > 1) and the S = 65 / H = 300 cases leave the level."""
    y0 = float(np.abs(np.log(d[f"{d[f'{tag}_set']}_train_y"].astype(np.float64))).max())
    return BOUND64 * max(1.0, float(np.abs(d[f"{tag}_s64"]).max()) / y0)


def _dev64(d, tag, out):
    return float(np.abs(out.astype(np.float64) - d[f"{tag}_s64"]).max())


def dump_rollouts(tags, path):
    """Child-process entry of test_wave_per_path_fallback_vs_fp64_reference."""
    d = _fx()
    json.dump({t: _run(d, t)[1].tolist() for t in tags}, open(path, "w"))


# ------------------------------------------------------------------------------------------------------ default engine
@pytest.mark.parametrize("tag", FX_TAGS)
def test_bordered_engine_vs_fp64_reference(tag):
    """Public Rollouts(..., pred_vol=, z=) on the default engine vs the reference's fp64 run at BOUND64, and vs its fp32 run
    at 2e-3 wherever that run is itself within 2e-3 - BOUND64 of fp64 (at k = 25 the reference's fp32 output drifts up to
    2.9e-2 from fp64 over 100 dependent steps: dewma / tewma / S = 65 / H = 300 paths wander far from the series).  No
    pivot needs jitter (no NumericalWarning, so info == 0), and the model is left in the reference's final state.
    Measured on the MI355X: <= 5.8e-5 at the series' level (dewma k = 25; <= 1.3e-5 for ewma, 1.8e-6 on the weather
    grid), tewma k = 25 3.0e-4 against its scaled bound 2.5e-3; the wave fallback and the re-substitution give the same."""
    d = _fx()
    model, out = _run(d, tag)
    S, H = d[f"{tag}_s64"].shape
    assert out.shape == (S, H) and np.isfinite(out).all()
    e64 = _dev64(d, tag, out)
    print(f"DEV bordered {tag} {e64:.3e} bound {_bound64(d, tag):.1e}")
    assert e64 <= _bound64(d, tag), (tag, e64)
    gap = float(np.abs(d[f"{tag}_s32"] - d[f"{tag}_s64"]).max())
    if gap <= BOUND32 - _bound64(d, tag):
        np.testing.assert_allclose(out, d[f"{tag}_s32"], atol=BOUND32, rtol=0)
    # rollout_utils.py:80-86 with idx = H-1
    iset = str(d[f"{tag}_set"])
    n = d[f"{iset}_train_x"].shape[0]
    ty = d[f"{iset}_train_y"]
    assert tuple(model.train_y.shape) == (S, n + H - 1) and tuple(model.log_vol_path.shape) == (S, n + H - 1)
    assert np.array_equal(model.train_y[:, n:].cpu().numpy(), out[:, :H - 1])
    assert torch.equal(model.train_y[:, :n], dev(ty)[1:].log().repeat(S, 1))
    assert np.array_equal(model.train_x.cpu().numpy(), np.concatenate((d[f"{iset}_train_x"], d[f"{iset}_test_x"][:H - 1])))
    assert model.mean_module.train_y is model.train_y


def test_wave_per_path_fallback_vs_fp64_reference(tmp_path):
    """The lane-eligible cases again, in a child process started with VOLT_TUNE=1 VOLT_ROLLOUT_LANE=0 (the wave-per-path
    engine; dewma k >= 300 and tewma k >= 200 run it by default and are covered above), vs the fp64 run at BOUND64."""
    d = _fx()
    tags = [t for t in FX_TAGS if _lane_eligible(str(d[f"{t}_mean"]), int(d[f"{t}_k"]))]
    assert len(tags) >= 15
    e = dict(os.environ)
    e.update(VOLT_TUNE="1", VOLT_ROLLOUT_LANE="0")
    f = str(tmp_path / "wave.json")
    code = ("import sys; sys.path.insert(0, 'tests'); import test_gpu_refshape as t; "
            f"t.dump_rollouts({tags!r}, {f!r})")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.load(open(f))
    for t in tags:
        e64 = _dev64(d, t, np.asarray(res[t], dtype=np.float32))
        print(f"DEV wave {t} {e64:.3e}")
        assert e64 <= _bound64(d, t), (t, e64)


@pytest.mark.parametrize("tag", ["ewma_k200", "dewma_k200", "tewma_k200", "meanrevert_k400", "weather_const"])
def test_dense_engine_vs_reference(tag):
    """engine="dense" (the reference's algorithm on the device, fp32 factor per step): one case per mean family plus the
    weather case, vs both fixtures at 2e-3 -- the dense engine carries the reference's own fp32 round-off (measured vs
    fp64: <= 6.7e-4)."""
    d = _fx()
    _, out = _run(d, tag, engine="dense")
    e64 = _dev64(d, tag, out)
    print(f"DEV dense {tag} {e64:.3e}")
    assert e64 <= BOUND32, (tag, e64)
    np.testing.assert_allclose(out, d[f"{tag}_s32"], atol=BOUND32, rtol=0)


@pytest.mark.parametrize("tag", ["ewma_k400", "tewma_k100"])
def test_resubstitute_engine_vs_fp64_reference(tag):
    """rollout_series(..., resubstitute=True) -- the re-solving cross-check of the default engine -- vs the fp64 run."""
    from volt_amd import rollout_engine as re_
    d = _fx()
    iset = str(d[f"{tag}_set"])
    tx, ty, vol = dev(d[f"{iset}_train_x"]), dev(d[f"{iset}_train_y"]), dev(d[f"{iset}_vol"])
    out, info = re_.rollout_series(tx, ty[1:].log()[None], vol.log()[None], dev(d[f"{iset}_test_x"]),
                                   dev(d[f"{iset}_pred_vol"])[None], dev(d[f"{iset}_z"])[None],
                                   MODES[str(d[f"{tag}_mean"])], int(d[f"{tag}_k"]), resubstitute=True)
    assert int((info != 0).sum()) == 0
    e64 = _dev64(d, tag, out[0].cpu().numpy())
    print(f"DEV resubstitute {tag} {e64:.3e}")
    assert e64 <= _bound64(d, tag), (tag, e64)


# ------------------------------------------------------------------------------------------------------ negative controls
def test_negative_controls_are_visible_at_the_bound():
    """Each deliberately wrong variant, same inputs, must land at least 3 x BOUND64 from the fp64 run:
    k + 1 taps at k = 25; dewma in place of tewma at k = 100; theta dropped in the weather case.

    Not separable, by construction: the mean-reverting latent_mean taken from the stacked series instead of the one fixed
    at construction (EWMA.py:124).  The latent enters MeanRevertingEMAMean as ema[1:] += theta * latent, the same shift
    for every mean value of one step, and with the noise-free volatility kernel K^-1 u = e_last, so the predictive mean is
    r_last + m_new = y_last - m[N-1] + m_new: the shift cancels exactly.  That variant is held against the fp64 fixture in
    tests/test_oracle_golden.py (test_meanrevert_latent_choice_cancels), where the fp64 oracle shows it to rounding.
    Measured on the MI355X: k + 1 6.5e-2 (324x), dewma for tewma 1.27 (6360x), theta dropped 1.0e-1 (504x)."""
    d = _fx()
    ctrl = {}
    _, out = _run(d, "ewma_k25", k=26)
    ctrl["k+1"] = _dev64(d, "ewma_k25", out)
    _, out = _run(d, "tewma_k100", mean="dewma")
    ctrl["dewma for tewma"] = _dev64(d, "tewma_k100", out)
    _, out = _run(d, "weather_const", theta=None)
    ctrl["theta dropped"] = _dev64(d, "weather_const", out)
    print("DEV controls", {k: f"{v:.3e} ({v / BOUND64:.1f}x)" for k, v in ctrl.items()})
    for name, v in ctrl.items():
        assert v >= 3 * BOUND64, (name, v)


# ------------------------------------------------------------------------------------------------------ twins
def _twin_model(t, tag):
    from volt_amd.gp import GaussianLikelihood
    from volt_amd.models import VoltMagpie, VoltronGP
    tx, ty, vol = dev(t["in_train_x"]), dev(t["in_train_y"]), dev(t["in_vol"])
    if tag.startswith("voltron"):
        m = VoltronGP(tx, ty[1:].log(), GaussianLikelihood().cuda(), vol)
        with torch.no_grad():
            m.mean_module.weights.fill_(float(t["lin_w"]))
            m.mean_module.bias.fill_(float(t["lin_b"]))
    else:
        m = VoltMagpie(tx, ty[1:].log(), GaussianLikelihood().cuda(), vol, k=int(t[f"{tag}_k"]))
    return m


def _reference_rng_use(k):
    """What the reference's EWMAMean takes from the CPU generator before GeneratePrediction draws: EWMA() builds a
    torch.nn.Conv1d(1, 1, k) per call (EWMA.py:22), whose initialisation draws, and the method calls the mean twice
    (VoltMagpie.py:82,85).  The EWMA here is a HIP kernel and draws nothing (README, reference quirks); k = 0: a mean
    without state (VoltronGP's linear mean) draws nothing in either."""
    for _ in range(2 if k else 0):
        torch.nn.Conv1d(1, 1, kernel_size=k)


@pytest.mark.parametrize("tag", TW_TAGS)
def test_model_method_twins_vs_fp64_reference(tag):
    """VoltronGP / VoltMagpie.GeneratePrediction(test_x, pred_vol, n_sample) (VoltronGP.py:62-95, VoltMagpie.py:67-99):
    the T-point joint predictive through trtri + gemm_nt, the squeeze at n_sample = 1, and the reference's error case
    (VoltMagpie at T = 4: an EWMA mean of length N + 1 added to T rows raises there, and here).  The draws: the repo must
    take torch.randn(T, n_sample) on the CPU generator, the reference's shape and order; the generator is advanced as the
    reference's Conv1d-based EWMA advances it (_reference_rng_use).  Measured on the MI355X: <= 3.8e-6 (VoltronGP,
    T = 100), <= 1.2e-6 (VoltMagpie) against TWIN_BOUND = 1e-4."""
    t = _tw()
    T_, ns, seed = int(t[f"{tag}_T"]), int(t[f"{tag}_n"]), int(t[f"{tag}_seed"])
    m = _twin_model(t, tag)
    test_x, pv = dev(t["in_test_x"][:T_]), dev(t["in_pred_vol"][0, :T_])
    if bool(t[f"{tag}_raises"]):
        with pytest.raises(RuntimeError):
            m.GeneratePrediction(test_x, pv, ns)
        return
    k = int(t[f"{tag}_k"])
    torch.manual_seed(seed)
    _reference_rng_use(k)
    assert np.array_equal(torch.randn(T_, ns).numpy(), t[f"{tag}_z"])
    torch.manual_seed(seed)
    _reference_rng_use(k)
    out = m.GeneratePrediction(test_x, pv, ns).cpu().numpy()
    assert out.shape == t[f"{tag}_s64"].shape
    e64 = float(np.abs(out.astype(np.float64) - t[f"{tag}_s64"]).max())
    print(f"DEV twin {tag} {e64:.3e}")
    assert e64 <= TWIN_BOUND, (tag, e64)


# ------------------------------------------------------------------------------------------------------ mean classes
@pytest.mark.parametrize("k", [200, 400])
@pytest.mark.parametrize("cname", ["ewma", "dewma", "tewma", "meanrevert"])
def test_mean_classes_beyond_n_and_stacked(cname, k):
    """The four mean classes' three forward branches at N = 399 with k in {200, 400} (k > N: the window reaches into the
    padding), then in the stacked [8, N+50] form Rollouts gives them (rollout_utils.py:81-82; MeanRevertingEMAMean keeps
    the latent fixed at construction), vs the reference's fp64 run at 2e-6 relative (its fp32 run is itself up to 3.3e-6
    relative off at tewma k = 400: the CPU conv1d sums 400 fp32 products in fp32, three levels deep)."""
    from volt_amd import means
    t = _tw()
    cls = {"ewma": means.EWMAMean, "dewma": means.DEWMAMean, "tewma": means.TEWMAMean,
           "meanrevert": means.MeanRevertingEMAMean}[cname]
    x, y, xs, ys = (dev(t[f"mc_{n}"]) for n in ("x", "y", "xstack", "ystack"))
    mod = cls(x, y, k)
    res = {"train": mod(x), "one": mod(x[-1:] + 1 / 252.), "other": mod(x[: x.shape[0] // 2])}
    mod.train_x, mod.train_y = xs, ys
    res.update(btrain=mod(xs), bone=mod(xs[-1:] + 1 / 252.), bother=mod(x))
    for br, v in res.items():
        ref = t[f"mc_{cname}_k{k}_{br}_64"]
        assert tuple(v.shape) == ref.shape, (br, tuple(v.shape), ref.shape)
        np.testing.assert_allclose(v.cpu().numpy(), ref, rtol=2e-6, atol=0, err_msg=br)
