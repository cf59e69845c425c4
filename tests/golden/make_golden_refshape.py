#!/usr/bin/env python3
"""Rollout / prediction-twin / mean-class fixtures at the reference drivers' own shapes, each run in fp32 AND fp64.

Why: rollouts.npz (make_golden.py) stops at N <= 120, H <= 8, k <= 25 and only has the reference's fp32 output, which
is itself up to ~1e-3 off an exact run at N = 399 -- too loose to see a wrong tap or a wrong padding value.  This
generator executes the reference's own code at the shapes its drivers use (experiments/stocks/GenerateMultiMeanPreds.py:
N = 399, H = 100, ewma / dewma / tewma x k up to 400; experiments/weather/GPGenerator.py: dt = 1/365, theta = 0.01, a
test grid two steps after the last train point) and runs every case twice:

  * fp32, exactly as the reference runs;
  * fp64: the same fp32 input VALUES cast to fp64, under torch.set_default_dtype(torch.float64).  The reference's own
    ``.type(torch.FloatTensor)`` casts on the means stay (they are its semantics), so the mean values are fp32-rounded
    in both runs; everything else (kernel fill, factor, solves, the rolled-out state) is fp64.

Both runs consume the identical N(0,1) numbers: the fp32 run's ``torch.randn`` draws are recorded and replayed (cast)
into the fp64 run -- torch's CPU generator gives different normals for float64, so reseeding would not do.  Every
``psd_safe_cholesky`` call is counted; a call that needed jitter fails the generator (today: none, in either precision).

Loading (as make_golden.py): the reference's means/EWMA.py, kernels/VolKernel.py, rollout_utils.py, models/VoltronGP.py
and models/VoltMagpie.py are executed from the reference tree with module stand-ins for the gpytorch / voltron names
they import.  Besides make_golden.py's stand-ins (Kernel, Mean, psd_safe_cholesky), these are RESTATEMENTS, not
gpytorch code:
    gpytorch.models.ExactGP    -> empty base class (only the twins' method bodies run, on a stand-in ``self``)
    ConstantMean               -> c for every input point (the weather driver's ``mean_func="constant"``)
    LinearMean(1)              -> w x + b, a [T] input read as [T,1] (gpytorch's matmul would take only T = 1)
    LogLinearMean              -> log(clamp(w x + b, 1e-6)) on that linear stand-in (voltron/means/loglinear_mean.py)
    voltron.models.BMGP        -> unused placeholders; the vol model is a fake returning a fixed log-vol draw
Everything else that runs -- Rollouts, GeneratePrediction, the model-method twins, EWMA and the four mean classes,
VolatilityKernel -- is the reference's code under real torch (CPU).

Writes tests/golden/rollouts_refshape.npz (rollouts) and tests/golden/refshape_twins.npz (twins + mean classes).
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_refshape.py      (about two minutes)
"""
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg

JITTERED = {"float32": 0, "float64": 0}
CALLS = {"float32": 0, "float64": 0}

# ---------------------------------------------------------------- cases
N, S, H = 399, 8, 100
STOCKS = [(m, k) for m in ("ewma", "dewma", "tewma") for k in (25, 100, 200, 300, 400)]
# tag -> (input set, mean, k, Rollouts theta)
ROLLOUT_CASES = {f"{m}_k{k}": ("s252", m, k, None) for m, k in STOCKS}
ROLLOUT_CASES.update({
    "meanrevert_k25": ("s252", "meanrevert", 25, None),
    "meanrevert_k400": ("s252", "meanrevert", 400, None),
    "ewma_k25_theta": ("s252", "ewma", 25, 0.01),
    "weather_const": ("w365", "const", 0, 0.01),
    "weather_loglin": ("w365", "loglin", 0, 0.01),
    "ewma_k25_s65": ("s65", "ewma", 25, None),
    "ewma_k25_h300": ("h300", "ewma", 25, None),
})
# input set -> (series seed, dt, S, H, weather grid)
INPUT_SETS = {"s252": (2024, 1 / 252., S, H, False), "w365": (2025, 1 / 365., S, H, True),
              "s65": (2024, 1 / 252., 65, H, False), "h300": (2024, 1 / 252., 4, 300, False)}
CONST = 2.3                        # weather constant mean (log scale)
LOGLIN_W, LOGLIN_B = 0.5, 9.5      # weather log-linear mean: log(0.5 x + 9.5) ~ log of the series' level
LIN_W, LIN_B = 0.3, 2.2            # VoltronGP twin's linear mean


def _install_more_standins(EW, VK):
    gp = sys.modules["gpytorch"]
    models = types.ModuleType("gpytorch.models")

    class ExactGP(torch.nn.Module):
        pass

    class ConstantMean(torch.nn.Module):
        def __init__(self, c=CONST):
            super().__init__()
            self.c = c

        def forward(self, x):
            return torch.full((x.shape[0],), self.c)

        __call__ = forward

    class LinearMean(torch.nn.Module):
        def __init__(self, w, b):
            super().__init__()
            self.w, self.b = w, b

        def forward(self, x):
            x = x if x.ndim > 1 else x.unsqueeze(-1)
            return (x * self.w).sum(-1) + self.b

        __call__ = forward

    class LogLinearMean(LinearMean):
        def forward(self, x):
            return super().forward(x).clamp(min=1e-6).log()

        __call__ = forward

    models.ExactGP = ExactGP
    gp.models = models
    gp.means.ConstantMean, gp.means.LinearMean = ConstantMean, LinearMean
    sys.modules["gpytorch.models"] = models
    vt = types.ModuleType("voltron")
    vm = types.ModuleType("voltron.models")
    bm = types.ModuleType("voltron.models.BMGP")
    bm.BMGP = bm.MultitaskBMGP = None
    vk = types.ModuleType("voltron.kernels")
    vk.VolatilityKernel = VK.VolatilityKernel
    vmeans = types.ModuleType("voltron.means")
    vmeans.EWMAMean, vmeans.DEWMAMean, vmeans.TEWMAMean = EW.EWMAMean, EW.DEWMAMean, EW.TEWMAMean
    for name, mod in (("voltron", vt), ("voltron.models", vm), ("voltron.models.BMGP", bm),
                      ("voltron.kernels", vk), ("voltron.means", vmeans)):
        sys.modules[name] = mod
    return ConstantMean, LinearMean, LogLinearMean


def _counting_cholesky():
    """Wrap the psd_safe_cholesky stand-in: count calls, and count the ones whose first factorisation failed."""
    c = sys.modules["gpytorch.utils.cholesky"]
    orig = c.psd_safe_cholesky

    def psd_safe_cholesky(A, *a, **kw):
        key = str(A.dtype).split(".")[-1]
        CALLS[key] += 1
        _, info = torch.linalg.cholesky_ex(A)
        if torch.any(info):
            JITTERED[key] += 1
        return orig(A, *a, **kw)
    c.psd_safe_cholesky = psd_safe_cholesky


class _ReplayRandn:
    """Replace torch.randn during a call: hand out the recorded draws in order, cast to the default dtype."""

    def __init__(self, draws):
        self.draws = list(draws)

    def __enter__(self):
        self._orig = torch.randn

        def rep(*shape, **kw):
            shape = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else shape
            d = self.draws.pop(0)
            assert tuple(d.shape) == tuple(shape), (d.shape, shape)
            return d.to(torch.get_default_dtype())
        torch.randn = rep
        return self

    def __exit__(self, *exc):
        torch.randn = self._orig
        assert exc[0] is not None or not self.draws, "not every recorded draw was consumed"


class _F64:
    def __enter__(self):
        self._old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *exc):
        torch.set_default_dtype(self._old)


def _inputs(name, g):
    seed, dt, s, h, weather = INPUT_SETS[name]
    F, vol = mg.sde_series(N, seed, dt)
    if weather:      # GPGenerator.py:38-41: train_x = arange(ntrain-1)/365, test_x = arange(ntrain, ntrain+H)/365
        train_x = torch.arange(N, dtype=torch.float32) / 365.
        test_x = torch.arange(N + 1, N + 1 + h, dtype=torch.float32) / 365.
    else:            # GenerateMultiMeanPreds.py:89-90
        train_x = torch.arange(N, dtype=torch.float32) * dt
        test_x = torch.arange(h, dtype=torch.float32) * dt + train_x[-1] + train_x[1]
    logv = (torch.randn(s, h, generator=g) * 0.05).cumsum(-1) + torch.tensor(vol)[-1].log()
    z = torch.randn(s, h, generator=g)
    return dict(train_x=train_x.numpy(), train_y=F, vol=vol, test_x=test_x.numpy(), pred_vol=logv.exp().numpy(),
                z=z.numpy())


def _rollout(RU, EW, means, inp, mean, k, theta, f64):
    ConstantMean, LinearMean, LogLinearMean = means
    dt = torch.float64 if f64 else torch.float32
    T = lambda a: torch.tensor(a).to(dt)
    train_x, train_y, test_x, vol = T(inp["train_x"]), T(inp["train_y"]), T(inp["test_x"]), T(inp["vol"])
    pred_vol, z = T(inp["pred_vol"]), torch.tensor(inp["z"])
    s = pred_vol.shape[0]

    class FakeVolModel:
        def __call__(self, x):
            return self

        def sample(self, size):
            return pred_vol.log()

    class FakeModel:
        pass
    model = FakeModel()
    model.train_x, model.train_y, model.log_vol_path = train_x, train_y[1:].log(), vol.log()
    if mean == "const":
        model.mean_module = ConstantMean()
    elif mean == "loglin":
        model.mean_module = LogLinearMean(LOGLIN_W, LOGLIN_B)
    else:
        cls = {"ewma": EW.EWMAMean, "dewma": EW.DEWMAMean, "tewma": EW.TEWMAMean,
               "meanrevert": EW.MeanRevertingEMAMean}[mean]
        model.mean_module = cls(train_x, train_y[1:].log(), k)
    model.covar_module = sys.modules["voltron.kernels"].VolatilityKernel()
    model.vol_model = FakeVolModel()
    draws = [z[:, i].reshape(s, 1, 1) for i in range(z.shape[1])]
    with _ReplayRandn(draws):
        out = RU.Rollouts(train_x, train_y, test_x, model, nsample=s, theta=theta)
    assert out.dtype == dt
    return out.numpy()


def _twin(cls, EW, means, inp, kind, k, T_, ns, seed, f64, z=None):
    """VoltronGP / VoltMagpie.GeneratePrediction (VoltronGP.py:62-95, VoltMagpie.py:67-99) on a stand-in self."""
    _, LinearMean, _ = means
    dt = torch.float64 if f64 else torch.float32
    Tt = lambda a: torch.tensor(a).to(dt)
    train_x, log_y, vol = Tt(inp["train_x"]), Tt(inp["train_y"])[1:].log(), Tt(inp["vol"])
    test_x, pv = Tt(inp["test_x"][:T_]), Tt(inp["pred_vol"][0, :T_])

    class Self:
        pass
    me = Self()
    me.train_x, me.train_y, me.train_inputs, me.log_vol_path = train_x, log_y, (train_x.unsqueeze(-1),), vol.log()
    me.covar_module = sys.modules["voltron.kernels"].VolatilityKernel()
    me.mean_module = LinearMean(LIN_W, LIN_B) if kind == "voltron" else EW.EWMAMean(train_x, log_y, k)
    if z is None:                             # fp32: the draw is recorded
        torch.manual_seed(seed)
        with mg._RecordRandn() as rec:
            try:
                out = cls.GeneratePrediction(me, test_x, pv, ns)
            except RuntimeError:
                out = None
        return out, (rec.draws[0] if rec.draws else None)
    with _ReplayRandn([z] if z is not None else []):
        try:
            out = cls.GeneratePrediction(me, test_x, pv, ns)
        except RuntimeError:
            out = None
    return out, z


def main():
    mg._install_standins()
    _counting_cholesky()
    VK = mg._load("ref_volkernel", "kernels/VolKernel.py")
    EW = mg._load("ref_ewma", "means/EWMA.py")
    means = _install_more_standins(EW, VK)
    RU = mg._load("ref_rollout", "rollout_utils.py")
    VG = mg._load("ref_voltrongp", "models/VoltronGP.py")
    VMp = mg._load("ref_voltmagpie", "models/VoltMagpie.py")
    g = torch.Generator().manual_seed(2026)
    out = {}
    inputs = {name: _inputs(name, g) for name in INPUT_SETS}
    for name, inp in inputs.items():
        for key, a in inp.items():
            out[f"{name}_{key}"] = np.asarray(a, dtype=np.float32)

    # ---- rollouts: fp32 and fp64 with the same draws -------------------------------------------------------------
    for tag, (iset, mean, k, theta) in ROLLOUT_CASES.items():
        inp = inputs[iset]
        s32 = _rollout(RU, EW, means, inp, mean, k, theta, False)
        with _F64():
            s64 = _rollout(RU, EW, means, inp, mean, k, theta, True)
        out[f"{tag}_set"], out[f"{tag}_mean"] = np.array(iset), np.array(mean)
        out[f"{tag}_k"] = np.array(k)
        out[f"{tag}_theta"] = np.array(np.nan if theta is None else theta)
        out[f"{tag}_s32"], out[f"{tag}_s64"] = s32.astype(np.float32), s64
        print(f"{tag:18s} |fp32 - fp64| max {np.abs(s32 - s64).max():.2e}", flush=True)
    out["jitter_calls"] = np.array([JITTERED["float32"], JITTERED["float64"]])
    out["const_c"], out["loglin_w"], out["loglin_b"] = np.array(CONST), np.array(LOGLIN_W), np.array(LOGLIN_B)
    np.savez_compressed(os.path.join(mg.OUT, "rollouts_refshape.npz"), **out)

    # ---- model-method twins ----------------------------------------------------------------------------------------
    tw = {"lin_w": np.array(LIN_W), "lin_b": np.array(LIN_B)}
    inp = inputs["s252"]
    for key in ("train_x", "train_y", "vol", "test_x", "pred_vol"):
        tw[f"in_{key}"] = np.asarray(inp[key], dtype=np.float32)
    twins = [(f"voltron_T{T_}_n{ns}", VG.VoltronGP, "voltron", 0, T_, ns) for T_ in (1, 10, 100) for ns in (1, 3)]
    twins += [(f"magpie_k{k}_T{T_}_n{ns}", VMp.VoltMagpie, "magpie", k, T_, ns)
              for k in (25, 400) for T_ in (1, 4) for ns in (1, 3)]
    for i, (tag, cls, kind, k, T_, ns) in enumerate(twins):
        seed = 300 + i
        o32, z = _twin(cls, EW, means, inp, kind, k, T_, ns, seed, False)
        with _F64():
            o64, _ = _twin(cls, EW, means, inp, kind, k, T_, ns, seed, True, z=z)
        assert (o32 is None) == (o64 is None), tag
        raises = o32 is None
        tw[f"{tag}_seed"], tw[f"{tag}_k"], tw[f"{tag}_T"], tw[f"{tag}_n"] = (np.array(v) for v in (seed, k, T_, ns))
        tw[f"{tag}_raises"] = np.array(raises)
        if raises:
            print(f"{tag:22s} raises in the reference", flush=True)
            continue
        tw[f"{tag}_z"] = z.numpy()
        tw[f"{tag}_s32"], tw[f"{tag}_s64"] = o32.numpy(), o64.numpy()
        print(f"{tag:22s} shape {tuple(o32.shape)} |fp32 - fp64| max {(o32.double() - o64).abs().max():.2e}", flush=True)

    # ---- mean classes at k > N and in the stacked [S, N+h] form Rollouts creates --------------------------------------
    y = torch.tensor(np.log(inp["train_y"][1:]))
    x = torch.tensor(inp["train_x"])
    hh = 50
    ext = torch.tensor(inp["pred_vol"][:, :hh])                # any [8,h] values near the series: a log-price walk
    ystack = torch.cat((y.repeat(S, 1), y[-1] + (ext - ext[:, :1]).cumsum(-1) * 0.1), -1)
    xstack = torch.cat((x, torch.tensor(inp["test_x"][:hh])))
    tw["mc_y"], tw["mc_x"], tw["mc_ystack"], tw["mc_xstack"] = y.numpy(), x.numpy(), ystack.numpy(), xstack.numpy()
    for cname, cls in (("ewma", EW.EWMAMean), ("dewma", EW.DEWMAMean), ("tewma", EW.TEWMAMean),
                       ("meanrevert", EW.MeanRevertingEMAMean)):
        for k in (200, 400):
            for prec in ("32", "64"):
                cast = (lambda a: a.double()) if prec == "64" else (lambda a: a)
                ctx = _F64() if prec == "64" else _NoCtx()
                with ctx:
                    mod = cls(cast(x), cast(y), k)
                    res = {"train": mod.forward(cast(x)), "one": mod.forward(cast(x[-1:]) + 1 / 252.),
                           "other": mod.forward(cast(x[: N // 2]))}
                    mod.train_x, mod.train_y = cast(xstack), cast(ystack)        # rollout_utils.py:81-82
                    res.update(btrain=mod.forward(cast(xstack)), bone=mod.forward(cast(xstack[-1:]) + 1 / 252.),
                               bother=mod.forward(cast(x)))
                for br, v in res.items():
                    assert v.dtype == torch.float32                              # the reference's FloatTensor cast
                    tw[f"mc_{cname}_k{k}_{br}_{prec}"] = v.numpy()
    tw["jitter_calls"] = np.array([JITTERED["float32"], JITTERED["float64"]])
    np.savez_compressed(os.path.join(mg.OUT, "refshape_twins.npz"), **tw)

    print("psd_safe_cholesky calls", CALLS, "needing jitter", JITTERED)
    assert JITTERED == {"float32": 0, "float64": 0}, "a fixture run needed jitter: the fixtures would not be comparable"
    for f in ("rollouts_refshape.npz", "refshape_twins.npz"):
        size = os.path.getsize(os.path.join(mg.OUT, f))
        print(f, size, "bytes")
        assert size <= 512 * 1024


class _NoCtx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


if __name__ == "__main__":
    main()
