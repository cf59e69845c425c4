"""Multi-task GPCV on the MI355X (volt_gpcv_mt_step_f32, MultitaskVariationalGP, FitGPCVMultitask) against the fp64
Kronecker-structured oracle of tests/mt_gpcv_ref.py (itself checked against the dense NT x NT definition in
tests/test_mt_gpcv_host.py).

Tolerances are those tests/test_gpu_gpcv.py applies to the single-task step (fp32 HIP path vs fp64 oracle): every scalar
and F within 5e-5 max(1, |ref|); gradients within 2e-3 of the largest reference entry, grad_K within 5e-3.  Every figure
is printed before it is asserted."""
import math
import warnings

import pytest
import torch

import mt_gpcv_ref as R
from volt_amd.synthetic import sde_series

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gh():
    gx, gw = R.gauss_hermite(75)
    return gx.float().to(DEV), gw.float().to(DEV)


def _step(p, x, y, kernel="bm", want_dk=False, K=None):
    from volt_amd import ops
    N, T = y.shape
    if K is None:
        K = R.data_cov(x, p["raw_vol"], kernel)
    f = lambda t: t.float().to(DEV)
    gx, gw = _gh()
    ws = ops.gpcv_mt_step(f(K), f(p["m"]), f(p["c"]), f(p["Lx"]), f(p["Lt"]), f(p["F"]), f(p["raw_var"]), f(y), gx, gw,
                          want_dk=want_dk, w_ell=1.0 / N, w_kl=1.0 / (N * T))
    torch.cuda.synchronize()
    return ws


def _rel(a, r):
    return float((a.double().cpu().reshape(r.shape) - r).abs().max() / r.abs().max())


SCALARS = ((0, "ell"), (1, "kl"), (2, "q"), (3, "ld_k"), (4, "ld_kt"), (5, "ld_sx"), (6, "ld_st"), (7, "tau_x"),
           (8, "tau_t"), (9, "tr_kinv"), (10, "gg"), (11, "tr_aa"), (12, "F"))


@pytest.mark.parametrize("N,T,kernel,x0", [(33, 1, "bm", 1), (200, 3, "bm", 1), (399, 8, "bm", 1), (399, 8, "bm", 0),
                                           (399, 64, "bm", 1), (640, 5, "bm", 1), (1024, 8, "bm", 1), (2048, 4, "bm", 1),
                                           (300, 2, "fbm", 1), (257, 4, "fbm", 1)])
def test_step_matches_oracle(N, T, kernel, x0):
    from volt_amd.variational import mt_dkl_dscale
    p, x, y = R.case(N, T, seed=100 + N + T, x0=x0)
    fbm = kernel == "fbm"
    terms, grads = R.value_and_grads(R.struct, p, x, y, kernel=kernel)
    dk = fbm or (N, T, x0) in ((399, 8, 1), (1024, 8, 1))       # grad_K on the model's own prior too, at two of its shapes
    ws = _step(p, x, y, kernel, want_dk=dk)
    assert ws.info.tolist() == [0, 0, 0]
    out = ws.out.double().cpu()
    for col, key in SCALARS:
        err = abs(float(out[col] - terms[key])) / max(1.0, abs(float(terms[key])))
        print(f"({N},{T},{kernel},x0={x0}) {key}: ref {float(terms[key]):.8g} got {float(out[col]):.8g} err {err:.2e}")
    for col, key in SCALARS:
        assert abs(float(out[col] - terms[key])) <= 5e-5 * max(1.0, abs(float(terms[key]))), key
    assert float(out[13]) == pytest.approx(R.JITTER)
    errs = {"m": _rel(ws.grad_M, grads["m"]), "Lx": _rel(ws.grad_Lx, grads["Lx"]), "Lt": _rel(ws.grad_Lt, grads["Lt"]),
            "F": _rel(ws.grad_covar_factor, grads["F"]), "raw_var": _rel(ws.grad_raw_var, grads["raw_var"]),
            "c": _rel(ws.grad_c, grads["c"])}
    vol = torch.sigmoid(p["raw_vol"]).reshape(())
    if dk:
        _, gk = R.value_and_grads(R.struct, p, x, y, kernel=kernel, with_K=True)
        errs["K"] = _rel(ws.grad_K, gk["K"])
    if fbm:
        # d/d raw_vol by the chain rule through the fp64 kernel derivative, as the model's autograd does in fp32
        rv = p["raw_vol"].clone().requires_grad_(True)
        dK = torch.autograd.functional.jacobian(lambda r: R.data_cov(x, r, kernel), rv).reshape(N, N)
        g_rv = float((ws.grad_K.double().cpu() * dK).sum())
    else:
        dkl = float(mt_dkl_dscale(out, vol, N, T))
        g_rv = -dkl / (N * T) * float(vol * (1 - vol))
    errs["raw_vol"] = abs(g_rv - float(grads["raw_vol"])) / abs(float(grads["raw_vol"]))
    print(f"({N},{T},{kernel},x0={x0}) gradient errors / largest reference entry:", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < (5e-3 if k == "K" else 2e-3), (k, v)
    assert float(ws.grad_Lx.triu(1).abs().max()) == 0.0 and float(ws.grad_Lt.triu(1).abs().max()) == 0.0


def test_one_task_equals_the_single_task_step():
    """T = 1 with covar_factor = 0, raw_var = log(e - 1), L_t = 1 (K_t = S_t = 1) is the single-task step: F, grad_M,
    grad_Lx, grad_mu agree with ops.gpcv_step at the same inputs.  Both sit inside the oracle tolerances, so the gate is
    twice those; what differs is only the order of fp32 sums (largest differences printed)."""
    from volt_amd import ops
    N = 399
    p, x, y = R.case(N, 1, seed=7)
    p["F"] = torch.zeros(1, 1, dtype=torch.float64)
    p["raw_var"] = torch.tensor([math.log(math.e - 1)], dtype=torch.float64)
    p["Lt"] = torch.ones(1, 1, dtype=torch.float64)
    ws = _step(p, x, y)
    f = lambda t: t.float().to(DEV)
    gx, gw = _gh()
    K = f(R.data_cov(x, p["raw_vol"])).unsqueeze(0)
    m, c = f(p["m"][:, 0]).reshape(1, N), f(p["c"])
    st = ops.gpcv_step(K, m - c, m, f(p["Lx"]).unsqueeze(0), f(y[:, 0]).reshape(1, N), gx, gw, w_ell=1.0 / N, w_kl=1.0 / N)
    torch.cuda.synchronize()
    assert ws.info.tolist() == [0, 0, 0] and int(st.info.abs().sum()) == 0
    F1, F0 = float(ws.out[12]), float(st.out[0, 9])
    d = {"F": abs(F1 - F0) / max(1.0, abs(F0)),
         "grad_M": float((ws.grad_M[:, 0] - st.grad_m[0]).abs().max() / st.grad_m[0].abs().max()),
         "grad_Lx": float((ws.grad_Lx - st.grad_Lq[0]).abs().max() / st.grad_Lq[0].abs().max()),
         "grad_mu": abs(float(ws.grad_c[0]) - float(st.grad_mu[0].sum())) / max(1.0, abs(float(st.grad_mu[0].sum())))}
    print("T = 1 vs ops.gpcv_step, largest differences:", {k: f"{v:.2e}" for k, v in d.items()})
    assert d["F"] <= 2 * 5e-5
    assert d["grad_M"] <= 2 * 2e-3 and d["grad_Lx"] <= 2 * 2e-3 and d["grad_mu"] <= 2 * 2e-3


@pytest.mark.parametrize("N,T", [(399, 8), (1024, 8)])
def test_step_is_bitwise_repeatable(N, T):
    from volt_amd import ops
    p, x, y = R.case(N, T, seed=11)
    f = lambda t: t.float().to(DEV)
    gx, gw = _gh()
    args = (f(R.data_cov(x, p["raw_vol"])), f(p["m"]), f(p["c"]), f(p["Lx"]), f(p["Lt"]), f(p["F"]), f(p["raw_var"]), f(y),
            gx, gw)
    ws = ops.GpcvMtWorkspace(N, T, True, torch.device(DEV))
    names = ("out", "grad_M", "grad_c", "grad_Lx", "grad_Lt", "grad_covar_factor", "grad_raw_var", "grad_K")
    first = None
    for rep in range(10):
        ops.gpcv_mt_step(*args, ws, want_dk=True, w_ell=1.0 / N, w_kl=1.0 / (N * T))
        torch.cuda.synchronize()
        got = [getattr(ws, n).clone() for n in names]
        assert all(bool(torch.isfinite(g).all()) for g in got)
        if first is None:
            first = got
        else:
            for n, a, b in zip(names, first, got):
                assert torch.equal(a, b), (rep, n)


def _public(N, T, kernel="bm", seed=3, x0=1):
    """A model on the device holding the parameters of R.case, its ELBO and targets."""
    from volt_amd.kernels import BMKernel, FBMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import MultitaskVariationalGP
    from volt_amd.variational import VariationalELBO
    p, x, y = R.case(N, T, seed=seed, x0=x0)
    kern = {"bm": BMKernel, "fbm": FBMKernel}[kernel]()
    model = MultitaskVariationalGP(x.float().to(DEV), T, covar_module=kern)
    with torch.no_grad():
        model.variational_mean.copy_(p["m"])
        model.variational_covar_root.copy_(p["Lx"])
        model.variational_task_covar_root.copy_(p["Lt"])
        model.index_kernel.covar_factor.copy_(p["F"])
        model.index_kernel.raw_var.copy_(p["raw_var"])
        model.data_kernel.raw_vol.copy_(p["raw_vol"])
        for t, b in enumerate(model.mean_module.base_means):
            b.constant.fill_(float(p["c"][t]))
    lh = VolatilityGaussianLikelihood(param="exp")
    return model, lh, VariationalELBO(lh, model, N * T), p, x, y


@pytest.mark.parametrize("kernel", ["bm", "fbm"])
def test_public_classes_backward_and_kl(kernel):
    """elbo(model(x), y).backward() gives the oracle's gradient on every parameter (names from named_parameters()), and
    model.kl_divergence() is the step's KL."""
    from volt_amd.variational import num_gauss_hermite_locs
    N, T = 300, 3
    model, lh, elbo, p, x, y = _public(N, T, kernel)
    terms, grads = R.value_and_grads(R.struct, p, x, y, kernel=kernel)
    xd = model.inducing_points
    with num_gauss_hermite_locs(75):
        val = elbo(model(xd), y.float().to(DEV))
        val.backward()
    assert abs(float(val.detach()) - float(terms["F"])) <= 5e-5 * max(1.0, abs(float(terms["F"])))
    ref = {"variational_mean": grads["m"], "variational_covar_root": grads["Lx"], "variational_task_covar_root": grads["Lt"],
           "index_kernel.covar_factor": grads["F"], "index_kernel.raw_var": grads["raw_var"],
           "data_kernel.raw_vol": grads["raw_vol"]}
    ref.update({f"mean_module.base_means.{t}.constant": grads["c"][t].reshape(1) for t in range(T)})
    names = [n for n, _ in model.named_parameters()]
    assert sorted(names) == sorted(ref)
    cmax = float(grads["c"].abs().max())
    for n, prm in model.named_parameters():
        assert prm.grad is not None and prm.grad.shape == prm.shape, n
        r = ref[n]
        den = cmax if "constant" in n else float(r.abs().max())
        err = float((prm.grad.double().cpu() - r).abs().max()) / den
        print(kernel, n, f"{err:.2e}")
        assert err < 2e-3, n
    kl = float(model.kl_divergence())
    assert abs(kl - float(terms["kl"])) <= 5e-5 * max(1.0, abs(float(terms["kl"])))
    assert abs(kl - float(elbo._mt_ws.out[1])) <= 1e-6 * abs(kl)
    latent = model(xd)
    var = (p["Lx"].tril() ** 2).sum(-1)[:, None] * (p["Lt"].tril() ** 2).sum(-1)[None, :]
    assert tuple(latent.mean.shape) == (N, T)
    assert float((latent.variance.detach().double().cpu() - var).abs().max() / var.max()) < 1e-5
    E = torch.randn(4, N, T, generator=torch.Generator().manual_seed(0))
    s = latent.rsample(base_samples=E.to(DEV)).double().cpu()
    want = p["m"] + p["Lx"].tril() @ E.double() @ p["Lt"].tril().T
    assert float((s - want).abs().max()) < 1e-4 * float(want.abs().max())


def test_failed_factorisation_and_nan_are_reported():
    """A symmetric K_x with one diagonal entry -1 (a dense data kernel, the grad_K route): info > 0 and NotPSDError from the
    ELBO, not a VoltHipError; NaN in M: NanError; a non-positive K_t pivot lands in its own slot.  (Numerical conditions
    the step reports.)"""
    from volt_amd import gp
    from volt_amd.gp import NanError, NotPSDError
    from volt_amd.variational import num_gauss_hermite_locs
    N, T = 200, 3

    class DenseKernel(gp.Kernel):
        def __init__(self, K):
            super().__init__()
            self.K = torch.nn.Parameter(K)

        def forward(self, x1, x2=None, **kw):
            return self.K

    model, lh, elbo, p, x, y = _public(N, T)
    K = R.data_cov(x, p["raw_vol"]).float()
    K[57, 57] = -1.0
    model.data_kernel = DenseKernel(K).to(DEV)
    yd = y.float().to(DEV)
    with num_gauss_hermite_locs(75):
        with pytest.raises(NotPSDError):
            elbo(model(model.inducing_points), yd)
        assert int(elbo._mt_ws.info[0]) > 0
        model2, lh2, elbo2, *_ = _public(N, T)
        with torch.no_grad():
            model2.variational_mean[5, 1] = float("nan")
        with pytest.raises(NanError):
            elbo2(model2(model2.inducing_points), yd)
        assert int(elbo2._mt_ws.info[0]) == 0
    p["raw_var"] = torch.full((T,), -800.0, dtype=torch.float64)          # softplus -> 0 and f = 0: K_t = 0
    p["F"] = torch.zeros(T, 1, dtype=torch.float64)
    ws = _step(p, x, y)
    assert int(ws.info[0]) == 0 and int(ws.info[1]) > 0 and int(ws.info[2]) == 1


def _price_matrix(n, T, seed):
    return torch.stack([torch.tensor(sde_series(n, seed + i)[0]) for i in range(T)])


def test_initialize_variational_parameters_matches_fp64_restatement():
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import MultitaskVariationalGP
    n, T = 300, 4
    F = _price_matrix(n, T, 2019)
    x = torch.arange(n, dtype=torch.float32) / 252
    yy = R.scaled_returns(x, F)
    f, S_root, c0 = R.init_variational(x.double(), yy.double())
    torch.manual_seed(9)
    model = MultitaskVariationalGP(x.to(DEV), T, covar_module=BMKernel())
    torch.manual_seed(9)
    _, cf0 = torch.randn(n, T), torch.randn(T, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.initialize_variational_parameters(VolatilityGaussianLikelihood(param="exp"), x.to(DEV), y=yy.to(DEV))
    assert float((model.variational_mean.detach().cpu().double() - f).abs().max()) < 1e-5
    consts = torch.stack([b.constant.detach().cpu().double().reshape(()) for b in model.mean_module.base_means])
    assert float((consts - c0).abs().max()) < 1e-5
    assert torch.allclose(model.index_kernel.covar_factor.detach().cpu(), cf0 / 10.)
    S_hip = model.variational_covar_root.detach().cpu().double()
    assert float(S_hip.triu(1).abs().max()) > 0                   # stored as the reference stores it: a full matrix
    cov_h, cov_r = S_hip @ S_hip.T, S_root @ S_root.T
    err = float((cov_h - cov_r).abs().max() / cov_r.abs().max())
    print("init: S_root S_root' relative error", f"{err:.2e}")
    assert err < 2e-3


def test_fit_tracks_fp64_adam_eager_and_captured():
    """60 Adam iterations of FitGPCVMultitask at (399, 4), eager and graph=True, against fp64 Adam on the oracle from the
    same start and lr: the band of test_learn_gpcv_tracks_oracle (loss within 5e-4 max(1, |want|), first loss within 1e-4
    relative); LearnGPCVMultitask returns [T,N], finite, >= 1e-3."""
    from volt_amd.train_utils import FitGPCVMultitask, LearnGPCVMultitask
    n, T, iters = 399, 4, 60
    F = _price_matrix(n, T, 2021)
    x = torch.arange(n, dtype=torch.float32) / 252
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(21)
        m0, _, _ = FitGPCVMultitask(x.to(DEV), F.to(DEV), train_iters=0)
        start = {"m": m0.variational_mean, "Lx": m0.variational_covar_root, "Lt": m0.variational_task_covar_root,
                 "c": torch.cat([b.constant.reshape(1) for b in m0.mean_module.base_means]),
                 "raw_vol": m0.data_kernel.raw_vol, "F": m0.index_kernel.covar_factor, "raw_var": m0.index_kernel.raw_var}
        start = {k: v.detach().cpu() for k, v in start.items()}
        torch.manual_seed(21)
        model, lh, losses = FitGPCVMultitask(x.to(DEV), F.to(DEV), train_iters=iters, graph=False)
        torch.manual_seed(21)
        model_g, _, losses_g = FitGPCVMultitask(x.to(DEV), F.to(DEV), train_iters=iters, graph=True)
        vol = LearnGPCVMultitask(x.to(DEV), F.to(DEV), train_iters=5)
    yy = R.scaled_returns(x.double(), F.double())
    want, ps = R.fit(x.double(), yy, start, iters)
    want = torch.tensor(want, dtype=torch.float64)
    got = torch.stack(losses).cpu().double()
    assert got.shape == want.shape
    band = ((got - want).abs() / want.abs().clamp_min(1.0))
    print("fit: max loss deviation", f"{float(band.max()):.2e}", "first", f"{abs(float(got[0] - want[0])) / abs(float(want[0])):.2e}",
          "loss", float(want[0]), "->", float(want[-1]))
    assert float(band.max()) < 5e-4
    assert abs(float(got[0] - want[0])) < 1e-4 * abs(float(want[0]))
    assert float(want[-1]) < float(want[0])
    last_g = float(losses_g[-1])
    print("fit: captured last loss", last_g, "eager", float(got[-1]), "fp64", float(want[-1]))
    assert abs(last_g - float(want[-1])) < 5e-4 * max(1.0, abs(float(want[-1])))
    assert abs(last_g - float(got[-1])) < 2 * 5e-4 * max(1.0, abs(float(want[-1])))
    assert float((model.variational_mean.detach().cpu().double() - ps["m"]).abs().max()) < 5e-3
    assert tuple(vol.shape) == (T, n) and bool(torch.isfinite(vol).all()) and float(vol.min()) >= 1e-3
