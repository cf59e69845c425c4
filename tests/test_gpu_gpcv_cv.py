"""The copula-process ("cv") GPCV step and its trainer on the MI355X against the fp64 reference of tests/gpcv_cv_ref.py
(itself checked in tests/test_gpcv_cv_host.py).  volt_gpcv_cv_step_f32 replaces volatility_likelihood.py:43-51 under the
75-node quadrature of the ELBO (train_utils.py:50).

Tolerances are the project's existing ones for this path (tests/test_gpu_gpcv.py): scalars and F 5e-5 max(1, |ref|);
grad_m, grad_Lq, grad_mu 2e-3 of the reference gradient's max; grad_K 5e-3; each of grad_a, grad_b, grad_c 2e-3 of that
vector's max.  Every case prints its figures before it asserts."""
import math
import warnings

import pytest
import torch

import gpcv_cv_ref as R
from oracle import gpcv_oracle as GO
from test_gpu_gpcv import GENERIC_SHAPES, _prices, _prior, _problem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(200, 1, "bm"), (399, 3, "bm"), (512, 2, "bm"), (300, 2, "fbm"), (33, 1, "bm"), (129, 2, "bm"), (257, 1, "fbm"),
          (640, 9, "bm")] + GENERIC_SHAPES                   # test_gpcv_step_matches_oracle's


def _reference(n, B, kernel, Kc, root_scale=1.0):
    """fp64 value and gradients per series: inputs from test_gpu_gpcv._problem, raw_a, raw_b, raw_c as the class draws them."""
    raw_vol = torch.logit(torch.tensor([0.2], dtype=torch.float64))
    gh_x, gh_w = GO.gauss_hermite(75)
    series = []
    for b in range(B):
        x, yy, m, Lq, c = _problem(n, 2019 + b)
        Lq = Lq.tril() * root_scale + Lq.triu(1)                                # (the junk above the diagonal stays junk)
        abc = torch.stack(R.constrain(*R.draw_raw(Kc, 7000 + 31 * b + Kc)))     # [3,Kc] transformed
        ps = [t.clone().requires_grad_(True) for t in (m, Lq, c, abc)]
        vol = torch.sigmoid(raw_vol)
        K = _prior(kernel, x, vol, 2019 + b).detach().requires_grad_(True)
        t = dict(GO.elbo_terms(ps[0], ps[1], ps[2], K, yy, gh_x, gh_w))         # KL and its pieces
        e, clamped = R.ell(ps[0], ps[1], yy, ps[3][0], ps[3][1], ps[3][2], gh_x, gh_w)
        t.update(ell=e, elbo=e / n - t["kl"] / n)
        g = torch.autograd.grad(t["elbo"], ps + [K])
        series.append(dict(yy=yy, m=m, Lq=Lq, c=c, abc=abc, K=K.detach(), grads=g, clamped=clamped,
                           terms={k: float(v.detach()) for k, v in t.items()}))
    return series, gh_x, gh_w


def _run(series, gh_x, gh_w, n, want_dk=True):
    from volt_amd import ops
    f32 = lambda key: torch.stack([s[key].to(torch.float32) for s in series]).to(DEV)
    K, m, Lq, y, abc = f32("K"), f32("m"), f32("Lq"), f32("yy"), f32("abc")
    mu = torch.stack([s["c"].to(torch.float32).expand(n) for s in series]).to(DEV)
    ws = ops.gpcv_cv_step(K, m - mu, m, Lq, y, abc, gh_x.to(DEV), (gh_w / math.sqrt(math.pi)).to(DEV), want_dk=want_dk,
                          w_ell=1.0 / n, w_kl=1.0 / n)
    torch.cuda.synchronize()
    return ws


def _check_against_reference(ws, series, label):
    assert int(ws.info.abs().sum()) == 0
    out = ws.out.double().cpu()
    worst = dict(scal=0.0, gm=0.0, gL=0.0, gmu=0.0, gK=0.0, ga=0.0, gb=0.0, gc=0.0)
    rel = lambda a, r: float((a.double().cpu() - r).abs().max() / r.abs().max())
    for b, s in enumerate(series):
        t = s["terms"]
        for col, key in ((0, "ell"), (1, "kl"), (2, "quad"), (3, "logdet_k"), (4, "logdet_s"), (5, "trace"), (9, "elbo")):
            worst["scal"] = max(worst["scal"], abs(float(out[b, col]) - t[key]) / max(1.0, abs(t[key])))
        gm, gL, gc_, gabc, gK = s["grads"]
        worst["gm"] = max(worst["gm"], rel(ws.grad_m[b], gm))
        worst["gL"] = max(worst["gL"], rel(ws.grad_Lq[b], gL))
        worst["gmu"] = max(worst["gmu"], abs(float(ws.grad_mu[b].sum()) - float(gc_)) / max(1.0, abs(float(gc_))))
        worst["gK"] = max(worst["gK"], rel(ws.grad_K[b], gK))
        for i, key in enumerate(("ga", "gb", "gc")):
            worst[key] = max(worst[key], rel(ws.grad_abc[b, i], gabc[i]))
    print("CVSTEP", label, "clamped %.3f" % max(s["clamped"] for s in series),
          " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert worst["scal"] <= 5e-5, worst
    assert worst["gm"] < 2e-3 and worst["gL"] < 2e-3 and worst["gmu"] < 2e-3, worst
    assert worst["gK"] < 5e-3, worst
    assert worst["ga"] < 2e-3 and worst["gb"] < 2e-3 and worst["gc"] < 2e-3, worst


@pytest.mark.parametrize("Kc", [1, 5, 8])
@pytest.mark.parametrize("n,B,kernel", SHAPES)
def test_cv_step_matches_fp64_reference(n, B, kernel, Kc):
    series, gh_x, gh_w = _reference(n, B, kernel, Kc)
    ws = _run(series, gh_x, gh_w, n)
    _check_against_reference(ws, series, f"n={n} B={B} {kernel} Kc={Kc}")


def test_cv_step_with_a_sizeable_share_of_clamped_nodes():
    """The covariance root scaled x10: the nodes reach far enough down that a sizeable share of them sits under the
    min_scale clamp (scale = 1e-3, no gradient).  Same tolerances."""
    n, B, Kc = 399, 3, 5
    series, gh_x, gh_w = _reference(n, B, "bm", Kc, root_scale=10.0)
    assert min(s["clamped"] for s in series) > 0.05, [s["clamped"] for s in series]
    ws = _run(series, gh_x, gh_w, n)
    _check_against_reference(ws, series, f"n={n} B={B} bm Kc={Kc} root x10")


@pytest.mark.parametrize("n,B", [(200, 1), (399, 2)])
def test_cv_step_reduces_to_the_exp_step(n, B):
    """Kc = 1, a = e^20, b = 1, c = -20: e^20 softplus(f - 20) = exp(f) (1 - exp(f - 20)/2 + ...), exp f to ~1e-9 at the
    f of these problems.  The "cv" step must then give what volt_gpcv_step_f32 gives on the same inputs: out to
    5e-5 max(1, |.|), gradients to 2e-3 of their max."""
    from volt_amd import ops
    probs = [_problem(n, 2019 + b) for b in range(B)]
    f32 = lambda ts: torch.stack([t.to(torch.float32) for t in ts]).to(DEV)
    x = probs[0][0]
    K = f32([GO.bm_cov(x, torch.tensor(0.2, dtype=torch.float64))] * B)
    m, Lq, y = f32([p[2] for p in probs]), f32([p[3] for p in probs]), f32([p[1] for p in probs])
    mu = f32([p[4].expand(n) for p in probs])
    gh_x, gh_w = GO.gauss_hermite(75)
    gx, gw = gh_x.to(DEV), (gh_w / math.sqrt(math.pi)).to(DEV)
    abc = torch.tensor([math.exp(20.0), 1.0, -20.0], device=DEV).reshape(1, 3, 1).expand(B, 3, 1)
    we = ops.gpcv_step(K, m - mu, m, Lq, y, gx, gw, want_dk=True, w_ell=1.0 / n, w_kl=1.0 / n)
    wc = ops.gpcv_cv_step(K, m - mu, m, Lq, y, abc, gx, gw, want_dk=True, w_ell=1.0 / n, w_kl=1.0 / n)
    torch.cuda.synchronize()
    assert int(we.info.abs().sum()) == 0 and int(wc.info.abs().sum()) == 0
    d_out = float(((wc.out - we.out).abs() / we.out.abs().clamp_min(1.0)).max())
    rel = lambda a, r: float((a - r).abs().max() / r.abs().max())
    figs = dict(out=d_out, gm=rel(wc.grad_m, we.grad_m), gL=rel(wc.grad_Lq, we.grad_Lq), gmu=rel(wc.grad_mu, we.grad_mu),
                gK=rel(wc.grad_K, we.grad_K))
    print("CVEXP", n, B, " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
    assert d_out <= 5e-5
    assert all(figs[k] < 2e-3 for k in ("gm", "gL", "gmu", "gK")), figs
    assert torch.equal(wc.out[:, 1:9], we.out[:, 1:9])            # what the likelihood does not touch is the same launches


@pytest.mark.parametrize("n,B,Kc", [(200, 1, 1), (399, 3, 5)])
def test_cv_step_is_bitwise_repeatable(n, B, Kc):
    """30 repeats on one workspace: every output, grad_abc included, keeps its bits (fixed-order reductions, no atomics)."""
    from volt_amd import ops
    gh_x, gh_w = GO.gauss_hermite(75)
    probs = [_problem(n, 2019 + b) for b in range(B)]
    f32 = lambda ts: torch.stack([t.to(torch.float32) for t in ts]).to(DEV)
    K = f32([GO.bm_cov(probs[0][0], torch.tensor(0.2, dtype=torch.float64))] * B)
    m, Lq, y = f32([p[2] for p in probs]), f32([p[3] for p in probs]), f32([p[1] for p in probs])
    mu = f32([p[4].expand(n) for p in probs])
    abc = f32([torch.stack(R.constrain(*R.draw_raw(Kc, 7000 + b))) for b in range(B)])
    gx, gw = gh_x.to(DEV), (gh_w / math.sqrt(math.pi)).to(DEV)
    ws = ops.GpcvWorkspace(B, n, True, torch.device(DEV), Kc=Kc)
    names = ("out", "grad_m", "grad_mu", "grad_Lq", "grad_K", "grad_abc", "info")
    first = None
    for _ in range(30):
        ops.gpcv_cv_step(K, m - mu, m, Lq, y, abc, gx, gw, ws, want_dk=True, w_ell=1.0 / n, w_kl=1.0 / n)
        got = [getattr(ws, k).clone() for k in names]
        if first is None:
            first = got
            assert int(ws.info.abs().sum()) == 0 and bool(torch.isfinite(ws.grad_abc).all())
        for k, a, b_ in zip(names, got, first):
            assert torch.equal(a, b_), k


def _public(n, K=1, seed=5, price_seed=2021):
    """A "cv" likelihood, its model (started by initialize_variational_parameters) and ELBO through the public classes."""
    from volt_amd import gp
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import SingleTaskVariationalGP
    from volt_amd.variational import VariationalELBO
    F, _ = _prices(n, price_seed)
    x = (torch.arange(n, dtype=torch.float32) / 252).to(DEV)
    yy = GO.scaled_returns(x.cpu(), F).to(DEV)
    torch.manual_seed(seed)
    lik = VolatilityGaussianLikelihood(K=K, param="cv").to(DEV)
    model = SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=lik, use_piv_chol_init=False,
                                    mean_module=gp.ConstantMean(), covar_module=BMKernel().to(DEV),
                                    learn_inducing_locations=False, use_whitened_var_strat=False)
    if K == 1:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model.initialize_variational_parameters(lik, x, y=yy)
    return model, lik, VariationalELBO(lik, model, n), x, yy


def test_errors_are_reported_by_kind(monkeypatch):
    """Kc = 0 and Kc = 9: the entry's argument code; a non-PD K: NotPSDError; NaN input: NanError; an internal code in
    info: VoltHipError; CPU tensors: VoltHipError."""
    from volt_amd import gp, ops
    from volt_amd._lib import VoltHipError
    from volt_amd.gp import NanError, NotPSDError
    from volt_amd.variational import num_gauss_hermite_locs
    n = 200
    z = lambda *s: torch.zeros(*s, device=DEV)
    eye = torch.eye(n, device=DEV)[None]
    # (an empty abc has no address: Kc = 0 is refused as argument 9, the null abc, or 10, Kc itself)
    for Kc, which in ((0, "#(9|10)$"), (9, "#10$")):
        with pytest.raises(VoltHipError, match="invalid argument " + which):
            ops.gpcv_cv_step(eye, z(1, n), z(1, n), eye, z(1, n), torch.ones(1, 3, Kc, device=DEV), z(75), z(75))
    with pytest.raises(VoltHipError):
        ops.gpcv_cv_step(eye.cpu(), z(1, n).cpu(), z(1, n).cpu(), eye.cpu(), z(1, n).cpu(), torch.ones(1, 3, 1), z(75).cpu(),
                         z(75).cpu())

    class DenseKernel(gp.Kernel):
        def __init__(self, K):
            super().__init__()
            self.K = torch.nn.Parameter(K)

        def forward(self, x1, x2=None, **kw):
            return self.K

    with num_gauss_hermite_locs(75):
        model, lik, elbo, x, yy = _public(n, K=5)
        good = elbo(model(x), yy)
        assert bool(torch.isfinite(good))
        K = GO.bm_cov(x.cpu().double(), torch.tensor(0.2, dtype=torch.float64)).float()
        K[57, 57] = -1.0
        model.covar_module = DenseKernel(K).to(DEV)
        with pytest.raises(NotPSDError):
            elbo(model(x), yy)
        assert int(elbo._ws.info[0]) > 0
        model2, lik2, elbo2, x, yy = _public(n, K=5)
        K = GO.bm_cov(x.cpu().double(), torch.tensor(0.2, dtype=torch.float64)).float()
        K[5, 7] = K[7, 5] = float("nan")
        model2.covar_module = DenseKernel(K).to(DEV)
        with pytest.raises(NanError):
            elbo2(model2(x), yy)
        model3, lik3, elbo3, x, yy = _public(n, K=5)
        real = ops.gpcv_cv_step

        def internal(*a, **kw):                                # the step ran; its info then reads as a hand-off time-out
            ws = real(*a, **kw)
            ws.info.fill_(-2 ** 31)
            return ws

        monkeypatch.setattr(ops, "gpcv_cv_step", internal)
        with pytest.raises(VoltHipError, match="internal"):
            elbo3(model3(x), yy)


def test_expected_log_prob_agrees_with_the_fused_cv_step():
    """expected_log_prob (torch, per point) sums to the likelihood term of the fused step, as for "exp"."""
    from volt_amd import ops
    from volt_amd.variational import num_gauss_hermite_locs
    n = 140
    model, lik, elbo, x, yy = _public(n, K=5, price_seed=77)
    d = model.variational_strategy._variational_distribution
    with torch.no_grad():
        d.variational_mean.copy_(-1.5 + 0.2 * torch.randn(n, device=DEV))
        d.chol_variational_covar.copy_((0.3 * torch.eye(n, device=DEV) + 0.01 * torch.randn(n, n, device=DEV)).tril())
    latent = model(x)
    with num_gauss_hermite_locs(75), torch.no_grad():
        per_point = lik.expected_log_prob(yy, latent)
    assert tuple(per_point.shape) == (n,)
    gh_x, gh_w = GO.gauss_hermite(75)
    K = GO.bm_cov(x.cpu().double(), torch.tensor(0.2, dtype=torch.float64)).float().to(DEV).unsqueeze(0)
    abc = torch.stack([lik.trans_a, lik.trans_b, lik.trans_c]).detach().reshape(1, 3, 5)
    mm = d.variational_mean.detach().reshape(1, n)
    ws = ops.gpcv_cv_step(K, mm, mm, d.chol_variational_covar.detach().reshape(1, n, n), yy.reshape(1, n), abc, gh_x.to(DEV),
                          (gh_w / math.sqrt(math.pi)).to(DEV))
    print("CVELP", float(per_point.sum()), float(ws.out[0, 0]))
    assert abs(float(per_point.sum()) - float(ws.out[0, 0])) < 2e-4 * abs(float(ws.out[0, 0]))


@pytest.mark.parametrize("tag", ["n60_f32", "n60_f64", "n90_f32", "n90_f64", "n80_wind_f32", "n80_wind_f64"])
def test_cv_start_up_matches_the_reference_code(golden, tag):
    """(e), device half: the HIP-backed ``initialize_variational_parameters`` ("cv", K = 1) against tests/golden/gpcv_cv.npz,
    outputs of the reference's own code (single_task_variational_gp.py:204-254, executed by make_golden_gpcv_cv.py) in fp32
    and in fp64, at the tolerance test_start_up_matches_the_reference_code uses for "exp": mean and constant 1e-5, the
    covariance the factor stands for 2e-3.  tests/test_gpcv_cv_host.py shows the reference's own fp32 run within the same
    band of its fp64 run."""
    from volt_amd import gp
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import SingleTaskVariationalGP
    g = golden("gpcv_cv")
    x = torch.tensor(g[f"{tag}_x"]).float().to(DEV)
    yy = torch.tensor(g[f"{tag}_y"]).float().to(DEV)
    raw = torch.tensor(g[f"{tag}_raw"]).float()
    lik = VolatilityGaussianLikelihood(K=1, param="cv")
    with torch.no_grad():
        lik.raw_a.copy_(raw[0]), lik.raw_b.copy_(raw[1]), lik.raw_c.copy_(raw[2])
    lik = lik.to(DEV)
    model = SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=lik, use_piv_chol_init=False,
                                    mean_module=gp.ConstantMean(), covar_module=BMKernel().to(DEV),
                                    learn_inducing_locations=False, use_whitened_var_strat=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.initialize_variational_parameters(lik, x, y=yy)
    d = model.variational_strategy._variational_distribution
    e_mean = float((d.variational_mean.detach().cpu().double() - torch.tensor(g[f"{tag}_mean"]).double()).abs().max())
    e_const = abs(float(model.mean_module.constant.detach()) - float(g[f"{tag}_const"].reshape(-1)[0]))
    S_hip, S_ref = d.chol_variational_covar.cpu().double(), torch.tensor(g[f"{tag}_chol"]).double()
    cov_h, cov_r = S_hip @ S_hip.mT, S_ref @ S_ref.mT
    e_cov = float((cov_h - cov_r).abs().max() / cov_r.abs().max())
    print("CVINIT", tag, f"mean {e_mean:.2e} const {e_const:.2e} cov {e_cov:.2e}")
    assert e_mean < 1e-5
    assert e_const < 1e-5
    assert e_cov < 2e-3


def _start_of(model, lik):
    d = model.variational_strategy._variational_distribution
    return ((d.variational_mean.detach().cpu(), d.chol_variational_covar.detach().cpu(),
             model.mean_module.constant.detach().cpu().reshape(())),
            [p.detach().cpu().reshape(-1) for p in (lik.raw_a, lik.raw_b, lik.raw_c)])


def test_fit_cv_tracks_fp64_adam_eager_and_captured():
    """40 Adam iterations of FitGPCV(param="cv", K=1, train_likelihood=True), eager and graph=True, against fp64 Adam on the
    reference from the same start, at the tolerances of test_learn_gpcv_tracks_oracle: losses 5e-4 relative (first loss
    1e-4), variational mean and scalar parameters (the likelihood's three included) 5e-3, readout 3e-2; the captured
    loop's last loss agrees with the eager one as test_fit_tracks_fp64_adam_eager_and_captured asks of "exp" loops."""
    from volt_amd.train_utils import FitGPCV
    n, iters = 250, 40
    F, _ = _prices(n, 2021)
    x = torch.arange(n, dtype=torch.float32) / 252
    kw = dict(param="cv", K=1, train_likelihood=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(17)
        m0, l0, _ = FitGPCV(x.to(DEV), F.to(DEV), train_iters=0, **kw)
        start, raws = _start_of(m0, l0)
        torch.manual_seed(17)
        model, lh, losses = FitGPCV(x.to(DEV), F.to(DEV), train_iters=iters, graph=False, **kw)
        torch.manual_seed(17)
        model_g, lh_g, losses_g = FitGPCV(x.to(DEV), F.to(DEV), train_iters=iters, graph=True, **kw)
    yy = GO.scaled_returns(x.double(), F.double())
    want, ps = R.learn(x.double(), yy, start, raws, iters)
    want = torch.tensor(want, dtype=torch.float64)
    got = torch.stack(losses).cpu().double()
    assert got.shape == want.shape
    band = float(((got - want).abs() / want.abs().clamp_min(1.0)).max())
    first = abs(float(got[0] - want[0])) / abs(float(want[0]))
    d = model.variational_strategy._variational_distribution
    e_mean = float((d.variational_mean.detach().cpu().double() - ps[0]).abs().max())
    e_vol = abs(float(model.covar_module.raw_vol.detach()) - float(ps[3]))
    e_const = abs(float(model.mean_module.constant.detach()) - float(ps[2]))
    e_lik = [abs(float(p.detach()) - float(q)) for p, q in zip((lh.raw_a, lh.raw_b, lh.raw_c), ps[4:])]
    moved = [abs(float(q) - float(r)) for q, r in zip(ps[4:], raws)]
    last_g = float(losses_g[-1])
    print("CVFIT band %.2e first %.2e mean %.2e vol %.2e const %.2e lik %s moved %s loss %.6f -> %.6f captured %.6f eager %.6f"
          % (band, first, e_mean, e_vol, e_const, ["%.2e" % e for e in e_lik], ["%.2e" % e for e in moved], float(want[0]),
             float(want[-1]), last_g, float(got[-1])))
    assert band < 5e-4
    assert first < 1e-4
    assert float(want[-1]) < float(want[0])
    assert e_mean < 5e-3 and e_vol < 5e-3 and e_const < 5e-3
    assert max(e_lik) < 5e-3
    assert min(moved) > 1e-3                                  # the likelihood's parameters did train
    assert abs(last_g - float(want[-1])) < 5e-4 * max(1.0, abs(float(want[-1])))
    assert abs(last_g - float(got[-1])) < 2 * 5e-4 * max(1.0, abs(float(want[-1])))
    assert float((model_g.variational_strategy._variational_distribution.variational_mean.detach().cpu().double()
                  - ps[0]).abs().max()) < 5e-3
    eps = torch.randn(10, n, generator=torch.Generator().manual_seed(7))
    ref = R.pred_scale(ps[0], ps[1], eps.double(), ps[4:])
    f = model(x.to(DEV)).rsample(base_samples=eps.to(DEV))
    vol = lh(f).scale.mean(0).cpu().double()
    e_read = float((vol - ref).abs().max() / ref.abs().max())
    print("CVFIT readout %.2e" % e_read)
    assert e_read < 3e-2


def test_learn_gpcv_cv_batched_equals_single(monkeypatch):
    """3 series in one batched "cv" fit (a [3,1] likelihood, trained) == three single fits from the same draws of raw_a,
    raw_b, raw_c and of the readout's normals, as test_learn_gpcv_batched_equals_single asks of "exp": 2e-3 of max."""
    from volt_amd.train_utils import LearnGPCV
    n, iters = 200, 15
    Fs = torch.stack([_prices(n, 2019 + i)[0] for i in range(3)])
    x = (torch.arange(n, dtype=torch.float32) / 252).to(DEV)
    kw = dict(param="cv", K=1, train_likelihood=True)
    draws = torch.rand(3, 3, 1, generator=torch.Generator().manual_seed(23))      # [which of a,b,c][series][K]
    eps = torch.randn(10, 3, n, generator=torch.Generator().manual_seed(3)).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        queue = [draws[0], draws[1], draws[2]]
        monkeypatch.setattr(torch, "rand", lambda *a, **k: queue.pop(0).clone())
        monkeypatch.setattr(torch, "randn", lambda *a, **k: eps.clone())
        vb = LearnGPCV(x, Fs.to(DEV), train_iters=iters, **kw)
        assert vb.shape == (3, n) and not queue
        for i in range(3):
            queue = [draws[0][i], draws[1][i], draws[2][i]]
            monkeypatch.setattr(torch, "rand", lambda *a, **k: queue.pop(0).clone())
            monkeypatch.setattr(torch, "randn", lambda *a, **k: eps[:, i, :].clone())
            vi = LearnGPCV(x, Fs[i].to(DEV), train_iters=iters, **kw)
            err = float((vi - vb[i]).abs().max() / vb[i].abs().max())
            print("CVBATCH", i, f"{err:.2e}")
            assert err < 2e-3


def test_learn_gpcv_defaults_are_unchanged():
    """LearnGPCV / FitGPCV with no new keyword: the "exp" loop as before -- the same losses, bit for bit, as the loop spelled
    out over the public classes (what FitGPCV did before it had the keywords), and the likelihood has no parameters."""
    from volt_amd import gp
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import SingleTaskVariationalGP
    from volt_amd.train_utils import LR_GPCV, FitGPCV, LearnGPCV
    from volt_amd.variational import VariationalELBO, num_gauss_hermite_locs
    n, iters = 150, 8
    F, _ = _prices(n, 2030)
    x, Fd = (torch.arange(n, dtype=torch.float32) / 252).to(DEV), F.to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model, lik, losses = FitGPCV(x, Fd, train_iters=iters, graph=False)
        assert lik.param == "exp" and not list(lik.parameters())
        yy = GO.scaled_returns(x, Fd)
        lik2 = VolatilityGaussianLikelihood(param="exp")
        model2 = SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=lik2, use_piv_chol_init=False,
                                         mean_module=gp.ConstantMean(), covar_module=BMKernel(),
                                         learn_inducing_locations=False, use_whitened_var_strat=False)
        model2.initialize_variational_parameters(lik2, x, y=yy)
        opt = torch.optim.Adam([{"params": model2.parameters()}], lr=LR_GPCV)
        elbo = VariationalELBO(lik2, model2, n, combine_terms=True)
        want = []
        for _ in range(iters):
            opt.zero_grad(set_to_none=True)
            with num_gauss_hermite_locs(75):
                loss = -elbo(model2(x), yy)
                loss.backward()
            want.append(loss.detach())
            opt.step()
        assert torch.equal(torch.stack(losses), torch.stack(want))
        torch.manual_seed(4)
        v1 = LearnGPCV(x, Fd, train_iters=iters)
        torch.manual_seed(4)
        v2 = LearnGPCV(x, Fd, train_iters=iters, param="exp", K=1, train_likelihood=False)
        assert torch.equal(v1, v2) and tuple(v1.shape) == (n,)
