"""The copula-process ("cv") GPCV likelihood without a GPU: the fp64 reference of tests/gpcv_cv_ref.py is itself checked
(brute-force quadrature, torch.distributions, the product's own torch ``expected_log_prob``, central differences), and so
is the host-side surface of the feature: VariationalELBO accepts a "cv" likelihood for the single-task model, the
K = 1 start-up values against the reference's own code (tests/golden/gpcv_cv.npz), the batched ``forward`` broadcast,
the C entry's argument codes."""
import math

import numpy as np
import pytest
import torch
from torch.distributions import Normal

import gpcv_cv_ref as R
from oracle import gpcv_oracle as GO

D = torch.float64


def _case(n, K, seed, spread=1.0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=D)
    m = -1.2 + 0.4 * r(n)
    Lq = spread * (0.3 * torch.eye(n, dtype=D) + 0.1 * r(n, n) / math.sqrt(n)).tril() + torch.triu(r(n, n), 1)
    y = 0.3 * r(n)
    return m, Lq, y, R.draw_raw(K, seed)


@pytest.mark.parametrize("K,spread", [(1, 1.0), (5, 1.0), (8, 1.0), (5, 10.0)])
def test_ell_matches_brute_force_quadrature_and_normal_log_prob(K, spread):
    """(a) every node's log density against torch.distributions.Normal (the closed form is exact: 1e-12), and, where the
    clamp is out of reach of all but the outermost nodes (weights below 1e-20), 75-node Gauss-Hermite against a 6000-node
    trapezoid rule over +-12 sd: the integrand is analytic where it has weight, both rules converge far below 1e-6,
    which is what is asked.  At spread 10 the clamp puts a kink into the
    integrand of 4 nodes in 10; Gauss-Hermite then differs from the integral by about 1 % -- a property of the 75-node
    rule the reference fixes (train_utils.py:50), not of this restatement -- so only the per-node check applies."""
    n = 40
    m, Lq, y, raws = _case(n, K, 5 + K, spread)
    a, b, c = R.constrain(*raws)
    gx, gw = GO.gauss_hermite(75)
    e, clamped = R.ell(m, Lq, y, a, b, c, gx, gw)
    var = Lq.tril().pow(2).sum(-1)
    z = torch.linspace(-12, 12, 6001, dtype=D)
    f = m[:, None] + var.sqrt()[:, None] * z
    lp = Normal(torch.zeros_like(f), R.warp(f, a, b, c).clamp(min=1e-3)).log_prob(y[:, None])
    brute = torch.trapezoid(lp * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi), z, dim=-1).sum()
    if spread == 1.0:
        assert clamped < 0.06
        assert abs(float(e - brute)) <= 1e-6 * abs(float(brute)), (float(e), float(brute))
    else:
        assert clamped > 0.05
    # per node: the reference's closed form is Normal.log_prob
    locs = torch.sqrt(2.0 * var)[None] * gx[:, None] + m[None]
    lpn = Normal(torch.zeros_like(locs), R.warp(locs, a, b, c).clamp(min=1e-3)).log_prob(y[None])
    e2 = ((lpn * gw[:, None]).sum(0) / math.sqrt(math.pi)).sum()
    assert abs(float(e - e2)) <= 1e-12 * abs(float(e2))


@pytest.mark.parametrize("K", [1, 5])
def test_ell_matches_the_likelihoods_expected_log_prob(K):
    """(b) the product's torch ``expected_log_prob`` in fp64 sums to the reference's ell."""
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.variational import num_gauss_hermite_locs
    n = 50
    m, Lq, y, raws = _case(n, K, 11 + K)
    lik = VolatilityGaussianLikelihood(K=K, param="cv").double()
    with torch.no_grad():
        lik.raw_a.copy_(raws[0]), lik.raw_b.copy_(raws[1]), lik.raw_c.copy_(raws[2])
    gx, gw = GO.gauss_hermite(75)
    e, _ = R.ell(m, Lq, y, *R.constrain(*raws), gx, gw)
    q = type("Q", (), {"mean": m, "variance": Lq.tril().pow(2).sum(-1)})()
    with num_gauss_hermite_locs(75), torch.no_grad():          # (the nodes come in q(f)'s dtype: fp64 here)
        per_point = lik.expected_log_prob(y, q)
    assert tuple(per_point.shape) == (n,)
    assert abs(float(per_point.sum() - e)) <= 1e-10 * abs(float(e))


@pytest.mark.parametrize("K", [1, 5, 8])
def test_reference_gradients_match_central_differences(K):
    """(c) autograd of the reference against central differences for raw_a, raw_b, raw_c (and m)."""
    n = 30
    m, Lq, y, raws = _case(n, K, 21 + K)
    x = torch.arange(n, dtype=D) / 252
    Kx = GO.bm_cov(x, torch.tensor(0.2, dtype=D))
    gx, gw = GO.gauss_hermite(75)
    c0 = torch.tensor([-1.0], dtype=D)

    def val(raws_, m_=m):
        return R.elbo_terms(m_, Lq, c0, Kx, y, *raws_, gx, gw)["elbo"]

    ps = [r.clone().requires_grad_(True) for r in raws]
    mm = m.clone().requires_grad_(True)
    grads = torch.autograd.grad(val(ps, mm), ps + [mm])
    h = 1e-6
    for which in range(3):
        for k in range(K):
            up, dn = [r.clone() for r in raws], [r.clone() for r in raws]
            up[which][k] += h
            dn[which][k] -= h
            fd = float(val(up) - val(dn)) / (2 * h)
            assert abs(fd - float(grads[which][k])) <= 1e-6 * max(1.0, abs(fd)), (which, k, fd, float(grads[which][k]))
    for i in (0, n // 2, n - 1):
        up, dn = m.clone(), m.clone()
        up[i] += h
        dn[i] -= h
        fd = float(val(raws, up) - val(raws, dn)) / (2 * h)
        assert abs(fd - float(grads[3][i])) <= 1e-6 * max(1.0, abs(fd))


def _single(n=12, batch=None):
    from volt_amd import gp
    from volt_amd.kernels import BMKernel
    from volt_amd.models import SingleTaskVariationalGP
    kw = {"batch_shape": torch.Size([batch])} if batch else {}
    x = (torch.arange(n, dtype=torch.float32) + 1) / 252
    return SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=None, use_piv_chol_init=False,
                                   mean_module=gp.ConstantMean(**kw), covar_module=BMKernel(**kw),
                                   learn_inducing_locations=False, use_whitened_var_strat=False), x


def test_variational_elbo_accepts_cv_for_the_single_task_model_only():
    """(d) the default likelihood -- VolatilityGaussianLikelihood() is "cv", K = 5 -- builds a VariationalELBO over
    SingleTaskVariationalGP; the multi-task model keeps refusing it; without a device the step itself refuses."""
    from volt_amd._lib import VoltHipError
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import MultitaskVariationalGP
    from volt_amd.variational import VariationalELBO
    model, x = _single()
    lik = VolatilityGaussianLikelihood()
    assert lik.param == "cv" and tuple(lik.raw_a.shape) == (5,)
    elbo = VariationalELBO(lik, model, 12)
    with pytest.raises(VoltHipError):                       # CPU tensors: no fallback
        elbo(model(x), torch.zeros(12))
    with pytest.raises(NotImplementedError):
        VariationalELBO(VolatilityGaussianLikelihood(K=9), model, 12)
    mt = MultitaskVariationalGP(x, 3, covar_module=BMKernel())
    with pytest.raises(NotImplementedError):
        VariationalELBO(VolatilityGaussianLikelihood(), mt, 36)


TAGS = ["n60", "n90", "n80_wind"]


@pytest.mark.parametrize("name", TAGS)
def test_start_up_reference_matches_the_reference_code(golden, name):
    """(e), host half: tests/gpcv_cv_ref.init_variational_cv in fp64 equals the fp64 run of the reference's own
    ``initialize_variational_parameters`` ("cv", K = 1) recorded in gpcv_cv.npz, to rounding; and the reference's fp32 run
    recorded beside it stays inside the tolerance the product's fp32 start-up is held to (test_gpu_gpcv_cv.py, the one
    test_start_up_matches_the_reference_code uses for "exp": mean and constant 1e-5, covariance 2e-3) -- so that tolerance
    asks of the product what the reference's own code achieves in the same precision."""
    g = golden("gpcv_cv")
    t64 = lambda k: torch.tensor(g[f"{name}_f64_{k}"]).double()
    raw = t64("raw")
    f, S_root, c0 = R.init_variational_cv(t64("x"), t64("y"), (raw[0], raw[1], raw[2]))
    assert float((f - t64("mean")).abs().max()) < 1e-10
    assert abs(float(c0) - float(t64("const").reshape(-1)[0])) < 1e-12
    cov, cov_g = S_root @ S_root.mT, t64("chol") @ t64("chol").mT
    assert float((cov - cov_g).abs().max() / cov_g.abs().max()) < 1e-8
    t32 = lambda k: torch.tensor(g[f"{name}_f32_{k}"]).double()
    assert np.array_equal(g[f"{name}_f32_raw"], g[f"{name}_f64_raw"].astype(np.float32))
    assert float((t32("mean") - t64("mean")).abs().max()) < 1e-5
    assert abs(float(t32("const").reshape(-1)[0]) - float(t64("const").reshape(-1)[0])) < 1e-5
    cov32 = t32("chol") @ t32("chol").mT
    assert float((cov32 - cov_g).abs().max() / cov_g.abs().max()) < 2e-3


def test_likelihood_scale_matches_the_reference_code(golden):
    """``forward`` ("cv", K = 1 and 5, unbatched) against the reference's own, fp32 and fp64."""
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    g = golden("gpcv_cv")
    for K in (1, 5):
        raw = torch.tensor(g[f"lik{K}_raw"])
        lik = VolatilityGaussianLikelihood(K=K, param="cv")
        with torch.no_grad():
            lik.raw_a.copy_(raw[0]), lik.raw_b.copy_(raw[1]), lik.raw_c.copy_(raw[2])
        f = torch.tensor(g[f"lik{K}_f"])
        assert torch.allclose(lik.forward(f).scale, torch.tensor(g[f"lik{K}_scale"]), rtol=1e-6, atol=0)
        lik = lik.double()
        assert torch.allclose(lik.forward(f.double()).scale, torch.tensor(g[f"lik{K}_scale64"]), rtol=1e-13, atol=0)
        assert torch.allclose(R.warp(f.double(), *R.constrain(*raw.double())).clamp(min=1e-3),
                              torch.tensor(g[f"lik{K}_scale64"]), rtol=1e-12, atol=0)


def test_start_up_for_more_than_one_term_raises():
    """(f) the reference's ``y / trans_a`` broadcast has no meaning for K > 1; the multi-task model keeps refusing "cv"."""
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    model, x = _single()
    with pytest.raises(NotImplementedError, match="broadcast"):
        model.initialize_variational_parameters(VolatilityGaussianLikelihood(), x, y=torch.ones(12))
    with pytest.raises(NotImplementedError, match="broadcast"):
        model.initialize_variational_parameters(VolatilityGaussianLikelihood(K=2, param="cv"), x, y=torch.ones(12))


def test_batched_forward_broadcasts_parameters_per_series():
    """(g) batch_shape=[T]: series t of samples [S,T,N] meets parameter set t (parameters as [T,1,K]), for N != T and
    N == T alike; the unbatched forward is untouched."""
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    torch.manual_seed(0)
    T, K = 3, 4
    lik = VolatilityGaussianLikelihood(K=K, batch_shape=torch.Size([T]), param="cv")
    assert tuple(lik.raw_a.shape) == (T, K)
    for N in (7, T):
        f = torch.randn(5, T, N)
        got = lik.forward(f).scale
        assert tuple(got.shape) == (5, T, N)
        for t in range(T):
            one = VolatilityGaussianLikelihood(K=K, param="cv")
            with torch.no_grad():
                one.raw_a.copy_(lik.raw_a[t]), one.raw_b.copy_(lik.raw_b[t]), one.raw_c.copy_(lik.raw_c[t])
            assert torch.equal(got[:, t], one.forward(f[:, t]).scale)
    a, b, c = R.constrain(lik.raw_a[0].detach(), lik.raw_b[0].detach(), lik.raw_c[0].detach())
    one = VolatilityGaussianLikelihood(K=K, param="cv")
    with torch.no_grad():
        one.raw_a.copy_(lik.raw_a[0]), one.raw_b.copy_(lik.raw_b[0]), one.raw_c.copy_(lik.raw_c[0])
    f = torch.randn(6, 9)
    want = (((b * f.unsqueeze(-1) + c).exp() + 1).log() * a).sum(-1).clamp(min=1e-3)
    assert torch.equal(one.forward(f).scale, want)


def test_trainer_keywords_are_keyword_only_with_todays_defaults():
    import inspect
    from volt_amd import train_utils
    for fn in (train_utils.FitGPCV, train_utils.LearnGPCV):
        ps = inspect.signature(fn).parameters
        for name, default in (("param", "exp"), ("K", 1), ("train_likelihood", False)):
            assert ps[name].kind == inspect.Parameter.KEYWORD_ONLY and ps[name].default == default


def test_cv_entry_argument_codes_without_a_device():
    """Kc outside 1..8 (VOLT_GPCV_CV_K_MAX) and null pointers return negative argument codes before anything is launched."""
    from volt_amd import _lib, ops
    L = _lib.lib()
    assert "volt_gpcv_cv_workspace_bytes" in _lib.EXPORTS and "volt_gpcv_cv_step_f32" in _lib.EXPORTS
    assert ops.GPCV_CV_K_MAX == 8
    base = L.volt_gpcv_workspace_bytes(2, 300, 1)
    assert L.volt_gpcv_cv_workspace_bytes(2, 300, 1, 0) == 0 and L.volt_gpcv_cv_workspace_bytes(2, 300, 1, 9) == 0
    assert L.volt_gpcv_cv_workspace_bytes(0, 300, 1, 5) == 0
    assert L.volt_gpcv_cv_workspace_bytes(2, 300, 1, 5) > base > 0
    p = 256                                                   # never dereferenced: validation comes first
    args = lambda **kw: [kw.get("K", p), 300, 90000, 1e-3, p, p, p, p, kw.get("abc", p), kw.get("Kc", 5), p, p, 75, 1e-6, 1e-3,
                         1.0, 1.0, p, p, p, p, None, kw.get("gabc", p), p, kw.get("ws", p), 2, kw.get("N", 300), 0, None]
    assert L.volt_gpcv_cv_step_f32(*args(Kc=0)) == -10
    assert L.volt_gpcv_cv_step_f32(*args(Kc=9)) == -10
    assert L.volt_gpcv_cv_step_f32(*args(abc=None)) == -9
    assert L.volt_gpcv_cv_step_f32(*args(gabc=None)) == -23
    assert L.volt_gpcv_cv_step_f32(*args(K=None)) == -1
    assert L.volt_gpcv_cv_step_f32(*args(ws=8)) == -25
    assert L.volt_gpcv_cv_step_f32(*args(N=0)) == -27
    with pytest.raises(_lib.VoltHipError):
        ops.gpcv_cv_step(torch.eye(4)[None], torch.zeros(1, 4), torch.zeros(1, 4), torch.eye(4)[None], torch.zeros(1, 4),
                         torch.ones(1, 3, 1), torch.zeros(3), torch.zeros(3))
