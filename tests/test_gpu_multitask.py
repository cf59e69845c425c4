"""MultitaskBMGP (voltron/models/BMGP.py:30-56) on the MI355X: the eigensolver, the Kronecker MLL and its five gradients,
the posterior, the opt-in on the batched models and the trainer -- against a dense fp64 restatement of the model.

The oracle below is the DEFINITION of the model, not the algebra of csrc/kron.hip: it builds the NT x NT covariance
K_x (x) K_t + I_N (x) diag(d) in gpytorch's interleaved order, takes log N(vec Y; vec mu, Sigma) / (N T) with a dense
Cholesky and differentiates it with torch autograd (fp64; on the CPU up to NT = 4096, on the GPU's torch above)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from volt_amd.synthetic import sde_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def va():
    assert torch.cuda.is_available()
    import volt_amd
    return volt_amd


# ------------------------------------------------------------------ the dense oracle
def oracle_parts(p, x, Y):
    """Everything in fp64 torch on the tensors' own device; p = dict of raw parameters (leaf tensors)."""
    N, T = Y.shape
    vol = torch.sigmoid(p["raw_vol"]).reshape(())
    Fm = p["covar_factor"].reshape(T, 1)
    Kt = Fm @ Fm.T + torch.diag(Fn.softplus(p["raw_var"]))
    d = Fn.softplus(p["raw_task_noises"]) + 1e-4 + Fn.softplus(p["raw_noise"]).reshape(()) + 1e-4
    M = torch.minimum(x[:, None], x[None, :])
    mu = -0.5 * vol ** 2 * x[:, None] * torch.diagonal(Kt)[None, :]
    return vol, Kt, d, M, mu


def oracle_mll(p, x, Y):
    """(mll, {name: gradient}) of log N(vec Y; vec mu, Sigma) / (N T)."""
    N, T = Y.shape
    devc = "cpu" if N * T <= 4096 else "cuda"
    q = {k: v.detach().to(devc, torch.float64).requires_grad_(True) for k, v in p.items()}
    xx, YY = x.to(devc, torch.float64), Y.to(devc, torch.float64)
    vol, Kt, d, M, mu = oracle_parts(q, xx, YY)
    S = torch.kron(vol * M, Kt) + torch.diag(d.repeat(N))
    r = (YY - mu).reshape(-1)
    L = torch.linalg.cholesky(S)
    a = torch.cholesky_solve(r[:, None], L)[:, 0]
    lp = -0.5 * (r @ a) - torch.log(torch.diagonal(L)).sum() - 0.5 * N * T * math.log(2 * math.pi)
    mll = lp / (N * T)
    mll.backward()
    return float(mll.detach()), {k: v.grad.detach().cpu() for k, v in q.items()}


def oracle_posterior(p, x, Y, xs):
    """Dense latent posterior of vec F* at xs [H]: (mean [H,T], cov [HT,HT]) in fp64."""
    N, T = Y.shape
    H = xs.shape[0]
    devc = "cpu" if N * T <= 4096 else "cuda"
    q = {k: v.detach().to(devc, torch.float64) for k, v in p.items()}
    xx, YY, xs = x.to(devc, torch.float64), Y.to(devc, torch.float64), xs.to(devc, torch.float64)
    vol, Kt, d, M, mu = oracle_parts(q, xx, YY)
    S = torch.kron(vol * M, Kt) + torch.diag(d.repeat(N))
    Ksx = torch.kron(vol * torch.minimum(xs[:, None], xx[None, :]), Kt)
    Kss = torch.kron(vol * torch.minimum(xs[:, None], xs[None, :]), Kt)
    L = torch.linalg.cholesky(S)
    r = (YY - mu).reshape(-1, 1)
    mus = -0.5 * vol ** 2 * xs[:, None] * torch.diagonal(Kt)[None, :]
    mean = mus + (Ksx @ torch.cholesky_solve(r, L)).reshape(H, T)
    cov = Kss - Ksx @ torch.cholesky_solve(Ksx.T.contiguous(), L)
    return mean.cpu(), cov.cpu()


def make_case(N, T, start, seed, dtype=torch.float32):
    """Grid x (from 0 or from dt), correlated log-vol paths Y [N,T] and random raw parameters (F of both signs)."""
    g = torch.Generator().manual_seed(seed)
    dt = 1.0 / 252
    x = (torch.arange(N, dtype=torch.float64) + (0 if start == 0 else 1)) * dt
    common = torch.cumsum(torch.randn(N, 1, generator=g, dtype=torch.float64), 0) * 0.05
    Y = -1.5 + common + torch.cumsum(torch.randn(N, T, generator=g, dtype=torch.float64), 0) * 0.03
    p = {
        "raw_vol": torch.randn(1, generator=g, dtype=torch.float64) * 0.5 - 1.0,
        "covar_factor": torch.randn(T, 1, generator=g, dtype=torch.float64) * 0.5,
        "raw_var": torch.randn(T, generator=g, dtype=torch.float64) - 1.0,
        "raw_task_noises": torch.randn(T, generator=g, dtype=torch.float64) - 3.0,
        "raw_noise": torch.randn(1, generator=g, dtype=torch.float64) - 4.0,
    }
    return ({k: v.to(dtype) for k, v in p.items()}, x.to(dtype), Y.to(dtype))


def build_model(p, x, Y):
    from volt_amd.gp import MultitaskGaussianLikelihood
    from volt_amd.models import MultitaskBMGP
    T = Y.shape[1]
    lh = MultitaskGaussianLikelihood(num_tasks=T).cuda()
    m = MultitaskBMGP(x.cuda(), Y.cuda(), lh).cuda()
    if x.dtype == torch.float64:
        m, lh = m.double(), lh.double()
        m.likelihood = lh
    with torch.no_grad():
        m.covar_module.data_covar_module.raw_vol.copy_(p["raw_vol"])
        m.covar_module.task_covar_module.covar_factor.copy_(p["covar_factor"])
        m.covar_module.task_covar_module.raw_var.copy_(p["raw_var"])
        lh.raw_task_noises.copy_(p["raw_task_noises"])
        lh.raw_noise.copy_(p["raw_noise"])
    return m, lh


def model_params(m, lh):
    return {"raw_vol": m.covar_module.data_covar_module.raw_vol, "covar_factor": m.covar_module.task_covar_module.covar_factor,
            "raw_var": m.covar_module.task_covar_module.raw_var, "raw_task_noises": lh.raw_task_noises,
            "raw_noise": lh.raw_noise}


# ------------------------------------------------------------------ eigensolver
def _eig_cases(T, rng):
    X = rng.standard_normal((3, T, T))
    spd = X @ X.transpose(0, 2, 1) + 0.1 * np.eye(T)
    u = rng.standard_normal(T)
    rank1 = np.outer(u, u) + 2.0 * np.eye(T)
    Q, _ = np.linalg.qr(rng.standard_normal((T, T)))
    cond = Q @ np.diag(np.logspace(0, -8, T)) @ Q.T
    cond = 0.5 * (cond + cond.T)
    return np.concatenate([spd, rank1[None], 3.0 * np.eye(T)[None], cond[None]])


@pytest.mark.parametrize("T", [1, 2, 3, 8, 31, 64])
def test_syev_small_eigenpairs(va, T):
    from volt_amd import ops
    S = _eig_cases(T, np.random.default_rng(T))
    lam, Q, info = ops.syev_small(torch.tensor(S, device="cuda"))
    lam, Q, info = lam.cpu().numpy(), Q.cpu().numpy(), info.cpu().numpy()
    assert (info >= 0).all(), info
    for b in range(S.shape[0]):
        nS = np.linalg.norm(S[b])
        assert np.linalg.norm(S[b] @ Q[b] - Q[b] * lam[b]) <= 1e-12 * nS, b
        assert np.linalg.norm(Q[b].T @ Q[b] - np.eye(T)) <= 1e-12, b
        ref = np.linalg.eigvalsh(S[b])
        # relative to the spectrum's scale: LAPACK's own small eigenvalues are accurate to eps * |S| only
        assert np.abs(lam[b] - ref).max() <= 1e-12 * np.abs(ref).max(), b
        assert (np.diff(lam[b]) >= 0).all()                  # ascending, as syev returns them


def test_syev_small_rejects_large_t(va):
    from volt_amd import ops
    with pytest.raises(ValueError, match="64"):
        ops.syev_small(torch.eye(65, dtype=torch.float64, device="cuda"))


# ------------------------------------------------------------------ the shared M
@pytest.mark.parametrize("N,T", [(399, 8), (1000, 16)])
def test_step_with_shared_m_is_bitwise_the_materialised_one(va, N, T):
    """The Kronecker step hands M to the existing step with batch stride 0 (ops.KRON_SHARED_K): the step must give
    bitwise what it gives on T materialised copies."""
    from volt_amd import ops
    assert ops.KRON_SHARED_K
    x = torch.arange(N, device="cuda", dtype=torch.float32) / 252.
    M = torch.minimum(x[:, None], x[None, :])
    g = torch.Generator(device="cuda").manual_seed(3)
    r = torch.randn(T, N, device="cuda", generator=g)
    s2 = torch.rand(T, device="cuda", generator=g) + 0.05
    o1, a1, i1 = (t.clone() for t in ops.mll_step(M.expand(T, N, N), r, s2, want_grad=True))
    o2, a2, i2 = (t.clone() for t in ops.mll_step(M.expand(T, N, N).contiguous(), r, s2, want_grad=True))
    assert torch.equal(i1, i2) and int(i1.abs().sum()) == 0
    assert torch.equal(o1, o2) and torch.equal(a1, a2)


# ------------------------------------------------------------------ MLL + gradients
# T = 64 at N = 128: the dense oracle's NT x NT fp64 autograd at N = 399 (25536^2) does not fit the library torch calls for
# it; NT = 8192 does (the Kronecker path itself runs T = 64 at N = 4096 in scripts/bench_multitask.py)
CASES = [(64, 1), (120, 3), (399, 8), (512, 16), (128, 64)]


@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("N,T", CASES)
def test_kron_mll_and_grads_vs_dense_oracle_fp32(va, N, T, start):
    from volt_amd.gp import ExactMarginalLogLikelihood
    p, x, Y = make_case(N, T, start, seed=100 * T + N + start)
    m, lh = build_model(p, x, Y)
    mll = ExactMarginalLogLikelihood(lh, m)
    out = mll(m(m.train_inputs[0]), m.train_targets)
    out.backward()
    ref, gref = oracle_mll(p, x.double(), Y.double())
    assert abs(float(out) - ref) <= 5e-5 * max(1.0, abs(ref)), (float(out), ref)
    for k, prm in model_params(m, lh).items():
        g = prm.grad.detach().cpu().double().reshape(gref[k].shape)
        assert float((g - gref[k]).abs().max()) <= 2e-3 * float(gref[k].abs().max()), (k, g, gref[k])


@pytest.mark.parametrize("start", [0, 1])
def test_kron_mll_and_grads_vs_dense_oracle_fp64(va, start):
    from volt_amd.gp import ExactMarginalLogLikelihood
    p, x, Y = make_case(399, 8, start, seed=7 + start, dtype=torch.float64)
    m, lh = build_model(p, x, Y)
    assert m.covar_module.task_covar_module.covar_factor.dtype == torch.float64
    mll = ExactMarginalLogLikelihood(lh, m)
    out = mll(m(m.train_inputs[0]), m.train_targets)
    assert out.dtype == torch.float64
    out.backward()
    ref, gref = oracle_mll(p, x, Y)
    assert abs(float(out) - ref) <= 1e-9 * max(1.0, abs(ref)), (float(out), ref)
    for k, prm in model_params(m, lh).items():
        g = prm.grad.detach().cpu().reshape(gref[k].shape)
        assert float((g - gref[k]).abs().max()) <= 1e-9 * max(1.0, float(gref[k].abs().max())), (k, g, gref[k])


def test_kron_mll_target_layout_and_task_limit(va):
    from volt_amd import ops
    from volt_amd.gp import ExactMarginalLogLikelihood, MultitaskGaussianLikelihood
    from volt_amd.models import MultitaskBMGP
    p, x, Y = make_case(40, 3, 1, seed=1)
    m, lh = build_model(p, x, Y)
    with pytest.raises(ValueError, match="N, T"):
        ExactMarginalLogLikelihood(lh, m)(m(m.train_inputs[0]), m.train_targets.t().contiguous())
    with pytest.raises(ValueError, match="64"):
        MultitaskBMGP(x.cuda(), torch.zeros(40, 65, device="cuda"), MultitaskGaussianLikelihood(65).cuda())
    with pytest.raises(ValueError, match="64"):
        ops.KronWorkspace(40, 65, torch.device("cuda"))


# ------------------------------------------------------------------ posterior
@pytest.mark.parametrize("H", [1, 8, 100])
@pytest.mark.parametrize("N,T", [(120, 3), (399, 8)])
def test_posterior_vs_dense_oracle(va, N, T, H):
    p, x, Y = make_case(N, T, 1, seed=N + T + H)
    m, lh = build_model(p, x, Y)
    m.eval()
    xs = x[-1] + (torch.arange(H, dtype=torch.float32) + 1) / 252.
    post = m(xs.cuda())
    mref, cref = oracle_posterior(p, x.double(), Y.double(), xs.double())
    mean = post.mean.detach().cpu().double()
    assert tuple(mean.shape) == (H, T)
    assert float((mean - mref).abs().max()) <= 2e-4 * max(1.0, float(mref.abs().max()))
    cov = post.covariance_matrix.cpu().double()
    assert float((cov - cref).abs().max()) <= 2e-4 * float(cref.abs().max())
    var = post.variance.cpu().double()
    assert float((var.reshape(-1) - torch.diagonal(cref)).abs().max()) <= 2e-4 * float(cref.abs().max())
    # a draw is mean + R z with R R' = cov (R[(h,t),(h',j)] = V[t,j] L_j[h,h'])
    V, L = post.root_blocks()
    V, L = V.cpu().double(), L.cpu().double()
    R = torch.einsum("tj,jhk->htkj", V, L).reshape(H * T, H * T)
    assert float((R @ R.T - cref).abs().max()) <= 2e-4 * float(cref.abs().max())
    z = torch.randn(H, T, generator=torch.Generator().manual_seed(H))
    s = post.sample(base_samples=z.cuda()).cpu().double()
    want = mean.reshape(-1) + R @ z.double().reshape(-1)
    assert float((s.reshape(-1) - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    assert tuple(post.sample(torch.Size((4,))).shape) == (4, H, T)


# ------------------------------------------------------------------ opt-in on the batched models
def test_batched_models_multitask_vol(va):
    from volt_amd.gp import ExactMarginalLogLikelihood, GaussianLikelihood
    from volt_amd.models import BMGP, MultitaskBMGP, VoltMagpie
    T, n, H = 4, 150, 6
    x, F, vol = sde_batch(T, n, seed=5)
    tx = torch.tensor(x, device="cuda")
    ty = torch.log(torch.tensor(F[:, 1:], device="cuda"))
    vp = torch.tensor(vol, device="cuda")
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    plain = VoltMagpie(tx, ty, GaussianLikelihood(batch_shape=torch.Size([T])).cuda(), vp, k=20)
    assert type(plain.vol_model) is BMGP                                         # the default is unchanged
    torch.manual_seed(0)
    m = VoltMagpie(tx, ty, GaussianLikelihood(batch_shape=torch.Size([T])).cuda(), vp, k=20, multitask_vol=True)
    assert isinstance(m.vol_model, MultitaskBMGP)
    assert float(m.vol_lh.noise) == pytest.approx(1e-3, rel=1e-5)
    assert tuple(m.vol_model.train_targets.shape) == (n, T)
    # VolMLL with the layouts the model was built with, against the oracle
    vm = m.vol_model
    p = {k: v.detach().cpu().double() for k, v in model_params(vm, m.vol_lh).items()}
    ref, _ = oracle_mll(p, tx.cpu().double(), vp.log().t().cpu().double())
    assert abs(float(m.VolMLL()) - ref) <= 5e-5 * max(1.0, abs(ref))
    # MeanPrediction: exp(posterior mean).T, and the prediction GeneratePrediction makes from it.  (On a batched VoltronGP:
    # batched VoltMagpie.GeneratePrediction does not take H test points -- its EWMA mean term has the train length --,
    # with or without the flag; the vol forecaster's wiring lives in models/_base.py, shared by both.)
    from volt_amd.models import VoltronGP
    torch.manual_seed(0)
    mv = VoltronGP(tx, ty, GaussianLikelihood(batch_shape=torch.Size([T])).cuda(), vp, multitask_vol=True)
    assert isinstance(mv.vol_model, MultitaskBMGP)
    torch.manual_seed(3)
    pred, pv = mv.MeanPrediction(test_x, return_vol=True)
    vm = mv.vol_model
    vm.eval()
    want = vm(test_x).mean.exp().t()
    assert tuple(pv.shape) == (T, H) and torch.allclose(pv, want, rtol=1e-6, atol=0)
    torch.manual_seed(3)
    assert torch.allclose(pred, mv.GeneratePrediction(test_x, pv), rtol=1e-6, atol=1e-6)
    pred_s, pv_s = mv.SamplePrediction(test_x, return_vol=True)
    assert tuple(pv_s.shape) == (T, H) and tuple(pred_s.shape) == (T, H) and bool(torch.isfinite(pred_s).all())
    # ... and the MLL of the opt-in vol model is what ExactMarginalLogLikelihood gives for it directly
    vm = m.vol_model
    vm.train()
    direct = ExactMarginalLogLikelihood(m.vol_lh, vm)(vm(vm.train_inputs[0]), vm.train_targets)
    assert float(direct) == pytest.approx(float(m.VolMLL()), rel=1e-6)


# ------------------------------------------------------------------ trainer
def _cpu_adam_oracle(p0, x, Y, iters, lr):
    """fp64 CPU Adam (torch.optim.Adam, the same hyper-parameters) on -oracle_mll."""
    q = {k: v.detach().double().clone().requires_grad_(True) for k, v in p0.items()}
    opt = torch.optim.Adam(list(q.values()), lr=lr)
    for _ in range(iters):
        opt.zero_grad()
        _, g = oracle_mll(q, x, Y)
        for k, v in q.items():
            v.grad = -g[k].reshape(v.shape)
        opt.step()
    return {k: v.detach() for k, v in q.items()}


def test_train_vol_model_multitask_matches_cpu_adam(va):
    from volt_amd.train_utils import LR_VOL, TrainVolModelMultitask
    T, n, iters = 8, 399, 30
    x, F, vol = sde_batch(T, n, seed=21)
    tx, vp = torch.tensor(x, device="cuda"), torch.tensor(vol, device="cuda")
    torch.manual_seed(5)
    m, lh = TrainVolModelMultitask(tx, vp, train_iters=iters, graph=False)
    torch.manual_seed(5)                                     # the same initial draws
    from volt_amd.gp import MultitaskGaussianLikelihood
    from volt_amd.models import MultitaskBMGP
    lh0 = MultitaskGaussianLikelihood(T).cuda()
    lh0.noise = 1e-3
    m0 = MultitaskBMGP(tx, vp.log().t(), lh0)
    p0 = {k: v.detach().cpu() for k, v in model_params(m0, lh0).items()}
    want = _cpu_adam_oracle(p0, tx.cpu().double(), vp.log().t().cpu().double(), iters, LR_VOL)
    for k, prm in model_params(m, lh).items():
        got = prm.detach().cpu().double().reshape(want[k].shape)
        assert float((got - want[k]).abs().max()) <= 2e-3, (k, got, want[k])


def test_train_vol_model_multitask_graph_equals_eager(va):
    """The whole iteration (prologue -> step -> epilogue -> fused Adam) captured once and replayed gives bitwise the
    losses of the same iteration run eagerly."""
    from volt_amd import gp
    from volt_amd.optim import FusedAdam
    from volt_amd.train_utils import LR_VOL
    T, n, iters, warm = 4, 300, 20, 3
    x, F, vol = sde_batch(T, n, seed=8)
    tx, vp = torch.tensor(x, device="cuda"), torch.tensor(vol, device="cuda")
    runs = {}
    for graph in (False, True):
        torch.manual_seed(9)
        lh = gp.MultitaskGaussianLikelihood(T).cuda()
        lh.noise = 1e-3
        from volt_amd.models import MultitaskBMGP
        m = MultitaskBMGP(tx, vp.log().t(), lh)
        opt = FusedAdam(list(m.parameters()), lr=LR_VOL)
        mll = gp.ExactMarginalLogLikelihood(lh, m)
        target = m.train_targets

        def it():
            loss = -mll(m(m.train_inputs[0]), target)
            loss.backward()
            return loss

        losses = []
        with gp.deferred_checks(immediate=True) as chk:
            nwarm = warm if graph else iters
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(nwarm):
                    opt.zero_grad(set_to_none=True)
                    losses.append(it().detach().clone())
                    opt.step()
            torch.cuda.current_stream().wait_stream(side)
            if graph:
                chk.immediate = False
                opt.zero_grad(set_to_none=True)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    static = it()
                    opt.step()
                for _ in range(warm, iters):
                    g.replay()
                    losses.append(static.detach().clone())
                assert chk.any_bad() == 0
        runs[graph] = torch.stack(losses).cpu()
    assert torch.equal(runs[False], runs[True]), (runs[False], runs[True])


def test_train_vol_model_multitask_recovers_correlation(va):
    """Seeded synthetic: four log-vol paths whose increments have correlation 0.9; the fitted K_t is positively correlated."""
    from volt_amd.train_utils import TrainVolModelMultitask
    T, n, rho = 4, 1000, 0.9
    rng = np.random.default_rng(2024)
    C = np.full((T, T), rho) + (1 - rho) * np.eye(T)
    inc = rng.standard_normal((n, T)) @ np.linalg.cholesky(C).T * 0.05
    logv = np.log(0.2) + np.cumsum(inc, 0)
    x = torch.arange(n, dtype=torch.float32, device="cuda") / 252.
    vp = torch.tensor(np.exp(logv).T, dtype=torch.float32, device="cuda")
    torch.manual_seed(1)
    m, lh = TrainVolModelMultitask(x, vp, train_iters=1000)
    Kt = m.covar_module.task_covar_module.covar_matrix.evaluate().detach().cpu().double()
    sd = torch.sqrt(torch.diagonal(Kt))
    corr = Kt / sd[:, None] / sd[None, :]
    off = corr[~torch.eye(T, dtype=torch.bool)]
    assert float(off.min()) > 0.5, corr
