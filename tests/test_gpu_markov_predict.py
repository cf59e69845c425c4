"""Prediction from the Markov GPCV away from its grid on the GPU (csrc/markov_predict.hip) against the fp64 loop
restatement tests/markov_predict_ref.py, from the two kernels up to model(test_x), the likelihood and PredictGPCV.

The cases are PR.GPU_CASES, the list the host tests tie to the dense definition.  Bounds (the chain family's): the plan's fp64 outputs 1e-10 of each quantity's scale (1e-8 from N = 4096 on: the scans' rounding
grows with N); the fp32 draws that plus 2^-23 |ref|, the output's own rounding.  The scan's boundaries: a thread's run is 4 points,
a wave's 256, the workgroup's chunk 2048; the draw stages 32 columns per chunk and 64 paths per wave."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import markov_predict_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
WORST = {}


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def gpu_plan(x, xs, v, mu, m, rho, gamma):
    from volt_amd import ops
    B = m.shape[0]
    return ops.markov_predict_plan(dev(x), dev(xs), dev(np.full(B, v)), dev(mu), dev(m), dev(rho), dev(gamma), jitter=PR.JITTER)


def note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def check_case(c):
    """Plan and draw of one case of PR.GPU_CASES through ops against the restatement, for the case's ``series``."""
    from volt_amd import ops
    x, xs, v, mu, m, rho, gamma = PR.case_inputs(c)
    N, B, Hn = c["N"], c["B"], xs.shape[0]
    plan = gpu_plan(x, xs, v, mu, m, rho, gamma)
    assert plan.info.tolist() == [0] * B
    got = {k: getattr(plan, k).cpu().numpy() for k in ("mean", "var_q", "var_p")}
    E = plan.E
    assert E <= 3 * Hn + 1 and plan.steps.tolist() == [E] * B
    f32 = PR.case_eps(c, E)
    draws = {p: ops.markov_predict_draw(plan, dev(f32), exp=c["exp"], part=p).cpu().numpy() for p in c["parts"]}
    t = PR.gpu_tol(N)
    for b in c["series"]:
        ref = PR.plan(x, xs, v, mu[b], m[b], rho[b], gamma[b])
        assert len(ref["steps"]) == E
        sc = max(np.abs(ref["var_q"]).max(), np.abs(ref["var_p"]).max())
        note("mean", np.abs(got["mean"][b] - PR.unsort(ref, ref["mean"])).max() / (t * max(1.0, np.abs(ref["mean"]).max())))
        note("var_q", np.abs(got["var_q"][b] - PR.unsort(ref, ref["var_q"])).max() / (t * sc))
        note("var_p", np.abs(got["var_p"][b] - PR.unsort(ref, ref["var_p"])).max() / (t * sc))
        for p, d in draws.items():
            r = PR.draw(ref, f32[b].astype(np.float64), part=p, exp=c["exp"])
            bound = t * max(1.0, np.abs(r).max()) + 2.0 ** -23 * np.abs(r)
            note("draw_" + p + ("_exp" if c["exp"] else ""), (np.abs(d[b] - r) / bound).max())
    bad = {k: w for k, w in WORST.items() if not w <= 1.0}
    assert not bad, (c, bad)


def teardown_module(module):
    for k, w in sorted(WORST.items()):
        print(f"markov_predict: largest error / bound of {k}: {w:.3e}")


@pytest.mark.parametrize("group", PR.GPU_GROUPS)
def test_plan_and_draw_match_the_restatement(group):
    """Every case of the shared list (tests/markov_predict_ref.py: N x B in full, the scan's edges, the point counts; families,
    path counts, x_0, v and regimes rotating inside), group by group."""
    for c in PR.GPU_CASES:
        if c["group"] == group:
            check_case(c)


def _fixture(N=130, B=3, family="mixed", regime="startup", v=0.2):
    x = PR.make_grid(N, PR.DT)
    m, rho, gamma, mu = PR.make_params(x, v, regime, B=B)
    return x, PR.make_points(x, family), v, mu, m, rho, gamma


def test_exact_identities():
    from volt_amd import ops
    x, _, v, mu, m, rho, gamma = _fixture()
    plan = gpu_plan(x, x, v, mu, m, rho, gamma)                        # `same`
    assert torch.equal(plan.mean.float(), dev(m))
    s = ops.markov_root_var(dev(rho), dev(gamma))
    assert torch.equal(plan.var_q, s) and bool((plan.var_p == 0).all())
    # duplicates: bitwise equal columns; any order of the points: the same numbers after un-permuting
    x, xs, v, mu, m, rho, gamma = _fixture()
    plan = gpu_plan(x, xs, v, mu, m, rho, gamma)
    eps = torch.randn(3, 70, plan.E, device=DEV)
    d = ops.markov_predict_draw(plan, eps)
    dup = [(i, j) for i in range(len(xs)) for j in range(i + 1, len(xs)) if xs[i] == xs[j]]
    assert len(dup) >= 4
    for i, j in dup:
        assert torch.equal(d[:, :, i], d[:, :, j]) and torch.equal(plan.mean[:, i], plan.mean[:, j])
    perm = np.random.default_rng(3).permutation(len(xs))
    plan2 = gpu_plan(x, xs[perm], v, mu, m, rho, gamma)
    d2 = ops.markov_predict_draw(plan2, eps)
    p = torch.as_tensor(perm, device=DEV)
    for a, b in ((plan.mean, plan2.mean), (plan.var_q, plan2.var_q), (plan.var_p, plan2.var_p)):
        assert torch.equal(a[:, p], b)
    # (equal points may swap places under another order: their columns are bitwise equal anyway)
    assert torch.equal(d[:, :, p], d2)


def _raw_plan(x, xs, v, mu, m, rho, gamma, pad=64, ws_fill=float("nan")):
    """volt_markov_predict_plan_f32 called directly, every output inside a NaN / -7 sentinel frame and the workspace NaN-filled."""
    from volt_amd import _lib
    L = _lib.lib()
    B, N = m.shape
    H = xs.shape[0]
    EM = 3 * H + 1
    f = lambda n: torch.full((n + 2 * pad,), float("nan"), dtype=torch.float64, device=DEV)
    i = lambda n: torch.full((n + 2 * pad,), -7, dtype=torch.int32, device=DEV)
    bufs = dict(mean=f(B * H), var_q=f(B * H), var_p=f(B * H), coef=f(B * EM * 3), code=i(B * EM), steps=i(B), info=i(B))
    nbytes = L.volt_markov_predict_workspace_bytes(B, N, H)
    ws = torch.full((nbytes // 8 + 64,), ws_fill, dtype=torch.float64, device=DEV)
    wptr = (ws.data_ptr() + 255) // 256 * 256
    ptr = lambda t: t.data_ptr() + pad * t.element_size()
    args = [dev(a) for a in (x, xs, np.full(B, v), mu, m, rho, gamma)]
    rc = L.volt_markov_predict_plan_f32(args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), PR.JITTER,
                                        *(a.data_ptr() for a in args[3:]), *(ptr(bufs[k]) for k in bufs), wptr, B, N, H,
                                        _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    for k, t in bufs.items():                                          # the frames are untouched
        edge = torch.cat([t[:pad], t[-pad:]])
        assert bool(edge.isnan().all()) if t.dtype == torch.float64 else bool((edge == -7).all()), k
    return {k: t[pad:-pad] for k, t in bufs.items()}


def test_sentinels_and_info_per_series():
    x, xs, v, mu, m, rho, gamma = _fixture()
    xs = np.sort(xs)
    B, H = m.shape[0], xs.shape[0]
    good = _raw_plan(x, xs, v, mu, m, rho, gamma)
    assert good["info"].tolist() == [0] * B and not bool(good["mean"].isnan().any())
    E = int(good["steps"][0])
    assert bool((good["code"].view(B, -1)[:, :E] % 8 > 0).all()) and bool((good["code"].view(B, -1)[:, E:] == 0).all())
    ref = gpu_plan(x, xs, v, mu, m, rho, gamma)
    assert torch.equal(good["mean"].view(B, H), ref._mean) and torch.equal(good["coef"].view(B, -1, 3), ref.coef)
    for h, value in ((0, -0.5), (4, float("nan")), (H - 1, float("inf")), (7, None)):
        bad = xs.copy().astype(np.float32)
        if value is None:
            bad[h] = bad[h - 3] * 0.5                                  # out of order
        else:
            bad[h] = value
        out = _raw_plan(x, bad, v, mu, m, rho, gamma)
        assert out["info"].tolist() == [-(h + 1)] * B and out["steps"].tolist() == [0] * B
        assert all(bool(out[k].isnan().all()) for k in ("mean", "var_q", "var_p", "coef"))
    # a NaN in rho: that series alone is NaN and reported, nothing faults
    rho2 = rho.copy()
    rho2[1, -1] = np.nan
    from volt_amd import ops
    plan = gpu_plan(x, xs, v, mu, m, rho2, gamma)
    assert plan.info.tolist() == [0, 1, 0]
    assert bool(plan.var_q[1].isnan().all()) and not bool(plan.var_q[[0, 2]].isnan().any())
    d = ops.markov_predict_draw(plan, torch.randn(B, 9, plan.E, device=DEV))
    assert bool(d[1].isnan().all()) and not bool(d[[0, 2]].isnan().any())
    # the draw of a failed plan is NaN; so is one whose rows of eps are shorter than the plan
    plan_bad = gpu_plan(x, np.where(np.arange(H) == 2, np.nan, xs), v, mu, m, rho, gamma)
    assert all(c < 0 for c in plan_bad.info.tolist())
    assert bool(ops.markov_predict_draw(plan_bad, torch.randn(B, 9, 3 * H + 1, device=DEV)).isnan().all())
    assert bool(ops.markov_predict_draw(ref, torch.randn(B, 9, ref.E - 1, device=DEV)).isnan().all())


def test_strided_inputs_repeats_and_graph_replay():
    from volt_amd import ops
    x, xs, v, mu, m, rho, gamma = _fixture(N=399, B=3)
    wide = lambda a: dev(np.repeat(a, 2, axis=1))[:, ::2]              # strided views of the same numbers
    args = (dev(x), dev(xs), dev(np.full(3, v)), dev(mu))
    plan = ops.markov_predict_plan(*args, dev(m), dev(rho), dev(gamma), jitter=PR.JITTER)
    plan_s = ops.markov_predict_plan(*args, wide(m), wide(rho), wide(gamma), jitter=PR.JITTER)
    E = plan.E
    eps = torch.randn(3, 130, 2 * E, device=DEV)
    first = ops.markov_predict_draw(plan, eps[:, :, :E].contiguous())
    assert torch.equal(plan.mean, plan_s.mean) and torch.equal(plan.coef, plan_s.coef)
    assert torch.equal(first, ops.markov_predict_draw(plan_s, eps[:, :, :E].contiguous()))
    assert torch.equal(first, ops.markov_predict_draw(plan, eps[:, :, :E]))       # a strided view of eps
    for _ in range(10):
        again = ops.markov_predict_plan(*args, dev(m), dev(rho), dev(gamma), jitter=PR.JITTER)
        assert torch.equal(again.coef, plan.coef) and torch.equal(again.var_q, plan.var_q) and torch.equal(again.code, plan.code)
        assert torch.equal(ops.markov_predict_draw(again, eps[:, :, :E]), first)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    ec = eps[:, :, :E].contiguous()
    with torch.cuda.stream(stream):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            out = ops.markov_predict_draw(plan, ec)
    torch.cuda.current_stream().wait_stream(stream)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)


# ------------------------------------------------------------------------------------------------------------ model level
def _model(N, B=None, regime="startup", v=0.2, seed=0):
    from volt_amd import gp
    from volt_amd.kernels import BMKernel
    from volt_amd.models import SingleTaskVariationalGP
    x = PR.make_grid(N, PR.DT)
    m, rho, gamma, mu = PR.make_params(x, v, regime, B=B or 1, seed=seed)
    kw = {"batch_shape": torch.Size([B])} if B else {}
    model = SingleTaskVariationalGP(init_points=dev(x).view(-1, 1), covar_module=BMKernel(**kw), mean_module=gp.ConstantMean(**kw),
                                    learn_inducing_locations=False, use_whitened_var_strat=False, prior_solver="markov").to(DEV)
    dist = model.variational_strategy._variational_distribution
    sq = (lambda a: dev(a)) if B else (lambda a: dev(a[0]))
    dist.variational_mean.data, dist.log_diag_precision_root.data, dist.coupling.data = sq(m), sq(rho), sq(gamma)
    model.mean_module.constant.data = dev(mu).reshape(model.mean_module.constant.shape)
    vol = model.covar_module.vol.detach().double().reshape(-1).cpu().numpy()
    return model, x, np.broadcast_to(vol, (B or 1,)), mu, m, rho, gamma


def test_model_mean_variance_rsample_and_covar_against_the_dense_definition():
    from volt_amd.variational import MIN_VARIANCE, MarkovPredictiveLatent
    model, x, vol, mu, m, rho, gamma = _model(130)
    xs = PR.make_points(x, "mixed", H=24)
    lat = model(dev(xs))
    assert isinstance(lat, MarkovPredictiveLatent) and lat.loc.shape == (24,) and not lat.loc.requires_grad
    mean_d, Cq, Cp = PR.dense_definition(x, xs, vol[0], mu[0], m[0], rho[0], gamma[0])
    C = Cq + Cp
    sc = np.abs(C).max()
    assert np.abs(lat.loc.cpu().double().numpy() - mean_d).max() <= 1e-10 + 2.0 ** -23 * np.abs(mean_d).max()
    assert np.abs(lat.variance.cpu().double().numpy() - np.maximum(np.diag(C), MIN_VARIANCE)).max() <= (1e-10 + 2.0 ** -23) * sc
    assert np.abs(lat._covar.cpu().double().numpy() - C).max() <= 1e-5 * sc      # (its own fp64 dense solve, rounded to fp32)
    assert torch.equal(model(dev(xs).view(-1, 1)).loc, lat.loc)
    # rsample is the restatement's linear map of its base samples, and its covariance is C
    E = lat.plan.E
    eps = torch.randn(7, E, device=DEV)
    ref = PR.draw(PR.plan(x, xs, vol[0], mu[0], m[0], rho[0], gamma[0]), eps.cpu().double().numpy())
    got = lat.rsample(base_samples=eps).cpu().double().numpy()
    assert got.shape == (7, 24) and (np.abs(got - ref) <= 1e-10 * max(1.0, np.abs(ref).max()) + 2.0 ** -23 * np.abs(ref)).all()
    unit = lat.rsample(base_samples=torch.eye(E, device=DEV)).double() - lat.plan.mean[0]      # rows: the map's columns
    assert np.abs((unit.mT @ unit).cpu().numpy() - C).max() <= 1e-5 * sc
    assert lat.rsample(torch.Size([4, 2])).shape == (4, 2, 24)
    with pytest.raises(ValueError, match="base_samples"):
        lat.rsample(base_samples=torch.zeros(3, E - 1, device=DEV))


@pytest.mark.parametrize("B", [None, 3])
def test_on_the_grid_the_prediction_is_q_u_itself_bitwise(B):
    """`same` at the model level: loc is variational_mean and variance is model(train_x).variance, bit for bit (the fp32 cast
    and the clamp included)."""
    from volt_amd.variational import MarkovPredictiveLatent, MarkovVariationalLatent
    model, x, *_ = _model(399, B=B)
    grid = model.variational_strategy.inducing_points
    on = model(grid)
    assert isinstance(on, MarkovVariationalLatent)
    lat = MarkovPredictiveLatent(model, grid.reshape(-1).clone())
    assert torch.equal(lat.loc, on.loc.detach()) and torch.equal(lat.variance, on.variance)
    rev = MarkovPredictiveLatent(model, grid.reshape(-1).flip(0))      # ... in any order
    assert torch.equal(rev.loc.flip(-1), on.loc.detach()) and torch.equal(rev.variance.flip(-1), on.variance)


def test_plan_replays_from_a_captured_graph():
    """volt_markov_predict_plan_f32 captured through the raw ABI: the replay rewrites every output bit for bit."""
    from volt_amd import _lib
    L = _lib.lib()
    x, xs, v, mu, m, rho, gamma = _fixture(N=399)
    xs = np.sort(xs)
    B, N, H = m.shape[0], m.shape[1], xs.shape[0]
    EM = 3 * H + 1
    want = _raw_plan(x, xs, v, mu, m, rho, gamma)
    f = lambda n: torch.zeros(n, dtype=torch.float64, device=DEV)
    i = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    bufs = dict(mean=f(B * H), var_q=f(B * H), var_p=f(B * H), coef=f(B * EM * 3), code=i(B * EM), steps=i(B), info=i(B))
    ws = torch.zeros(L.volt_markov_predict_workspace_bytes(B, N, H) // 8 + 64, dtype=torch.float64, device=DEV)
    wptr = (ws.data_ptr() + 255) // 256 * 256
    args = [dev(a) for a in (x, xs, np.full(B, v), mu, m, rho, gamma)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            rc = L.volt_markov_predict_plan_f32(args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), PR.JITTER,
                                                *(a.data_ptr() for a in args[3:]), *(t.data_ptr() for t in bufs.values()), wptr,
                                                B, N, H, _lib.stream_ptr())
    assert rc == 0
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(2):
        for t in bufs.values():
            t.fill_(5)
        ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k, t in bufs.items():
            assert torch.equal(t, want[k]), k


@pytest.mark.parametrize("param,K", [("exp", 1), ("cv", 1), ("cv", 5)])
def test_likelihood_of_the_prediction(param, K):
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    model, x, *_ = _model(130)
    lik = VolatilityGaussianLikelihood(param="exp") if param == "exp" else VolatilityGaussianLikelihood(K=K, param="cv").to(DEV)
    xs = dev(PR.make_points(x, "mixed", H=24))
    torch.manual_seed(5)
    scale = lik(model(xs), return_gaussian=False).scale
    torch.manual_seed(5)
    f = model(xs).rsample(torch.Size([scale.shape[0]]))
    assert scale.shape == f.shape and torch.equal(scale, lik(f, return_gaussian=False).scale) and bool((scale > 0).all())


def test_batched_equals_per_series():
    from volt_amd import ops
    B = 3
    model, x, vol, mu, m, rho, gamma = _model(130, B=B)
    xs = PR.make_points(x, "mixed", H=24)
    lat = model(dev(xs))
    assert lat.loc.shape == (B, 24) and lat.variance.shape == (B, 24)
    eps = torch.randn(5, B, lat.plan.E, device=DEV)
    f = lat.rsample(base_samples=eps)
    assert f.shape == (5, B, 24)
    for b in range(B):
        one = gpu_plan(x, xs, vol[b], mu[b:b + 1], m[b:b + 1], rho[b:b + 1], gamma[b:b + 1])
        assert torch.equal(one.mean[0].float(), lat.loc[b]) and torch.equal((one.var_q + one.var_p)[0].float().clamp_min(1e-6), lat.variance[b])
        assert torch.equal(ops.markov_predict_draw(one, eps[:, b].unsqueeze(0).contiguous())[0], f[:, b])


@pytest.mark.parametrize("T,N", [(1, 399), (3, 130)])
def test_predict_gpcv_after_a_fit(T, N):
    from volt_amd import train_utils
    from volt_amd.synthetic import sde_series
    train_x = torch.arange(N, dtype=torch.float32, device=DEV) / 252                 # (x_0 = 0: valid under the level's jitter)
    prices = torch.stack([torch.tensor(sde_series(N, 2021 + i)[0]) for i in range(T)]).to(DEV)      # [T, N + 1] prices
    model, lik, _ = train_utils.FitGPCV(train_x, prices[0] if T == 1 else prices, train_iters=40, solver="markov")
    grid = model.variational_strategy.inducing_points.reshape(-1)
    test_x = torch.cat([grid[-1] + torch.arange(1, 11, device=DEV) / 252, (grid[5:9] + grid[6:10]) / 2, grid[3:5]])
    torch.manual_seed(9)
    paths = train_utils.PredictGPCV(model, lik, test_x, nsample=12)
    assert paths.shape == ((12, 16) if T == 1 else (12, T, 16)) and bool(torch.isfinite(paths).all()) and bool((paths > 0).all())
    # against the restatement on the fitted parameters, for the same base samples
    lat = model(test_x)
    torch.manual_seed(9)
    eps = torch.randn(12, *((T,) if T > 1 else ()), lat.plan.E, device=DEV)
    dist = model.variational_strategy._variational_distribution
    g = lambda t: t.detach().double().reshape(T, -1).cpu().numpy()
    m, rho, gamma = g(dist.variational_mean), g(dist.log_diag_precision_root), g(dist.coupling)
    mu = model.mean_module.constant.detach().float().double().reshape(-1).cpu().numpy()
    vol = model.covar_module.vol.detach().float().double().reshape(-1).cpu().numpy()
    xg, xt = grid.double().cpu().numpy(), test_x.double().cpu().numpy()
    for b in range(T):
        ref = PR.plan(xg, xt, np.broadcast_to(vol, T)[b], np.broadcast_to(mu, T)[b], m[b], rho[b], gamma[b])
        e = (eps[:, b] if T > 1 else eps).cpu().double().numpy()
        want = np.maximum(np.exp(PR.draw(ref, e)), lik.MIN_SCALE)
        got = (paths[:, b] if T > 1 else paths).cpu().double().numpy()
        assert (np.abs(got - want) <= 1e-10 * max(1.0, np.abs(want).max()) + 4 * 2.0 ** -23 * np.abs(want)).all()   # (fp32 f, then fp32 exp)
        assert np.abs(lat.loc.reshape(T, -1)[b].cpu().double().numpy() - PR.unsort(ref, ref["mean"])).max() <= 1e-10 + 2.0 ** -23 * np.abs(ref["mean"]).max()


def test_peak_allocation_at_two_long_series():
    from volt_amd import ops
    B, N, H, S = 2, 65536, 100, 1000
    g = torch.Generator(device="cpu").manual_seed(1)
    x = (torch.arange(1, N + 1, dtype=torch.float32) / 252).to(DEV)
    m, rho, gamma = (torch.randn(B, N, generator=g).to(DEV) * s + o for s, o in ((0.5, -1.0), (0.3, 1.0), (0.2, -0.6)))
    xs = torch.cat([x[-1] + torch.arange(1, 51, device=DEV) / 252, (x[1000:1050] + x[1001:1051]) / 2])
    vol, mu = torch.full((B,), 0.2, device=DEV), torch.full((B,), -0.8, device=DEV)
    ops.markov_predict_plan(x[:64], xs[:4] * 0, vol, mu, m[:, :64], rho[:, :64], gamma[:, :64])        # (the library is loaded)
    eps = torch.randn(B, S, 3 * H + 1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    plan = ops.markov_predict_plan(x, xs, vol, mu, m, rho, gamma)
    out = ops.markov_predict_draw(plan, eps)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base - out.numel() * 4
    print(f"peak allocation above the inputs and the result at 2 x 65536, H = 100, S = 1000: {peak / 2 ** 20:.2f} MB")
    assert plan.info.tolist() == [0, 0] and bool(torch.isfinite(out).all())
    assert peak <= 8 * 2 ** 20


# ------------------------------------------------------------------------------------------------------------ multi-task
def _mt_model(N, T, regime):
    from volt_amd.kernels import BMKernel
    from volt_amd.models import MultitaskVariationalGP
    v = float(PR.f32(0.2))
    x = PR.make_grid(N, PR.DT)
    _, rho, gamma, _ = PR.make_params(x, v, regime)
    M = PR.f32(np.random.default_rng(N + T).normal(-1.0, 0.5, (N, T)))
    Lt, f, raw_var, c = PR.make_task_params(T)
    model = MultitaskVariationalGP(dev(x), num_tasks=T, covar_module=BMKernel(), prior_solver="markov").to(DEV)
    with torch.no_grad():
        for t, a in ((model.variational_mean, M), (model.log_diag_precision_root, rho[0]), (model.coupling, gamma[0]),
                     (model.variational_task_covar_root, Lt), (model.index_kernel.raw_var, raw_var)):
            t.copy_(dev(a))
        model.index_kernel.covar_factor.copy_(dev(f).reshape(T, 1))
        for t, mm in enumerate(model.mean_module.base_means):
            mm.constant.fill_(float(c[t]))
        model.data_kernel.vol = v
    v = float(model.data_kernel.vol.detach().float().double().reshape(-1)[0])     # (as the kernel's parameter holds it)
    return model, (x, v, c, M, rho[0], gamma[0], Lt, f, raw_var)


@pytest.mark.parametrize("N,T,regime", [(130, 3, "startup"), (399, 8, "random")])
def test_multitask_prediction(N, T, regime):
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.variational import MIN_VARIANCE, MultitaskMarkovPredictiveLatent
    model, (x, v, c, M, rho, gamma, Lt, f, raw_var) = _mt_model(N, T, regime)
    xs = PR.make_points(x, "mixed", H=24)
    lat = model(dev(xs))
    assert isinstance(lat, MultitaskMarkovPredictiveLatent) and lat.loc.shape == (24, T) and lat.event_shape == (24, T)
    maps = PR.mt_maps(x, xs, v, c, M, rho, gamma, Lt, f, raw_var)
    mean, var, Gk, Gb = maps
    assert np.abs(lat.loc.cpu().double().numpy() - mean).max() <= 1e-10 + 2.0 ** -23 * np.abs(mean).max()
    assert np.abs(lat.variance.cpu().double().numpy() - np.maximum(var, MIN_VARIANCE)).max() <= (1e-10 + 2.0 ** -23) * var.max()
    E = lat.plan.E
    eps = torch.randn(6, T, E, device=DEV)
    got = lat.rsample(base_samples=eps).cpu().double().numpy()
    ref = PR.mt_draw(maps, eps.cpu().numpy())
    # the two T x T products run in torch's fp32: 2 T products of fp32-rounded parts, summed in fp32, plus the mean
    flat = np.abs(eps.cpu().double().numpy()).transpose(0, 2, 1).reshape(6, -1)
    mass = (flat @ (np.abs(Gk) + np.abs(Gb)).T).reshape(6, 24, T) + np.abs(mean)[None]
    bound = 1e-10 * max(1.0, np.abs(ref).max()) + (2 * T + 4) * 2.0 ** -24 * mass
    print(f"multi-task {N} x {T}: largest rsample error / bound {(np.abs(got - ref) / bound).max():.3f}")
    assert got.shape == (6, 24, T) and (np.abs(got - ref) <= bound).all()
    if N <= 130:
        _, C = PR.mt_dense_definition(x, xs, v, c, M, rho, gamma, Lt, f, raw_var)
        assert np.abs(lat._covar.cpu().double().numpy() - C).max() <= 1e-5 * np.abs(C).max()
    assert lat.rsample(torch.Size([3])).shape == (3, 24, T)
    lik = VolatilityGaussianLikelihood(K=2, param="cv", batch_shape=torch.Size([T])).to(DEV)
    scale = lik(lat, return_gaussian=False).scale
    assert scale.shape[1:] == (24, T) and bool((scale > 0).all())


@pytest.mark.parametrize("H,S", [(19, 70), (32, 64), (33, 1)])
def test_draw_writes_nothing_outside_its_output(H, S):
    """volt_markov_predict_draw_f32 called directly with ``out`` inside a frame of sentinels (7.0: not a value a failed plan
    writes) and eps rows longer than the plan: the frame is untouched, columns of eps beyond the plan's steps are not read."""
    from volt_amd import _lib, ops
    x, _, v, mu, m, rho, gamma = _fixture()
    xs = np.sort(PR.make_points(x, "mixed", H=H))
    plan = gpu_plan(x, xs, v, mu, m, rho, gamma)
    H = plan.H                                                         # (the family's own count where H is its default)
    B, E, pad = m.shape[0], plan.E, 96
    eps = torch.randn(B, S, E + 5, device=DEV)
    want = ops.markov_predict_draw(plan, eps[:, :, :E].contiguous())
    eps[:, :, E:] = float("nan")
    buf = torch.full((B * S * H + 2 * pad,), 7.0, device=DEV)
    for off in (pad, pad + 1):                                         # 16-byte aligned output, and not
        buf.fill_(7.0)
        rc = _lib.lib().volt_markov_predict_draw_f32(plan._mean.data_ptr(), plan.coef.data_ptr(), plan.code.data_ptr(),
                                                     plan.steps.data_ptr(), eps.data_ptr(), buf.data_ptr() + 4 * off, B, S, H,
                                                     E + 5, 0, _lib.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((buf[:off] == 7.0).all()) and bool((buf[off + B * S * H:] == 7.0).all())
        assert torch.equal(buf[off:off + B * S * H].view(B, S, H), want)
