"""The one-sweep posterior of the Brownian-motion vol forecaster on the MI355X (posterior="sweep"):
volt_bm_post_* (csrc/bm.hip) and ops.bm_post against the fp64 restatement of tests/bm_post_ref.py, memory safety and bitwise
repeats, the beyond-the-grid identities, the failure codes, BMGP / MultitaskBMGP(posterior="sweep") against the dense fp64
posterior and against posterior="solve", the models and the stocks driver, and the memory at N = 65536.  The restatement
is checked against dense fp64 LAPACK in tests/test_bm_post_host.py, where the negative controls for these bounds also live."""
import functools
import warnings

import numpy as np
import pytest
import torch

import bm_chain_ref as chain
import bm_post_ref as ref

pytestmark = pytest.mark.gpu

NOISES = (1e-3, 1e-1, 0.69)
BMAX = 65


def f64_tol(n):
    return 1e-10 if n <= 1024 else 1e-8           # the chain kernels' gates (tests/test_gpu_bm_linear.py)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a)).to(dtype).cuda()


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(n, H, own, B=BMAX):
    """fp32-representable inputs (as float64 arrays) and the restatement's forms for B series: vol 0.05 .. 0.9, the noise
    level NOISES[b % 3], one irregular grid (from dt at an odd n, from 0 at an even n; ``own``: every series a stretched copy of
    it, re-rounded), the mixed
    test points of the host test, sorted.  Computed once; the series are independent, so the first B rows are the case of B."""
    rng = np.random.default_rng(7 * n + H)
    x = f32(chain.grids(n, rng)["irregular_dt" if n % 2 else "irregular_zero"])
    if own:
        x = f32(x[None, :] * (1.0 + 0.25 * np.arange(B)[:, None] / B))
    assert (np.diff(x, axis=-1) > 0).all() and (x[..., 0] >= 0).all()
    vol = f32(rng.uniform(0.05, 0.9, B))
    s2 = f32(np.array([NOISES[b % 3] for b in range(B)]))
    r = f32(np.cumsum(rng.standard_normal((B, n)) * 0.05, axis=1) - 2.0)
    xs = np.sort(f32(ref.test_points(x if not own else x[0], H, rng)))
    out, info = ref.post_forms_ref(x, vol, s2, r, xs)
    assert not info.any()
    for a in (x, vol, s2, r, xs, out):
        a.setflags(write=False)
    return x, vol, s2, r, xs, out


def check_forms(got, want, vol, r, xs, n):
    """err <= tol * scale per series: max |r| for m (row 0), vol max xi for p and q.  Returns the largest err / bound."""
    tol = f64_tol(n)
    scale = np.stack([np.abs(r).max(1), vol * xs.max(), vol * xs.max()], axis=1)[:, :, None]
    err = np.abs(got - want)
    bound = tol * scale + 0.0 * err
    assert (err <= bound).all(), (np.argwhere(err > bound)[:4], (err / np.maximum(bound, 1e-300)).max())
    return float((err / np.maximum(bound, 1e-300)).max())


SHAPES = [(1, 1, 1), (2, 3, 2), (3, 65, 20), (63, 1, 63), (64, 3, 64), (65, 65, 65), (129, 3, 130), (399, 65, 20), (399, 1, 130)]


# ------------------------------------------------------------------------------------------------ 1: ops.bm_post
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("own", [False, True], ids=["shared", "own"])
@pytest.mark.parametrize("n,B,H", SHAPES)
def test_bm_post_matches_the_restatement(n, B, H, own, dtype):
    from volt_amd import ops
    x, vol, s2, r, xs, want = case(n, H, own)
    xx = x[:B] if own else x
    out, info = ops.bm_post(dev(xx, dtype), dev(xs, dtype), dev(vol[:B], dtype), dev(s2[:B], dtype), dev(r[:B], dtype))
    assert out.dtype == torch.float64 and tuple(out.shape) == (B, 3, H) and info.dtype == torch.int32 and not info.any()
    worst = check_forms(out.cpu().numpy(), want[:B], vol[:B], r[:B], xs, n)
    print(f"bm_post N = {n} B = {B} H = {H} {'own' if own else 'shared'} {dtype}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_bm_post_two_long_series(dtype):
    from volt_amd import ops
    n, B, H = 4096, 2, 20
    x, vol, s2, r, xs, want = case(n, H, False, B=B)
    out, info = ops.bm_post(dev(x, dtype), dev(xs, dtype), dev(vol, dtype), dev(s2, dtype), dev(r, dtype))
    assert not info.any()
    print(f"bm_post 2 x {n} {dtype}: largest error / bound {check_forms(out.cpu().numpy(), want, vol, r, xs, n):.3f}")


# ------------------------------------------------------------------------------------------------ 2: memory safety, repeats
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,B,H", [(1, 1, 1), (65, 3, 65), (399, 65, 20), (63, 5, 130)])
def test_bm_post_writes_nothing_past_its_buffers_and_repeats_bitwise(n, B, H, dtype):
    """NaN / -77 sentinels behind out and info survive; the per-series grids are a strided view inside a NaN-filled buffer, so
    a read outside a series' row shows; ten runs agree bit for bit.  ops.bm_post on the same strided view gives the same bits."""
    from volt_amd import _lib, ops
    x, vol, s2, r, xs, want = case(n, H, True)
    guard, pad = 64, 5
    xbuf = torch.full((B, n + 2 * pad), float("nan"), dtype=dtype, device="cuda")
    xbuf[:, pad:pad + n] = dev(x[:B], dtype)
    xv = xbuf[:, pad:pad + n]
    obuf = torch.full((B * 3 * H + guard,), float("nan"), dtype=torch.float64, device="cuda")
    ibuf = torch.full((B + guard,), -77, dtype=torch.int32, device="cuda")
    xsd, vd, sd, rd = dev(xs, dtype), dev(vol[:B], dtype), dev(s2[:B], dtype), dev(r[:B], dtype)
    fn = _lib.lib().volt_bm_post_f32 if dtype == torch.float32 else _lib.lib().volt_bm_post_f64

    def run():
        obuf[:B * 3 * H].fill_(float("nan"))
        _lib.check(fn(xv.data_ptr(), xv.stride(0), xsd.data_ptr(), vd.data_ptr(), sd.data_ptr(), rd.data_ptr(), obuf.data_ptr(),
                      ibuf.data_ptr(), B, n, H, _lib.stream_ptr()), "volt_bm_post")
        return obuf[:B * 3 * H].view(B, 3, H).clone(), ibuf[:B].clone()

    first, info = run()
    assert not info.any()
    check_forms(first.cpu().numpy(), want[:B], vol[:B], r[:B], xs, n)
    for _ in range(9):
        o, i = run()
        assert torch.equal(o, first) and torch.equal(i, info)
    assert torch.isnan(obuf[B * 3 * H:]).all() and bool((ibuf[B:] == -77).all())
    o, i = ops.bm_post(xv, xsd, vd, sd, rd)
    assert torch.equal(o, first) and torch.equal(i, info)


# ------------------------------------------------------------------------------------------------ 3: beyond the grid
@pytest.mark.parametrize("n", [65, 399])
def test_beyond_the_grid_p_is_q_and_both_are_the_vk_forms(n):
    """Test points past x_{N-1}: every column is k = v x, so p = q bit for bit, and p, m are rho = V'A^-1 V, tau = V'A^-1 r of
    ops.vk_forms(V = v x, jitter = s) to 1e-12 relative."""
    from volt_amd import ops
    x, vol, s2, r, _, _ = case(n, 20, False)
    B = 6
    xs = x[-1] * (1.0 + np.array([1e-12, 1e-6, 0.01, 0.01, 0.5, 7.0]))
    out, info = ops.bm_post(dev(x, torch.float64), dev(xs, torch.float64), dev(vol[:B], torch.float64),
                            dev(s2[:B], torch.float64), dev(r[:B], torch.float64))
    assert not info.any()
    assert torch.equal(out[:, 1], out[:, 2])
    assert bool((out[:, :, 1:] == out[:, :, :1]).all())                          # and the same at every such point
    worst = 0.0
    for b in range(B):
        forms, finfo = ops.vk_forms(dev(vol[b] * x, torch.float64), float(s2[b]), dev(r[b:b + 1], torch.float64))
        assert not finfo.any()
        rho, tau = float(forms[0, 0]), float(forms[0, 1])
        ep, em = abs(float(out[b, 1, 0]) - rho) / abs(rho), abs(float(out[b, 0, 0]) - tau) / abs(tau)
        worst = max(worst, ep, em)
        assert ep <= 1e-12 and em <= 1e-12, (b, ep, em)
    print(f"beyond the grid N = {n}: largest relative difference from vk_forms {worst:.2e} (bound 1e-12)")


# ------------------------------------------------------------------------------------------------ 4: failure codes
def test_bm_post_info():
    from volt_amd import ops
    n, B, H = 64, 3, 130
    x, vol, s2, r, xs, want = case(n, H, False)
    assert x[0] == 0.0 and xs[9] > 0                                             # (n even: the grid from 0)
    D = torch.float64
    args = lambda s, t: (dev(x, D), dev(t, D), dev(vol[:B], D), dev(s, D), dev(r[:B], D))
    s = s2[:B].copy()
    s[1] = 0.0                                                                   # d_0 = v x_0 + s = 0
    out, info = ops.bm_post(*args(s, xs))
    assert info.tolist() == [0, 1, 0]
    assert torch.isnan(out[1]).all() and torch.isfinite(out[0]).all() and torch.isfinite(out[2]).all()
    check_forms(out[[0, 2]].cpu().numpy(), want[[0, 2]], vol[[0, 2]], r[[0, 2]], xs, n)
    s[1] = -1.0
    out, info = ops.bm_post(*args(s, xs))
    assert info[0] == 0 and info[1] > 0 and info[2] == 0 and torch.isnan(out[1]).all()
    for h, val in ((0, -1e-3), (5, float("nan")), (7, float("inf")), (10, None), (100, None), (129, float("nan"))):
        t = xs.copy()
        t[h] = t[h - 1] * 0.5 if val is None else val                            # None: smaller than its predecessor
        assert val is not None or t[h] < t[h - 1]
        out, info = ops.bm_post(*args(s2[:B], t))
        assert info.tolist() == [-(h + 1)] * B, (h, info.tolist())
        assert torch.isnan(out).all()                                            # every block's rows, not only the bad point's


def test_bm_post_validates_shapes():
    from volt_amd import ops
    x, xs, v, r = (torch.ones(s, device="cuda") for s in ((9,), (4,), (2,), (2, 9)))
    with pytest.raises(ValueError):
        ops.bm_post(x, xs, v, v, r[0])
    with pytest.raises(ValueError):
        ops.bm_post(x[:7], xs, v, v, r)
    with pytest.raises(ValueError):
        ops.bm_post(r[:1], xs, v, v, r)
    with pytest.raises(ValueError):
        ops.bm_post(x, xs.reshape(2, 2), v, v, r)


# ------------------------------------------------------------------------------------------------ 5: the models
def _bmgp(x, y, dtype, posterior):
    from volt_amd.gp import GaussianLikelihood
    from volt_amd.models import BMGP
    bs = torch.Size(y.shape[:-1])
    lh = GaussianLikelihood(batch_shape=bs).cuda().to(dtype)
    m = BMGP(dev(x, dtype), dev(y, dtype), lh, solver="linear", posterior=posterior).cuda().to(dtype)
    with torch.no_grad():
        if len(bs):
            m.covar_module.raw_vol.copy_(torch.linspace(-1.5, 0.5, bs[0], dtype=dtype).reshape(-1, 1))
            lh.raw_noise.copy_(torch.linspace(-3.0, 0.0, bs[0], dtype=dtype).reshape(-1, 1))
        else:
            m.covar_module.raw_vol.fill_(-0.7)
            lh.raw_noise.fill_(-2.0)
    return m.eval(), lh


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [20, 65])
def test_bmgp_sweep_posterior(H, dtype):
    """The shapes and bounds of tests/test_gpu_bm_linear.py::test_bmgp_linear_posterior on posterior="sweep", the test points
    shuffled (and, at H = 65, with xi = 0, a grid point and a duplicate among them): against the fp64 dense posterior 1e-9 of
    scale (fp64 model) / 8 x 2^-24 max |y|, max K_** (fp32 model: the residual's three roundings and the output's one pass
    through a smoother of gain <= 1; the covariance sees only the output's rounding).  Against posterior="solve": the sum of
    the two routes' bounds, each being gated against the same dense posterior."""
    n, T = 399, 3
    x = f32(chain.grids(n)["uniform_dt"])
    y = f32(np.cumsum(np.random.default_rng(8).standard_normal((T, n)) * 0.05, axis=1) - 2.0)
    inside = 0.5 * (x[10:10 + H // 2] + x[11:11 + H // 2]) if H > 20 else 0.5 * (x[200:205] + x[201:206])
    xs = f32(np.concatenate([inside, x[-1] + (1 + np.arange(H - len(inside))) / 252.0]))
    if H > 20:
        xs[:3] = 0.0, x[37], xs[5]
    xs = xs[np.random.default_rng(H).permutation(H)]
    worst = [0.0, 0.0, 0.0, 0.0]
    for yy in (y, y[1]):
        m, lh = _bmgp(x, yy, dtype, "sweep")
        ms, _ = _bmgp(x, yy, dtype, "solve")
        post, posts = m(dev(xs, dtype)), ms(dev(xs, dtype))
        vol = m.covar_module.vol.detach().double().cpu().reshape(-1)
        noise = lh.noise.detach().double().cpu().reshape(-1)
        y2 = np.atleast_2d(yy)
        assert post.mean.dtype == dtype and tuple(post.mean.shape) == tuple(yy.shape[:-1]) + (H,)
        assert tuple(post.covariance_matrix.shape) == tuple(yy.shape[:-1]) + (H, H)
        mean, cov = post.mean.double().cpu().reshape(-1, H), post.covariance_matrix.double().cpu().reshape(-1, H, H)
        smean, scov = posts.mean.double().cpu().reshape(-1, H), posts.covariance_matrix.double().cpu().reshape(-1, H, H)
        assert torch.equal(cov, cov.mT)
        for t in range(y2.shape[0]):
            wm, wc = chain.dense_posterior(x, float(vol[t]), float(noise[t]), y2[t], xs)
            if dtype == torch.float64:
                mtol, ctol = 1e-9 * np.abs(wm).max(), 1e-9 * np.abs(wc).max()
            else:
                mtol, ctol = 8 * 2.0 ** -24 * np.abs(y2[t]).max(), 8 * 2.0 ** -24 * float(vol[t]) * xs.max()
            em, ec = np.abs(mean[t].numpy() - wm).max(), np.abs(cov[t].numpy() - wc).max()
            sm, sc = float((mean[t] - smean[t]).abs().max()), float((cov[t] - scov[t]).abs().max())
            worst = [max(a, b) for a, b in zip(worst, (em / mtol, ec / ctol, sm / (2 * mtol), sc / (2 * ctol)))]
            print(f"H = {H} {dtype} series {t}: |sweep - dense fp64| / bound  mean {em / mtol:.3f}  cov {ec / ctol:.3f};  "
                  f"|sweep - solve| / bound  mean {sm / (2 * mtol):.3f}  cov {sc / (2 * ctol):.3f}")
            assert em <= mtol and ec <= ctol, (t, em, mtol, ec, ctol)
            assert sm <= 2 * mtol and sc <= 2 * ctol, (t, sm, mtol, sc, ctol)
        if H == 20:                                                              # (H = 65 holds xi = 0 and a duplicate: singular)
            draw = post.sample(torch.Size((4,)))                                 # batched, then one series
            assert tuple(draw.shape) == (4,) + tuple(post.mean.shape) and torch.isfinite(draw).all()
    print(f"BMGP sweep H = {H} {dtype}: largest error / bound {max(worst):.3f}")


def test_bmgp_sweep_names_a_bad_test_point():
    from volt_amd.gp import NanError, NotPSDError
    x = f32(chain.grids(65)["uniform_dt"])
    m, lh = _bmgp(x, np.zeros(65), torch.float32, "sweep")
    xs = torch.tensor([0.5, 0.1, -0.2, 0.3], device="cuda")
    with pytest.raises(ValueError, match="test point 2"):
        m(xs)
    xs[2] = float("nan")
    with pytest.raises(ValueError, match="test point 2"):
        m(xs)
    xs[2] = 0.2
    with torch.no_grad():
        lh.raw_noise.fill_(float("nan"))
    with pytest.raises(NanError) as err:
        m(xs)
    assert not isinstance(err.value, NotPSDError)


MT_CASES = [(120, 3, 1, 0), (120, 3, 8, 1), (120, 3, 100, 0), (399, 8, 8, 0), (399, 8, 100, 1)]


@pytest.mark.parametrize("N,T,H,start", MT_CASES)
def test_multitask_sweep_posterior_vs_dense_oracle(N, T, H, start):
    """tests/test_gpu_multitask_linear.py::test_linear_posterior_vs_dense_oracle's checks and bound (2e-4) on
    posterior="sweep", the test points shuffled, two of them inside the grid and one on it; and against "solve"."""
    from test_gpu_multitask import make_case, model_params, oracle_posterior
    from volt_amd.gp import MultitaskGaussianLikelihood
    from volt_amd.models import MultitaskBMGP
    p, x, Y = make_case(N, T, start, seed=N + T + H)
    posts = {}
    xs = x[-1] + (torch.arange(H, dtype=torch.float32) + 1) / 252.
    if H >= 8:
        xs[:3] = torch.stack([0.5 * (x[40] + x[41]), x[17], 0.5 * (x[5] + x[6])])
    xs = xs[torch.randperm(H, generator=torch.Generator().manual_seed(H))]
    for posterior in ("sweep", "solve"):
        lh = MultitaskGaussianLikelihood(num_tasks=T).cuda()
        m = MultitaskBMGP(x.cuda(), Y.cuda(), lh, solver="linear", posterior=posterior).cuda()
        with torch.no_grad():
            for k, prm in model_params(m, lh).items():
                prm.copy_(p[k])
        posts[posterior] = m.eval()(xs.cuda())
    post = posts["sweep"]
    mref, cref = oracle_posterior(p, x.double(), Y.double(), xs.double())
    mean = post.mean.detach().cpu().double()
    assert tuple(mean.shape) == (H, T)
    cov = post.covariance_matrix.cpu().double()
    em = float((mean - mref).abs().max()) / max(1.0, float(mref.abs().max()))
    ec = float((cov - cref).abs().max()) / float(cref.abs().max())
    sm = float((mean - posts["solve"].mean.cpu().double()).abs().max()) / max(1.0, float(mref.abs().max()))
    sc = float((cov - posts["solve"].covariance_matrix.cpu().double()).abs().max()) / float(cref.abs().max())
    print(f"multitask sweep {N} x {T} H = {H}: / dense fp64 oracle  mean {em:.2e}  cov {ec:.2e};  / solve  mean {sm:.2e}  "
          f"cov {sc:.2e}  (bound 2e-4)")
    assert em <= 2e-4 and ec <= 2e-4
    assert sm <= 4e-4 and sc <= 4e-4                                             # each route within 2e-4 of the same oracle
    var = post.variance.cpu().double()
    assert float((var.reshape(-1) - torch.diagonal(cref)).abs().max()) <= 2e-4 * float(cref.abs().max())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                          # (a jittered pivot of an fp32 block is not this test's)
        draw = post.sample(torch.Size((4,)))
    assert tuple(draw.shape) == (4, H, T) and torch.isfinite(draw).all()


# ------------------------------------------------------------------------------------------------ 6: models and drivers
def _count_bm_post(monkeypatch):
    """A spy on ops.bm_post (the models call it through the module): the list grows by one per launch of the sweep."""
    from volt_amd import ops
    calls, real = [], ops.bm_post

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "bm_post", spy)
    return calls


def test_volt_magpie_and_volt_forecast_with_the_sweep_posterior(monkeypatch):
    """VoltMagpie(vol_solver="linear", vol_posterior="sweep"): with the same seed MeanPrediction agrees with the dense model's
    to the dense tolerance (2e-3 on log-prices, tests/test_gpu_api.py), as the "solve" route is held to in
    tests/test_gpu_bm_linear.py.  Volt keeps the posterior through Train's refit; its Forecast at H = 6 takes the sweep (one
    launch, counted); and two further Volts, one with vol_posterior="sweep" and one with "solve", built, trained and forecast
    under the same seeds agree within the same 2e-3 at H = 6 (Rollouts repeats the model's state, so a model forecasts once)."""
    from volt_amd.gp import GaussianLikelihood
    from volt_amd.models import VoltMagpie
    from volt_amd.models.Volt import Volt
    from volt_amd.synthetic import sde_series
    n, H = 90, 1
    F, vol = sde_series(n, 31)
    tx = torch.arange(n, device="cuda") / 252.
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    ty, vp = dev(F)[1:].log(), dev(vol)
    sweep = VoltMagpie(tx, ty, GaussianLikelihood().cuda(), vp, k=20, vol_solver="linear", vol_posterior="sweep")
    dense = VoltMagpie(tx, ty, GaussianLikelihood().cuda(), vp, k=20)
    assert sweep.vol_model.posterior == "sweep" and sweep.vol_posterior == "sweep" and dense.vol_model.posterior == "solve"
    torch.manual_seed(2)
    s, pv = sweep.SamplePrediction(test_x, return_vol=True)
    assert torch.isfinite(s).all() and torch.isfinite(pv).all() and tuple(pv.shape) == (H,)
    torch.manual_seed(7)
    a = sweep.MeanPrediction(test_x, n_sample=3)
    torch.manual_seed(7)
    b = dense.MeanPrediction(test_x, n_sample=3)
    print(f"VoltMagpie MeanPrediction |sweep - dense| = {float((a - b).abs().max()):.3e} (bound 2e-3)")
    assert a.shape == b.shape and float((a - b).abs().max()) < 2e-3
    with pytest.raises(ValueError, match="vol_posterior"):
        VoltMagpie(tx, ty, GaussianLikelihood().cuda(), vp, k=20, vol_posterior="sweep")

    n, H, S = 130, 6, 8
    F, vol = sde_series(n, 5)
    tx = torch.arange(n + 1, device="cuda") / 252.
    m = Volt(tx, dev(F).log(), mean="ewma", vol_path=dev(vol), k=10, vol_solver="linear", vol_posterior="sweep")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.Train(gpcv_iters=5, vol_mod_iters=5, data_mod_iters=4)
    assert m.vol_model.solver == "linear" and m.vol_model.posterior == "sweep"
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    calls = _count_bm_post(monkeypatch)
    torch.manual_seed(11)
    out = m.Forecast(test_x, nsample=S)
    assert tuple(out.shape) == (S, H) and torch.isfinite(out).all()
    assert len(calls) == 1                                                       # the vol forecast came from ONE sweep
    torch.manual_seed(3)
    m2 = Volt(tx, dev(F).log(), mean="ewma", vol_path=dev(vol), k=10, vol_solver="linear", vol_posterior="solve")
    torch.manual_seed(3)
    m1 = Volt(tx, dev(F).log(), mean="ewma", vol_path=dev(vol), k=10, vol_solver="linear", vol_posterior="sweep")
    outs = []
    for mm in (m1, m2):
        torch.manual_seed(5)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mm.Train(gpcv_iters=5, vol_mod_iters=5, data_mod_iters=4)
        torch.manual_seed(11)
        outs.append(mm.Forecast(test_x, nsample=S))
    assert m1.vol_model.posterior == "sweep" and m2.vol_model.posterior == "solve" and len(calls) == 2
    d2 = float((outs[0] - outs[1]).abs().max())
    print(f"Volt built, trained and forecast twice under the same seeds: max |sweep - solve| = {d2:.3e} (bound 2e-3)")
    assert d2 < 2e-3


@pytest.mark.parametrize("multitask", [False, True], ids=["batched", "multitask"])
def test_stocks_driver_with_the_sweep_posterior(multitask, monkeypatch):
    """The same window, seeds and draws through vol_posterior="solve" and "sweep": the samples (log-price paths) agree within
    the dense route's 2e-3, and the driver's window took the sweep: ONE ops.bm_post launch with "sweep", none with "solve"."""
    from volt_amd import train_utils
    from volt_amd.forecast import GenerateStockPredictionsBatch
    from volt_amd.synthetic import sde_batch
    B, ntrain, H, S = 3, 130, 4, 5
    fit = train_utils.TrainVolModelMultitask if multitask else train_utils.TrainVolModelBatch
    vm, _ = fit(torch.arange(1, 33, device="cuda") / 252., torch.full((2, 32), 0.2, device="cuda"), train_iters=0,
                solver="linear", vol_posterior="sweep")
    assert vm.posterior == "sweep" and vm.solver == "linear"                     # what the driver's window builds
    _, F, _ = sde_batch(B, ntrain + 5, seed=77)
    closes = torch.as_tensor(np.asarray(F)).cuda()
    outs, vols = {}, {}
    calls = _count_bm_post(monkeypatch)
    for posterior in ("solve", "sweep"):
        g = torch.Generator(device="cuda").manual_seed(1)
        torch.manual_seed(1)
        dbg = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            outs[posterior] = GenerateStockPredictionsBatch(["AAA", "BBB", "CCC"], closes, forecast_horizon=H, train_iters=3,
                                                            nsample=S, ntrain=ntrain, mean="ewma", k=10, ntimes=1, vol_iters=4,
                                                            generator=g, debug=dbg, vol_solver="linear",
                                                            multitask_vol=multitask, vol_posterior=posterior)
        vols[posterior] = dbg["pred_vol"]
        assert len(calls) == (1 if posterior == "sweep" else 0), (posterior, len(calls))
    out = outs["sweep"]
    assert tuple(out.shape) == (B, S, H) and torch.isfinite(out).all() and bool((vols["sweep"] > 0).all())
    diff = float((out - outs["solve"]).abs().max())
    print(f"stocks driver ({'multitask' if multitask else 'batched'}): max |sweep - solve| = {diff:.3e} on the samples, "
          f"{float((vols['sweep'] / vols['solve'] - 1).abs().max()):.3e} relative on pred_vol (bound 2e-3)")
    assert diff < 2e-3


# ------------------------------------------------------------------------------------------------ 7: long series
def _peak_growth(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = fn()
    torch.cuda.synchronize()
    return res, torch.cuda.max_memory_allocated() - base


def test_bmgp_sweep_at_2_x_65536_allocates_no_n_by_h_array():
    """2 x 65536 at H = 20: the posterior matches the restatement to the bounds of
    tests/test_gpu_bm_linear.py::test_no_quadratic_memory_at_n_65536, and its peak allocation above the inputs is <= 8 MB
    (the solve route's workspace alone is (1 + H) T N doubles = 22 MB)."""
    n, B, H = 65536, 2, 20
    rng = np.random.default_rng(9)
    x = f32(chain.grids(n, rng)["uniform_dt"])
    r = f32(np.cumsum(rng.standard_normal((B, n)) * 0.05, axis=1) - 2.0)
    m, lh = _bmgp(x, r, torch.float32, "sweep")
    xs = f32(x[-1] + (1 + np.arange(H)) / 252.0)
    xs[:2] = f32([0.5 * (x[1000] + x[1001]), x[40000]])
    xsd = dev(xs)
    post, grown = _peak_growth(lambda: m(xsd))
    print(f"BMGP sweep 2 x {n} H = {H}: peak allocation above the inputs {grown / 2 ** 20:.2f} MB (bound 8 MB)")
    assert grown <= 8 * 2 ** 20, grown
    vol64 = m.covar_module.vol.detach().double().cpu().numpy().reshape(-1)
    noise64 = lh.noise.detach().double().cpu().numpy().reshape(-1)
    resid = f32((dev(r) - m.mean_module(dev(x))).detach().cpu().numpy())              # what the model hands the sweep
    order = np.argsort(xs, kind="stable")
    out, info = ref.post_forms_ref(x, vol64, noise64, resid, xs[order])
    assert not info.any()
    got_m, got_c = post.mean.double().cpu().numpy(), post.covariance_matrix.double().cpu().numpy()
    for t in range(B):
        wm, wc = np.empty(H), np.empty((H, H))
        wm[order] = -0.5 * vol64[t] ** 2 * xs[order] + out[t, 0]
        wc[np.ix_(order, order)] = ref.markov_cov_ref(vol64[t] * xs[order] - out[t, 1], vol64[t] * xs[order] - out[t, 2])
        em = np.abs(got_m[t] - wm).max() / (8 * 2.0 ** -24 * np.abs(r).max())
        ec = np.abs(got_c[t] - wc).max() / (8 * 2.0 ** -24 * vol64.max() * xs.max())
        print(f"  series {t}: error / bound  mean {em:.3f}  cov {ec:.3f}")
        assert em <= 1 and ec <= 1


def test_multitask_sweep_at_65536_x_8_allocates_no_n_by_h_array():
    """65536 x 8 at H = 20: after a first call has built the model's Kronecker workspace, a posterior's peak allocation above
    the inputs and that workspace is <= 8 MB; mean and covariance agree with posterior="solve" within 2 x 2e-4."""
    from test_gpu_multitask import make_case, model_params
    from volt_amd.gp import MultitaskGaussianLikelihood
    from volt_amd.models import MultitaskBMGP
    N, T, H = 65536, 8, 20
    p, x, Y = make_case(N, T, 1, seed=9)
    xc, Yc = x.cuda(), Y.cuda()
    xs = xc[-1] + (torch.arange(H, device="cuda") + 1) / 252.
    posts = {}
    for posterior in ("sweep", "solve"):
        lh = MultitaskGaussianLikelihood(num_tasks=T).cuda()
        m = MultitaskBMGP(xc, Yc, lh, solver="linear", posterior=posterior).cuda().eval()
        with torch.no_grad():
            for k, prm in model_params(m, lh).items():
                prm.copy_(p[k])
        m(xs)                                                                    # builds the workspace
        posts[posterior], grown = _peak_growth(lambda: m(xs))
        print(f"MultitaskBMGP {posterior} {N} x {T} H = {H}: peak allocation above inputs and workspace {grown / 2 ** 20:.2f} MB")
        if posterior == "sweep":
            assert grown <= 8 * 2 ** 20, grown
    a, b = posts["sweep"], posts["solve"]
    assert tuple(a.mean.shape) == (H, T) and torch.isfinite(a.mean).all()
    cs, cb = a.covariance_matrix.double(), b.covariance_matrix.double()
    em = float((a.mean.double() - b.mean.double()).abs().max()) / max(1.0, float(b.mean.abs().max()))
    ec = float((cs - cb).abs().max()) / float(cb.abs().max())
    print(f"  |sweep - solve| / scale  mean {em:.2e}  cov {ec:.2e} (bound 4e-4)")
    assert em <= 4e-4 and ec <= 4e-4
