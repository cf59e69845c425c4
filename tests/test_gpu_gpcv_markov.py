"""The O(N) GPCV step for the Markov variational family on the GPU (csrc/gpcv_markov.hip) against the fp64 loop
restatement tests/gpcv_markov_ref.py, from the kernels up to FitGPCV / LearnGPCV / the stocks driver.

Bounds (the project's GPCV bounds): scalars and F 5e-5 max(1, |ref|); gradients 2e-3 of the gradient's max per series;
dF/dvol 2e-3 |ref| (exactly 0 at N = 1, x_0 = 0, where q_0 = j does not depend on vol).  The scan's boundaries: a thread's run is
4 points, a wave's 256, the step's workgroup chunk 2048 (the draw's 1024)."""
import functools
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpcv_markov_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
J = MR.J
SCALAR_TOL, GRAD_TOL, DV_TOL = 5e-5, 2e-3, 2e-3
OUT = dict(ell=0, kl=1, quad=2, logdet_k=3, logdet_s=4, trace=5, dFdv=6, F=9)
WORST = {}


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


case = MR.case            # the cases and their fp64 references: tests/gpcv_markov_ref.py (shared with the host tests)


def run(ps, we, wk, ws=None, nan_gamma=True):
    from volt_amd import ops
    ghx, ghw = MR.gauss_hermite(75)
    st = lambda k: dev(np.stack([p[k] for p in ps]))
    gam = st("gam")
    if nan_gamma:
        gam[:, -1] = float("nan")                                   # the unused last coupling
    m = st("m")
    mu = dev(np.stack([np.broadcast_to(p["mu"], m.shape[1:]) for p in ps]))      # (a number per series, or [N])
    abc = dev(np.stack([np.stack(p["abc"]) for p in ps])) if ps[0]["abc"] is not None else None
    ws = ops.gpcv_markov_step(dev(ps[0]["x"]), dev([p["v"] for p in ps]), m - mu, m, st("rho"), gam, st("y"), dev(ghx), dev(ghw),
                              ws, abc=abc, jitter=J, w_ell=we, w_kl=wk)
    torch.cuda.synchronize()
    return ws


def ratios(ws, refs, n):
    """error / bound per quantity, the worst series."""
    out = ws.out.cpu().double().numpy()
    r = {}
    for b, ref in enumerate(refs):
        for k, col in OUT.items():
            if k == "dFdv":
                if ref[k] == 0.0:
                    e = 0.0 if out[b, col] == 0.0 else float("inf")
                else:
                    e = abs(out[b, col] - ref[k]) / (DV_TOL * abs(ref[k]))
            else:
                e = abs(out[b, col] - ref[k]) / (SCALAR_TOL * max(1.0, abs(ref[k])))
            r[k] = max(r.get(k, 0.0), e)
        for k in MR.GRADS:
            got = getattr(ws, k)[b].cpu().double().numpy()
            if k == "grad_gamma":
                assert got[-1] == 0.0
                if n == 1:
                    continue
            r[k] = max(r.get(k, 0.0), np.abs(got - ref[k]).max() / (GRAD_TOL * np.abs(ref[k]).max()))
        if ref["grad_abc"] is not None:
            got = ws.grad_abc[b].cpu().double().numpy()
            r["grad_abc"] = max(r.get("grad_abc", 0.0), np.abs(got - ref["grad_abc"]).max() / (GRAD_TOL * np.abs(ref["grad_abc"]).max()))
        s = ws.s[b].cpu().numpy()
        r["s"] = max(r.get("s", 0.0), np.abs(s - ref["s"]).max() / (1e-12 * np.abs(ref["s"]).max()))   # fp64 on both sides
    return r


def check(ws, refs, n, label):
    assert not ws.info.any(), ws.info.tolist()
    r = ratios(ws, refs, n)
    for k, e in r.items():
        WORST[k] = max(WORST.get(k, 0.0), e)
    print(f"{label}: error / bound " + " ".join(f"{k} {e:.3f}" for k, e in r.items()))
    assert all(e <= 1.0 for e in r.values()), r


@pytest.mark.parametrize("n,B", [c[:2] for c in MR.EXP_CASES])
def test_exp_step_matches_the_restatement(n, B):
    ps, refs, we, wk = case(n, B)
    check(run(ps, we, wk), refs, n, f"exp {B} x {n}")


@pytest.mark.parametrize("n,B,Kc", [c[:3] for c in MR.CV_CASES])
def test_cv_step_matches_the_restatement(n, B, Kc):
    ps, refs, we, wk = case(n, B, Kc)
    check(run(ps, we, wk), refs, n, f"cv K={Kc} {B} x {n}")


@pytest.mark.parametrize("kind,Kc", [(c[3], c[2]) for c in MR.KIND_CASES])
def test_floored_variances_and_clamped_scales(kind, Kc):
    ps, refs, we, wk = case(130, 3, Kc, kind)
    if kind == "floored":
        assert all((r["s"][::2] < 1e-6).all() for r in refs)
    check(run(ps, we, wk), refs, 130, f"{kind} K={Kc}")


def test_zz_print_the_largest_error_over_bound():
    print("largest error / bound over every case run so far:", {k: f"{e:.3f}" for k, e in WORST.items()})


# ------------------------------------------------------------------------------------------------ buffers, repeatability, graph
@pytest.mark.parametrize("n,B,Kc", [(1, 1, 0), (65, 3, 5), (399, 1, 0), (2049, 2, 0)])
def test_step_writes_nothing_past_its_buffers_and_repeats_bitwise(n, B, Kc):
    """NaN in the unused last coupling; NaN sentinels behind every output; a workspace filled with NaN bit patterns (0xFF
    bytes), guarded on both sides; ten runs agree bit for bit."""
    from volt_amd import ops
    ps, refs, we, wk = case(n, B, Kc)
    ws = ops.GpcvMarkovWorkspace(B, n, DEV, Kc)
    ws.buf.fill_(0xFF)
    guard = 64
    sizes = dict(out=(B, 12), grad_m=(B, n), grad_mu=(B, n), grad_rho=(B, n), grad_gamma=(B, n))
    if Kc:
        sizes["grad_abc"] = (B, 3, Kc)
    bufs = {}
    for k, shape in sizes.items():
        bufs[k] = torch.full((int(np.prod(shape)) + guard,), float("nan"), device=DEV)
        setattr(ws, k, bufs[k][:int(np.prod(shape))].view(shape))
    ibuf = torch.full((B + guard,), -77, dtype=torch.int32, device=DEV)
    ws.info = ibuf[:B]
    got = run(ps, we, wk, ws)
    assert got is ws and ws.out.data_ptr() == bufs["out"].data_ptr()
    check(ws, refs, n, f"sentinels {B} x {n} K={Kc}")
    first = {k: getattr(ws, k).clone() for k in list(sizes) + ["info", "s"]}
    for _ in range(9):
        for k, shape in sizes.items():
            bufs[k][:int(np.prod(shape))].fill_(float("nan"))
        off = ws.ptr - ws.buf.data_ptr()
        ws.buf[off:off + ws.nbytes].fill_(0xFF)
        run(ps, we, wk, ws)
        for k, v in first.items():
            assert torch.equal(getattr(ws, k), v), k
    for k, shape in sizes.items():
        assert torch.isnan(bufs[k][int(np.prod(shape)):]).all(), k
    assert bool((ibuf[B:] == -77).all())
    off = ws.ptr - ws.buf.data_ptr()
    assert bool((ws.buf[off + ws.nbytes:] == 0xFF).all()) and bool((ws.buf[:off] == 0xFF).all())


def test_graph_replay_equals_eager():
    from volt_amd import ops
    n, B, Kc = 399, 3, 5
    ps, refs, we, wk = case(n, B, Kc)
    eager = run(ps, we, wk)
    want = {k: getattr(eager, k).clone() for k in ("out", "grad_m", "grad_mu", "grad_rho", "grad_gamma", "grad_abc", "info")}
    ghx, ghw = MR.gauss_hermite(75)
    st = lambda k: dev(np.stack([p[k] for p in ps]))
    m, mu = st("m"), dev([p["mu"] for p in ps]).reshape(-1, 1)
    args = (dev(ps[0]["x"]), dev([p["v"] for p in ps]), m - mu, m, st("rho"), st("gam"), st("y"), dev(ghx), dev(ghw))
    abc = dev(np.stack([np.stack(p["abc"]) for p in ps]))
    ws = ops.GpcvMarkovWorkspace(B, n, DEV, Kc)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gpcv_markov_step(*args, ws, abc=abc, jitter=J, w_ell=we, w_kl=wk)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.gpcv_markov_step(*args, ws, abc=abc, jitter=J, w_ell=we, w_kl=wk)
    for k in want:
        getattr(ws, k).fill_(-1 if k == "info" else float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for k, v in want.items():
        assert torch.equal(getattr(ws, k), v), k


# ------------------------------------------------------------------------------------------------ side by side with gpcv_bm_step
@pytest.mark.parametrize("B,n", [(1, 399), (8, 399), (2, 1024)])
def test_prior_independent_outputs_are_as_accurate_as_the_quadratic_step(B, n):
    """ops.gpcv_bm_step on the dense Lq = chol(P^-1) against ops.gpcv_markov_step on (rho, gamma): ell, logdet S and the rows'
    part of grad_m do not depend on the prior.  Both steps run with resid = m - mu = 0, so that grad_m IS the rows' part
    w_ell dE/dm (with a residual, each step's fp32 grad_m carries the rounding of its own, much larger, prior term).  The Markov
    step's error against fp64 is at most the larger of the quadratic step's own and one output rounding, 2^-23 |ref|."""
    from volt_amd import ops
    ps, _, we, wk = case(n, B)
    ghx, ghw = MR.gauss_hermite(75)
    ps = [dict(p, mu=p["m"]) for p in ps]
    refs = [MR.step(p["x"], p["v"], J, p["mu"], p["m"], p["rho"], p["gam"], p["y"], ghx, ghw, we, wk) for p in ps]
    wm = run(ps, we, wk)
    Lq = []
    for p in ps:
        Lp = MR.dense_root(p["rho"], p["gam"])
        S = np.linalg.inv(Lp @ Lp.T)
        Lq.append(np.linalg.cholesky(0.5 * (S + S.T)))
    st = lambda k: dev(np.stack([p[k] for p in ps]))
    m, mu = st("m"), st("m")
    x = ps[0]["x"] if ps[0]["x"][0] > 0 else ps[0]["x"] + 1.0 / 252        # (the quadratic step's prior: any valid grid will do)
    wb = ops.gpcv_bm_step(dev(x), dev([p["v"] for p in ps]), m - mu, m, dev(np.stack(Lq)), st("y"), dev(ghx), dev(ghw),
                          jitter=J, w_ell=we, w_kl=wk)
    torch.cuda.synchronize()
    assert not wb.info.any() and not wm.info.any()
    bad = []
    for b, ref in enumerate(refs):
        rows_ref = ref["grad_m"]
        assert not ref["grad_mu"].any()
        for name, em, eb, scale in (
                ("ell", abs(float(wm.out[b, 0]) - ref["ell"]), abs(float(wb.out[b, 0]) - ref["ell"]), abs(ref["ell"])),
                ("logdet_s", abs(float(wm.out[b, 4]) - ref["logdet_s"]), abs(float(wb.out[b, 4]) - ref["logdet_s"]), abs(ref["logdet_s"])),
                ("rows grad_m", np.abs(wm.grad_m[b].cpu().double().numpy() - rows_ref).max(),
                 np.abs(wb.grad_m[b].cpu().double().numpy() - rows_ref).max(), np.abs(rows_ref).max())):
            ok = em <= max(eb, 2.0 ** -23 * scale)
            print(f"{B} x {n} series {b} {name:12s}: markov {em:.3e}  quadratic {eb:.3e}  (|ref| {scale:.3e}){'' if ok else '  <-- worse'}")
            if not ok:
                bad.append((b, name))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the draw and the variance
@pytest.mark.parametrize("S", [1, 10, 65])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 129, 399, 1023, 1024, 1025, 2049])
def test_draw_matches_the_restatement(n, S):
    from volt_amd import ops
    B = 2
    ps = [MR.make_inputs(n, 500 + n + b) for b in range(B)]
    eps = np.asarray(np.random.default_rng(n + S).standard_normal((B, S, n)), dtype=np.float32)
    st = lambda k: dev(np.stack([p[k] for p in ps]))
    gam = st("gam")
    gam[:, -1] = float("nan")
    got = ops.markov_root_draw(st("m"), st("rho"), gam, dev(eps)).cpu().double().numpy()
    for b, p in enumerate(ps):
        want = MR.draw(p["m"], p["rho"], p["gam"], eps[b].astype(np.float64))
        assert (np.abs(got[b] - want) <= 2.0 ** -23 * np.abs(want) + 1e-10 * np.abs(want).max()).all(), (n, S, b)


def test_latent_variance_equals_the_steps_s_and_samples_have_it():
    n, B = 399, 3
    ps, refs, we, wk = case(n, B)
    ws = run(ps, we, wk, nan_gamma=False)
    model, lh = _model(dev(ps[0]["x"]), batch=B)
    d = model.variational_strategy._variational_distribution
    with torch.no_grad():
        d.log_diag_precision_root.copy_(dev(np.stack([p["rho"] for p in ps])))
        d.coupling.copy_(dev(np.stack([p["gam"] for p in ps])))
        d.variational_mean.copy_(dev(np.stack([p["m"] for p in ps])))
    lat = model(dev(ps[0]["x"]))
    assert torch.equal(lat.variance, ws.s.to(torch.float32).clamp_min(1e-6))
    f = lat.rsample(torch.Size([4000]))
    assert tuple(f.shape) == (4000, B, n)
    sv = f.double().var(0).cpu().numpy()
    want = np.stack([r["s"] for r in refs])
    assert np.abs(sv / want - 1).max() < 6 * math.sqrt(2.0 / 4000)                  # a sample variance: sd sqrt(2 / S) relative
    S = lat._covar[0].double().cpu().numpy()                                        # dense only on request
    assert np.abs(np.diag(S) - want[0]).max() <= 1e-5 * want[0].max()


# ------------------------------------------------------------------------------------------------ model level
def _model(x, param="exp", K=1, batch=None, seed=5):
    from volt_amd import gp
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import SingleTaskVariationalGP
    kw = {"batch_shape": torch.Size([batch])} if batch else {}
    torch.manual_seed(seed)
    lh = VolatilityGaussianLikelihood(param="exp") if param == "exp" else VolatilityGaussianLikelihood(K=K, param=param, **kw).to(DEV)
    model = SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=lh, use_piv_chol_init=False,
                                    mean_module=gp.ConstantMean(**kw), covar_module=BMKernel(**kw),
                                    learn_inducing_locations=False, use_whitened_var_strat=False, prior_solver="markov").to(DEV)
    n = x.shape[0]
    shape = (batch,) if batch else ()
    d = model.variational_strategy._variational_distribution
    with torch.no_grad():
        ps = [MR.make_inputs(n, 900 + b) for b in range(batch or 1)]
        for t, k in ((d.variational_mean, "m"), (d.log_diag_precision_root, "rho"), (d.coupling, "gam")):
            t.data = dev(np.stack([p[k] for p in ps])).reshape(*shape, n)                # (batched: [T,N])
        model.mean_module.constant.fill_(-0.9)
    assert tuple(d.coupling.shape) == shape + (n,)
    return model, lh


def _elbo_and_grads(model, lh, x, yy):
    from volt_amd.variational import VariationalELBO, num_gauss_hermite_locs
    elbo = VariationalELBO(lh, model, yy.shape[-1])
    ps = list(model.parameters())
    ps += [q for q in lh.parameters() if all(q is not p for p in ps)]
    for p in ps:
        p.requires_grad_(True)
        p.grad = None
    with num_gauss_hermite_locs(75):
        val = elbo(model(x), yy)
    (val.sum() if val.ndim else val).backward()
    return val.detach(), {id(p): p.grad.clone() for p in ps if p.grad is not None}, ps


@pytest.mark.parametrize("param,K", [("exp", 1), ("cv", 5)])
def test_elbo_backward_reaches_every_parameter(param, K):
    """VariationalELBO's value and the gradient of EVERY parameter -- raw_vol and the "cv" raws through their constraints --
    against the restatement."""
    n = 130
    x = (torch.arange(1, n + 1, dtype=torch.float32) / 252).to(DEV)
    yy = dev(np.random.default_rng(4).standard_normal(n) * 0.2)
    model, lh = _model(x, param, K)
    val, grads, ps = _elbo_and_grads(model, lh, x, yy)
    names = dict((id(p), k) for k, p in list(model.named_parameters()) + [("likelihood." + k, p) for k, p in lh.named_parameters()])
    assert all(id(p) in grads for p in ps), [names[id(p)] for p in ps if id(p) not in grads]
    d = model.variational_strategy._variational_distribution
    f64 = lambda t: t.detach().cpu().double().numpy().reshape(-1)
    raw_vol = float(model.covar_module.raw_vol.detach())
    v = 1.0 / (1.0 + math.exp(-raw_vol))
    v32 = float(torch.sigmoid(model.covar_module.raw_vol.detach()).float())
    abc = None
    if param == "cv":
        abc = tuple(f64(t) for t in (lh.trans_a, lh.trans_b, lh.trans_c))
    ghx, ghw = MR.gauss_hermite(75)
    ref = MR.step(f64(x), v32, J, -0.9, f64(d.variational_mean), f64(d.log_diag_precision_root), f64(d.coupling), f64(yy), ghx, ghw,
                  1.0 / n, 1.0 / n, abc=abc)
    assert abs(float(val) - ref["F"]) <= SCALAR_TOL * max(1.0, abs(ref["F"]))
    want = {"variational_strategy._variational_distribution.variational_mean": ref["grad_m"],
            "variational_strategy._variational_distribution.log_diag_precision_root": ref["grad_rho"],
            "variational_strategy._variational_distribution.coupling": ref["grad_gamma"],
            "mean_module.constant": np.array([ref["grad_mu"].sum()]),
            "covar_module.raw_vol": np.array([ref["dFdv"] * v * (1 - v)])}
    if param == "cv":
        sig = lambda t: 1.0 / (1.0 + np.exp(-f64(t)))
        sb, sc = sig(lh.raw_b), sig(lh.raw_c)
        want.update({"likelihood.raw_a": ref["grad_abc"][0] * sig(lh.raw_a), "likelihood.raw_b": ref["grad_abc"][1] * 3 * sb * (1 - sb),
                     "likelihood.raw_c": ref["grad_abc"][2] * 6 * sc * (1 - sc)})
    seen = set()
    for p in ps:
        k = names[id(p)]
        err = np.abs(f64(grads[id(p)]) - want[k]).max() / np.abs(want[k]).max()
        print(f"  grad {k}: {err:.2e}")
        assert err < GRAD_TOL, (k, err)
        seen.add(k)
    assert seen == set(want)


def test_elbo_batched_equals_per_series():
    """A batched model's ELBO [T] equals the T separate models': value bitwise, gradients 1e-6 (of their max)."""
    n, T = 130, 3
    x = (torch.arange(n, dtype=torch.float32) / 252).to(DEV)
    yy = dev(np.random.default_rng(4).standard_normal((T, n)) * 0.2)
    mb, lb = _model(x, batch=T)
    with torch.no_grad():
        mb.covar_module.raw_vol.copy_(torch.logit(torch.tensor([[0.2], [0.5], [0.1]])))
    vb, gb, pb = _elbo_and_grads(mb, lb, x, yy)
    for i in range(T):
        mi, li = _model(x)
        with torch.no_grad():
            for (_, p), (_, q) in zip(mi.named_parameters(), mb.named_parameters()):
                p.copy_(q[i].reshape(p.shape))
        vi, gi, pi = _elbo_and_grads(mi, li, x, yy[i])
        assert torch.equal(vi, vb[i])
        for p, q in zip(pi, pb):
            a, b = gi[id(p)], gb[id(q)][i].reshape(p.shape)
            assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), float((a - b).abs().max() / b.abs().max())


# ------------------------------------------------------------------------------------------------ trainer and drivers
def _prices(n, seed):
    from volt_amd.synthetic import sde_series
    return torch.tensor(sde_series(n, seed)[0])


@functools.lru_cache(maxsize=None)
def _fit_reference(n, T, iters=40):
    """The start-up values FitGPCV(solver="markov") makes, and fp64 Adam on the restatement from them, per series."""
    from volt_amd.train_utils import FitGPCV
    F = torch.stack([_prices(n, 2021 + i) for i in range(T)])                      # [T, n + 1] prices
    x = torch.arange(n, dtype=torch.float32) / 252                                  # (x_0 = 0: valid under the level's jitter)
    out = []
    f64 = lambda t: t.detach().cpu().double().numpy().reshape(-1)
    for i in range(T):
        m0, _, _ = FitGPCV(x.to(DEV), F[i].to(DEV), train_iters=0, solver="markov")
        d0 = m0.variational_strategy._variational_distribution
        yy = f64((F[i][1:] - F[i][:-1]) / F[i][:-1] / (x[1] - x[0]) ** 0.5)         # the scaled returns, in fp32 as FitGPCV forms them
        start = (f64(d0.variational_mean), f64(d0.log_diag_precision_root), f64(d0.coupling), f64(m0.mean_module.constant))
        out.append(MR.learn(f64(x), yy, start, iters))
    return x, F, out


def _fit_errors(model, T, i, ps):
    """|parameter - fp64 Adam's| for series i: variational mean, log_diag_precision_root, coupling, raw_vol, constant."""
    d = model.variational_strategy._variational_distribution
    f64 = lambda t: t.detach().cpu().double().reshape(T, -1)[i].numpy()
    return dict(mean=np.abs(f64(d.variational_mean) - ps[0]).max(), rho=np.abs(f64(d.log_diag_precision_root) - ps[1]).max(),
                gamma=np.abs(f64(d.coupling) - ps[2]).max(), raw_vol=abs(f64(model.covar_module.raw_vol)[0] - ps[4][0]),
                const=abs(f64(model.mean_module.constant)[0] - ps[3][0]))


@pytest.mark.parametrize("n,T", [(399, 1), (130, 3)])
def test_fit_gpcv_markov_tracks_fp64_adam_and_captured_equals_eager(n, T, monkeypatch):
    """FitGPCV(solver="markov") for 40 Adam iterations against fp64 Adam on the restatement from the same start, with the
    trainer bounds of the "linear" row -- losses 5e-4 (of max(1, |loss|)), every parameter 5e-3: the variational mean,
    log_diag_precision_root, coupling, raw_vol and the constant -- for the eager loop (torch.optim.Adam, every loss) AND for the
    captured loop as LearnGPCV runs it (optim.FusedAdam; it returns its last loss).  Then: the captured loop equals an eager
    one bit for bit when both run the same optimiser arithmetic (FusedAdam also runs eagerly; torch.optim.Adam rounds
    differently whatever the step)."""
    from volt_amd import train_utils
    from volt_amd.train_utils import FitGPCV
    iters = 40
    x, F, want = _fit_reference(n, T)
    prices = F[0] if T == 1 else F

    def fit(graph):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return FitGPCV(x.to(DEV), prices.to(DEV), train_iters=iters, solver="markov", graph=graph)

    model, lh, losses = fit(False)
    assert model.prior_solver == "markov"
    got = torch.stack(losses).cpu().double().reshape(len(losses), -1)
    for i in range(T):
        rec, ps = want[i]
        w = torch.tensor(rec, dtype=torch.float64)
        err = float(((got[:, i] - w).abs() / w.abs().clamp_min(1.0)).max())
        errs = _fit_errors(model, T, i, ps)
        print(f"fit eager {T} x {n} series {i}: loss {err:.2e} " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        assert err < 5e-4 and max(errs.values()) < 5e-3, (err, errs)
    captured, _, lc = fit(True)                                  # the default optimiser of a captured loop: FusedAdam
    last = sum(want[i][0][-1] for i in range(T))
    lerr = abs(float(lc[-1].sum()) - last) / max(1.0, abs(last))
    assert len(lc) == 1 and lerr < 5e-4, lerr
    for i in range(T):
        errs = _fit_errors(captured, T, i, want[i][1])
        print(f"fit captured {T} x {n} series {i}: last loss {lerr:.2e} " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        assert max(errs.values()) < 5e-3, errs
    adam = train_utils._adam
    monkeypatch.setattr(train_utils, "_adam", lambda params, lr, graph: adam(params, lr, True))
    eager, _, le = fit(False)                                    # eager, with the captured loop's optimiser
    assert torch.equal(le[-1].sum(), lc[-1].sum())
    for a, b in zip(eager.parameters(), captured.parameters()):
        assert torch.equal(a, b)


def test_learn_gpcv_markov_returns_a_positive_scale():
    from volt_amd.train_utils import LearnGPCV
    n = 200
    x = (torch.arange(n, dtype=torch.float32) / 252).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vol = LearnGPCV(x, _prices(n, 2019).to(DEV), train_iters=15, solver="markov")
        volb = LearnGPCV(x, torch.stack([_prices(n, 2019), _prices(n, 2020)]).to(DEV), train_iters=15, solver="markov",
                         param="cv", K=1)
    assert tuple(vol.shape) == (n,) and torch.isfinite(vol).all() and bool((vol > 0).all())
    assert tuple(volb.shape) == (2, n) and torch.isfinite(volb).all() and bool((volb > 0).all())


def test_stocks_driver_with_the_markov_gpcv_solver(tmp_path):
    from volt_amd.forecast import GenerateStockPredictionsBatch
    from volt_amd.synthetic import sde_batch
    B, T, ntrain, H, S = 3, 70, 64, 4, 5
    _, F, _ = sde_batch(B, T - 1, seed=77)
    closes = torch.as_tensor(np.asarray(F)).to(DEV)
    g = torch.Generator(device="cuda").manual_seed(1)
    out = GenerateStockPredictionsBatch(["AAA", "BBB", "CCC"], closes, forecast_horizon=H, train_iters=3, nsample=S,
                                        ntrain=ntrain, mean="ewma", save=True, k=10, ntimes=1, vol_iters=2,
                                        par_dir=str(tmp_path), generator=g, gpcv_solver="markov")
    assert tuple(out.shape) == (B, S, H) and torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------ failures
def test_nan_input_raises_nan_error_and_refusals():
    from volt_amd.forecast import GenerateStockPredictionsBatch
    from volt_amd.safe import NanError
    from volt_amd.train_utils import FitGPCV
    n = 65
    x = (torch.arange(1, n + 1, dtype=torch.float32) / 252).to(DEV)
    yy = dev(np.random.default_rng(4).standard_normal(n) * 0.2)
    model, lh = _model(x)
    with torch.no_grad():
        model.variational_strategy._variational_distribution.variational_mean[7] = float("nan")
    with pytest.raises(NanError):
        _elbo_and_grads(model, lh, x, yy)
    ps, refs, we, wk = case(65, 3)
    bad = [dict(p) for p in ps]
    bad[1]["v"] = float("nan")
    ws = run(bad, we, wk)
    assert ws.info.tolist() == [0, 1, 0] and torch.isfinite(ws.out[[0, 2], :10]).all()
    with pytest.raises(ValueError, match="kernel='bm'"):
        FitGPCV(x, torch.ones(n + 1, device=DEV), kernel="fbm", solver="markov")
    with pytest.raises(ValueError, match='gpcv_solver="markov"'):
        GenerateStockPredictionsBatch(["a", "b"], torch.ones(2, 40, device=DEV), ntrain=30, multitask_gpcv=True,
                                      gpcv_solver="markov")


# ------------------------------------------------------------------------------------------------ memory
def test_two_series_of_65536_points_stay_within_64_mb():
    """Construction, start-up values, one ELBO step and its backward at 2 x 65536: the peak allocation above the inputs is at
    most 64 MB, the project's cap for its linear routes (a dense Lq alone would be 2 x 17 GB)."""
    from volt_amd import gp
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import SingleTaskVariationalGP
    from volt_amd.variational import VariationalELBO, num_gauss_hermite_locs
    n, T = 65536, 2
    x = (torch.arange(1, n + 1, dtype=torch.float32) / 252).to(DEV)
    yy = dev(np.random.default_rng(1).standard_normal((T, n)) * 0.2)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    kw = {"batch_shape": torch.Size([T])}
    lh = VolatilityGaussianLikelihood(param="exp")
    model = SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=lh, use_piv_chol_init=False,
                                    mean_module=gp.ConstantMean(**kw), covar_module=BMKernel(**kw),
                                    learn_inducing_locations=False, use_whitened_var_strat=False, prior_solver="markov").to(DEV)
    model.initialize_variational_parameters(lh, x, y=yy)
    elbo = VariationalELBO(lh, model, n)
    with num_gauss_hermite_locs(75):
        val = elbo(model(x), yy)
    val.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"2 x {n}: peak allocation above the inputs {peak / 2 ** 20:.1f} MB; ELBO {val.tolist()}")
    assert torch.isfinite(val).all() and all(torch.isfinite(p.grad).all() for p in model.parameters())
    assert peak <= 64 * 2 ** 20
