"""The multi-task GPCV step for the Markov variational family on the GPU (csrc/gpcv_mt_markov.hip) against the
fp64 loop restatement tests/mt_gpcv_markov_ref.py, from the kernels up to FitGPCVMultitask / LearnGPCVMultitask / the stocks
driver.

Bounds (the project's GPCV bounds): scalars and F 5e-5 max(1, |ref|); gradients 2e-3 of the gradient's largest reference
entry; dF/dvol 2e-3 |ref| (exactly 0 at N = 1, x_0 = 0, where q_0 = j does not depend on vol); grad_abc 2e-3; .s 1e-12 (fp64
on both sides).
Tiles (csrc/gpcv_mt_markov.hip): the scans compose 4 points a thread, 256 a wave, 2048 a chunk; the quadrature pass takes
16 rows a workgroup (MM_ROWS); the partial sums of G, G2 take 128 rows a workgroup (MM_GCH), staged 32 at a time (MM_GST);
grad_M takes 32 rows a workgroup (MM_MROWS); the "cv" parameter partials (one per quadrature workgroup) are added by 256
threads, so N = 4097 makes 257 of them.  mt_gpcv_markov_ref.BOUNDARIES has both sides of each."""
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
import mt_gpcv_markov_ref as MM  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
J = MM.J
OUT = {k: i for i, k in enumerate(MM.SCALARS)}              # out[0..10]
FIELDS = dict(grad_M="grad_M", grad_c="grad_c", grad_rho="grad_rho", grad_gamma="grad_gamma", grad_Lt="grad_Lt",
              grad_f="grad_covar_factor", grad_raw_var="grad_raw_var")
WORST = {}


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


case = MM.case            # the cases and their fp64 references: tests/mt_gpcv_markov_ref.py (shared with the host tests)


def step_args(p, nan_gamma=True):
    ghx, ghw = MR.gauss_hermite(75)
    gam = dev(p["gam"])
    if nan_gamma:
        gam[-1] = float("nan")                                          # the unused last coupling
    abc = dev(np.stack(p["abc"], 1)) if p["abc"] is not None else None    # [T,3,Kc]
    return (dev(p["x"]), dev([p["v"]]), dev(p["M"]), dev(p["c"]), dev(p["rho"]), gam, dev(p["Lt"]), dev(p["f"]), dev(p["raw_var"]),
            dev(p["y"]), dev(ghx), dev(ghw)), abc


def run(p, we, wk, ws=None, nan_gamma=True):
    from volt_amd import ops
    args, abc = step_args(p, nan_gamma)
    ws = ops.gpcv_mt_markov_step(*args, ws, abc=abc, jitter=J, w_ell=we, w_kl=wk)
    torch.cuda.synchronize()
    return ws


def outputs(ws):
    out = ws.out.cpu().double().numpy()
    o = {k: out[i] for k, i in OUT.items()}
    o.update({k: getattr(ws, f).cpu().double().numpy() for k, f in FIELDS.items()})
    if ws.grad_abc is not None:
        o["grad_abc"] = ws.grad_abc.cpu().double().numpy()
    return o


def check(ws, ref, n, label):
    assert not ws.info.any(), ws.info.tolist()
    o = outputs(ws)
    assert o["grad_gamma"][-1] == 0.0
    assert not np.triu(o["grad_Lt"], 1).any()
    r = MM.bound_excess(o, ref, n)
    s = ws.s.cpu().numpy()
    r["s"] = float(np.abs(s - ref["s"]).max() / (1e-12 * np.abs(ref["s"]).max()))   # fp64 on both sides
    for k, e in r.items():
        WORST[k] = max(WORST.get(k, 0.0), e)
    print(f"{label}: error / bound " + " ".join(f"{k} {e:.3f}" for k, e in r.items()))
    assert all(e <= 1.0 for e in r.values()), r


@pytest.mark.parametrize("n,T", [c[:2] for c in MM.EXP_CASES])
def test_exp_step_matches_the_restatement(n, T):
    p, ref, we, wk = case(n, T)
    check(run(p, we, wk), ref, n, f"exp {n} x {T}")


@pytest.mark.parametrize("n,T,Kc", [c[:3] for c in MM.CV_CASES])
def test_cv_step_matches_the_restatement(n, T, Kc):
    p, ref, we, wk = case(n, T, Kc)
    check(run(p, we, wk), ref, n, f"cv K={Kc} {n} x {T}")


@pytest.mark.parametrize("kind,Kc", [(c[3], c[2]) for c in MM.KIND_CASES])
def test_floored_variances_and_clamped_scales(kind, Kc):
    p, ref, we, wk = case(130, 3, Kc, kind)
    if kind == "floored":
        assert (ref["s"][::2] * (np.tril(p["Lt"]) ** 2).sum(1).max() < 1e-6).all()
    check(run(p, we, wk), ref, 130, f"{kind} K={Kc}")


def test_zz_print_the_largest_error_over_bound():
    print("largest error / bound over every case run so far:", {k: f"{e:.3f}" for k, e in WORST.items()})


# ------------------------------------------------------------------------------------------------ buffers, repeatability, graph
@pytest.mark.parametrize("n,T,Kc", [(1, 1, 0), (65, 3, 5), (399, 64, 0), (2049, 2, 0)])
def test_step_writes_nothing_past_its_buffers_and_repeats_bitwise(n, T, Kc):
    """NaN in the unused last coupling; NaN sentinels behind every output; a workspace filled with NaN bit patterns (0xFF
    bytes), guarded on both sides; ten runs agree bit for bit."""
    from volt_amd import ops
    p, ref, we, wk = case(n, T, Kc)
    ws = ops.GpcvMtMarkovWorkspace(n, T, DEV, Kc)
    ws.buf.fill_(0xFF)
    guard = 64
    sizes = dict(out=(12,), grad_M=(n, T), grad_c=(T,), grad_rho=(n,), grad_gamma=(n,), grad_Lt=(T, T), grad_covar_factor=(T,),
                 grad_raw_var=(T,))
    if Kc:
        sizes["grad_abc"] = (T, 3, Kc)
    bufs = {}
    for k, shape in sizes.items():
        bufs[k] = torch.full((int(np.prod(shape)) + guard,), float("nan"), device=DEV)
        setattr(ws, k, bufs[k][:int(np.prod(shape))].view(shape))
    ibuf = torch.full((2 + guard,), -77, dtype=torch.int32, device=DEV)
    ws.info = ibuf[:2]
    got = run(p, we, wk, ws)
    assert got is ws and ws.out.data_ptr() == bufs["out"].data_ptr()
    check(ws, ref, n, f"sentinels {n} x {T} K={Kc}")
    first = {k: getattr(ws, k).clone() for k in list(sizes) + ["info", "s"]}
    for _ in range(9):
        for k, shape in sizes.items():
            bufs[k][:int(np.prod(shape))].fill_(float("nan"))
        off = ws.ptr - ws.buf.data_ptr()
        ws.buf[off:off + ws.nbytes].fill_(0xFF)
        run(p, we, wk, ws)
        for k, v in first.items():
            assert torch.equal(getattr(ws, k), v), k
    for k, shape in sizes.items():
        assert torch.isnan(bufs[k][int(np.prod(shape)):]).all(), k
    assert bool((ibuf[2:] == -77).all())
    off = ws.ptr - ws.buf.data_ptr()
    assert bool((ws.buf[off + ws.nbytes:] == 0xFF).all()) and bool((ws.buf[:off] == 0xFF).all())


def test_graph_replay_equals_eager():
    from volt_amd import ops
    n, T, Kc = 399, 2, 5
    p, ref, we, wk = case(n, T, Kc)
    eager = run(p, we, wk, nan_gamma=False)
    names = list(FIELDS.values()) + ["out", "grad_abc", "info"]
    want = {k: getattr(eager, k).clone() for k in names}
    args, abc = step_args(p, nan_gamma=False)
    ws = ops.GpcvMtMarkovWorkspace(n, T, DEV, Kc)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gpcv_mt_markov_step(*args, ws, abc=abc, jitter=J, w_ell=we, w_kl=wk)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.gpcv_mt_markov_step(*args, ws, abc=abc, jitter=J, w_ell=we, w_kl=wk)
    for k in want:
        getattr(ws, k).fill_(-1 if k == "info" else float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for k, v in want.items():
        assert torch.equal(getattr(ws, k), v), k


# ------------------------------------------------------------------------------------------------ model level
def _model(p, param="exp", K=1, seed=5):
    """MultitaskVariationalGP(prior_solver="markov") on the device with the parameters of the inputs ``p``."""
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import MultitaskVariationalGP
    n, T = p["M"].shape
    torch.manual_seed(seed)
    lh = VolatilityGaussianLikelihood(param="exp") if param == "exp" else \
        VolatilityGaussianLikelihood(K=K, param=param, batch_shape=torch.Size([T])).to(DEV)
    model = MultitaskVariationalGP(dev(p["x"]), num_tasks=T, covar_module=BMKernel(), prior_solver="markov").to(DEV)
    with torch.no_grad():
        for t, k in ((model.variational_mean, "M"), (model.log_diag_precision_root, "rho"), (model.coupling, "gam"),
                     (model.variational_task_covar_root, "Lt"), (model.index_kernel.raw_var, "raw_var")):
            t.copy_(dev(p[k]))
        model.index_kernel.covar_factor.copy_(dev(p["f"]).reshape(T, 1))
        for t, m in enumerate(model.mean_module.base_means):
            m.constant.fill_(float(p["c"][t]))
        model.data_kernel.vol = float(p["v"])
    return model, lh


def _elbo_and_grads(model, lh, x, yy, num_data):
    from volt_amd.variational import VariationalELBO, num_gauss_hermite_locs
    elbo = VariationalELBO(lh, model, num_data)
    ps = list(model.parameters()) + list(lh.parameters())
    for q in ps:
        q.requires_grad_(True)
        q.grad = None
    with num_gauss_hermite_locs(75):
        val = elbo(model(x), yy)
    val.backward()
    return val.detach(), {id(q): q.grad.clone() for q in ps if q.grad is not None}, ps


@pytest.mark.parametrize("param,K", [("exp", 1), ("cv", 5)])
def test_elbo_backward_reaches_every_parameter(param, K):
    """VariationalELBO's value and the gradient of EVERY parameter -- raw_vol and the "cv" raws through their constraints --
    against the restatement at the model's weights 1/N and 1/(N T)."""
    n, T = 130, 3
    p = MM.make_inputs(n, T, 77, x0_zero=True)
    model, lh = _model(p, param, K)
    x = dev(p["x"])
    val, grads, ps = _elbo_and_grads(model, lh, x, dev(p["y"]), n * T)
    names = dict((id(q), k) for k, q in list(model.named_parameters()) + [("likelihood." + k, q) for k, q in lh.named_parameters()])
    assert all(id(q) in grads for q in ps), [names[id(q)] for q in ps if id(q) not in grads]
    f64 = lambda t: t.detach().cpu().double().numpy()
    v = float(torch.sigmoid(model.data_kernel.raw_vol.detach().double()))
    v32 = float(torch.sigmoid(model.data_kernel.raw_vol.detach()).float())
    abc = tuple(f64(t) for t in (lh.trans_a, lh.trans_b, lh.trans_c)) if param == "cv" else None
    ghx, ghw = MR.gauss_hermite(75)
    c = np.array([float(m.constant.detach()) for m in model.mean_module.base_means])
    ref = MM.step(p["x"], v32, J, c, p["M"], p["rho"], p["gam"], p["Lt"], p["f"], p["raw_var"], p["y"], ghx, ghw, 1.0 / n,
                  1.0 / (n * T), abc=abc)
    assert abs(float(val) - ref["F"]) <= MM.SCALAR_TOL * max(1.0, abs(ref["F"]))
    want = {"variational_mean": ref["grad_M"], "log_diag_precision_root": ref["grad_rho"], "coupling": ref["grad_gamma"],
            "variational_task_covar_root": ref["grad_Lt"], "index_kernel.covar_factor": ref["grad_f"].reshape(T, 1),
            "index_kernel.raw_var": ref["grad_raw_var"], "data_kernel.raw_vol": np.array([ref["dFdv"] * v * (1 - v)])}
    want.update({f"mean_module.base_means.{t}.constant": np.array(ref["grad_c"][t]) for t in range(T)})
    if param == "cv":
        sig = lambda t: 1.0 / (1.0 + np.exp(-f64(t)))
        sb, sc = sig(lh.raw_b), sig(lh.raw_c)
        want.update({"likelihood.raw_a": ref["grad_abc"][:, 0] * sig(lh.raw_a), "likelihood.raw_b": ref["grad_abc"][:, 1] * 3 * sb * (1 - sb),
                     "likelihood.raw_c": ref["grad_abc"][:, 2] * 6 * sc * (1 - sc)})
    seen = set()
    scale_c = np.abs(ref["grad_c"]).max()
    for q in ps:
        k = names[id(q)]
        denom = scale_c if k.startswith("mean_module") else np.abs(want[k]).max()   # (grad_c is ONE gradient of T entries)
        err = np.abs(f64(grads[id(q)]).reshape(np.shape(want[k])) - want[k]).max() / denom
        print(f"  grad {k}: {err:.2e}")
        assert err < MM.GRAD_TOL, (k, err)
        seen.add(k)
    assert seen == set(want)
    kl = model.kl_divergence()
    assert abs(float(kl) - ref["kl"]) <= MM.SCALAR_TOL * max(1.0, abs(ref["kl"]))


@pytest.mark.parametrize("n,Kc", [(399, 0), (130, 5), (1, 0)])
def test_one_task_with_unit_task_covariances_is_within_the_bounds_of_the_single_task_restatement(n, Kc):
    """T = 1 with K_t = S_t = 1 (f = 0, raw_var = log(e - 1), Lt = 1): the step against gpcv_markov_ref.step, same bounds."""
    from volt_amd import ops
    ghx, ghw = MR.gauss_hermite(75)
    p = MR.make_inputs(n, 60 + n, x0_zero=n % 2 == 1)
    abc1 = MR.make_abc(Kc, n) if Kc else None
    we, wk = 1.0 / n, 0.7 / (n + 3)
    one = MR.step(p["x"], p["v"], J, p["mu"], p["m"], p["rho"], p["gam"], p["y"], ghx, ghw, we, wk, abc=abc1)
    abc = dev(np.stack(abc1)[None]) if Kc else None                              # [1,3,Kc]
    ws = ops.gpcv_mt_markov_step(dev(p["x"]), dev([p["v"]]), dev(p["m"][:, None]), dev([p["mu"]]), dev(p["rho"]), dev(p["gam"]),
                                 dev([[1.0]]), dev([0.0]), dev([math.log(math.e - 1.0)]), dev(p["y"][:, None]), dev(ghx), dev(ghw),
                                 abc=abc, jitter=J, w_ell=we, w_kl=wk)
    torch.cuda.synchronize()
    assert not ws.info.any()
    o = outputs(ws)
    for k, k1 in (("ell", "ell"), ("kl", "kl"), ("quad", "quad"), ("logdet_km", "logdet_k"), ("logdet_sx", "logdet_s"),
                  ("tau_x", "trace"), ("F", "F")):
        assert abs(o[k] - one[k1]) <= MM.SCALAR_TOL * max(1.0, abs(one[k1])), (k, o[k], one[k1])
    if one["dFdv"] == 0.0:
        assert o["dFdv"] == 0.0
    else:
        assert abs(o["dFdv"] - one["dFdv"]) <= MM.DV_TOL * abs(one["dFdv"])
    for k, k1 in (("grad_M", "grad_m"), ("grad_rho", "grad_rho")) + ((("grad_gamma", "grad_gamma"),) if n > 1 else ()):
        assert np.abs(o[k].reshape(-1) - one[k1]).max() <= MM.GRAD_TOL * np.abs(one[k1]).max(), k
    assert abs(o["grad_c"][0] - one["grad_mu"].sum()) <= MM.GRAD_TOL * abs(one["grad_mu"].sum())
    assert np.abs(ws.s.cpu().numpy() - one["s"]).max() <= 1e-12 * one["s"].max()
    if Kc:
        assert np.abs(o["grad_abc"][0] - one["grad_abc"]).max() <= MM.ABC_TOL * np.abs(one["grad_abc"]).max()


def test_latent_variance_equals_the_steps_s_st_and_samples_have_it():
    n, T = 399, 2
    p, ref, we, wk = case(n, T)
    ws = run(p, we, wk, nan_gamma=False)
    model, lh = _model(p)
    lat = model(dev(p["x"]))
    st = dev(p["Lt"], torch.float64).tril().pow(2).sum(-1)
    assert torch.equal(lat.variance, (ws.s.unsqueeze(-1) * st.unsqueeze(-2)).to(torch.float32).clamp_min(1e-6))
    assert tuple(lat.event_shape) == (n, T) and lat.num_tasks == T
    torch.manual_seed(2)
    F = lat.rsample(torch.Size([4000]))
    assert tuple(F.shape) == (4000, n, T)
    want = ref["s"][:, None] * (np.tril(p["Lt"]) ** 2).sum(1)[None, :]
    sv = F.double().var(0).cpu().numpy()
    assert np.abs(sv / want - 1).max() < 6 * math.sqrt(2.0 / 4000)                  # a sample variance: sd sqrt(2 / S) relative
    assert np.abs(F.double().mean(0).cpu().numpy() - p["M"]).max() < 6 * np.sqrt(want.max() / 4000)
    # the two tasks of one draw are correlated through Lt: cov(F_n0, F_n1) = s_n (Lt Lt')_01
    cov01 = ((F[:, :, 0].double() - dev(p["M"][:, 0], torch.float64)) * (F[:, :, 1].double() - dev(p["M"][:, 1], torch.float64))).mean(0)
    St = np.tril(p["Lt"]) @ np.tril(p["Lt"]).T
    sd = ref["s"] * math.sqrt((St[0, 0] * St[1, 1] + St[0, 1] ** 2) / 4000)           # sd of a sample covariance of two Gaussians
    assert (np.abs(cov01.cpu().numpy() - ref["s"] * St[0, 1]) < 6 * sd).all()
    S = lat._covar.double().cpu().numpy()                                           # dense only on request
    assert np.abs(np.diag(S).reshape(n, T) - want).max() <= 1e-5 * want.max()


# ------------------------------------------------------------------------------------------------ trainer and drivers
def _prices(n, seed):
    from volt_amd.synthetic import sde_series
    return torch.tensor(sde_series(n, seed)[0])


@functools.lru_cache(maxsize=None)
def _fit_reference(n, T, iters=40):
    """The start-up values FitGPCVMultitask(solver="markov") makes, and fp64 Adam on the restatement from them."""
    from volt_amd.train_utils import FitGPCVMultitask
    F = torch.stack([_prices(n, 2021 + i) for i in range(T)])                      # [T, n + 1] prices
    x = torch.arange(n, dtype=torch.float32) / 252                                  # (x_0 = 0: valid under the level's jitter)
    torch.manual_seed(9)
    m0, _, _ = FitGPCVMultitask(x.to(DEV), F.to(DEV), train_iters=0, solver="markov")
    f64 = lambda t: t.detach().cpu().double().numpy()
    yy = f64(((F[:, 1:] - F[:, :-1]) / F[:, :-1] / (x[1] - x[0]) ** 0.5).t())       # the scaled returns, in fp32 as the fit forms them
    c0 = np.array([float(m.constant.detach()) for m in m0.mean_module.base_means])
    start = (f64(m0.variational_mean), f64(m0.log_diag_precision_root), f64(m0.coupling), f64(m0.variational_task_covar_root), c0,
             f64(m0.index_kernel.covar_factor).reshape(-1), f64(m0.index_kernel.raw_var))
    return x, F, MM.learn(f64(x), yy, start, iters)


def _fit_errors(model, ps):
    f64 = lambda t: t.detach().cpu().double().numpy()
    c = np.array([float(m.constant.detach()) for m in model.mean_module.base_means])
    got = (f64(model.variational_mean), f64(model.log_diag_precision_root), f64(model.coupling), f64(model.variational_task_covar_root),
           c, f64(model.index_kernel.covar_factor).reshape(-1), f64(model.index_kernel.raw_var), f64(model.data_kernel.raw_vol))
    names = ("mean", "rho", "gamma", "Lt", "const", "covar_factor", "raw_var", "raw_vol")
    return {k: float(np.abs(g.reshape(w.shape) - w).max()) for k, g, w in zip(names, got, ps)}


@pytest.mark.parametrize("n,T", [(130, 3), (399, 8)])
def test_fit_multitask_markov_tracks_fp64_adam_and_captured_equals_eager(n, T, monkeypatch):
    """FitGPCVMultitask(solver="markov") for 40 Adam iterations against fp64 Adam on the restatement from the same start,
    with tests/test_gpu_gpcv_markov.py's trainer bounds -- losses 5e-4 (of max(1, |loss|)), every parameter 5e-3 -- for the
    eager loop (torch.optim.Adam, every loss) AND for the captured loop (optim.FusedAdam; it returns its last loss).  Then: the
    captured loop equals an eager one bit for bit when both run the same optimiser arithmetic."""
    from volt_amd import train_utils
    from volt_amd.train_utils import FitGPCVMultitask
    iters = 40
    x, F, (rec, ps) = _fit_reference(n, T)

    def fit(graph):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.manual_seed(9)
            return FitGPCVMultitask(x.to(DEV), F.to(DEV), train_iters=iters, solver="markov", graph=graph)

    model, lh, losses = fit(False)
    assert model.prior_solver == "markov" and len(losses) == iters
    got = torch.stack(losses).cpu().double().reshape(-1)
    w = torch.tensor(rec, dtype=torch.float64)
    err = float(((got - w).abs() / w.abs().clamp_min(1.0)).max())
    errs = _fit_errors(model, ps)
    print(f"fit eager {n} x {T}: loss {err:.2e} " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert err < 5e-4 and max(errs.values()) < 5e-3, (err, errs)
    captured, _, lc = fit(True)                                  # the default optimiser of a captured loop: FusedAdam
    lerr = abs(float(lc[-1]) - rec[-1]) / max(1.0, abs(rec[-1]))
    errs = _fit_errors(captured, ps)
    print(f"fit captured {n} x {T}: last loss {lerr:.2e} " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert len(lc) == 1 and lerr < 5e-4 and max(errs.values()) < 5e-3, (lerr, errs)
    adam = train_utils._adam
    monkeypatch.setattr(train_utils, "_adam", lambda params, lr, graph: adam(params, lr, True))
    eager, _, le = fit(False)                                    # eager, with the captured loop's optimiser
    assert torch.equal(le[-1], lc[-1])
    for a, b in zip(eager.parameters(), captured.parameters()):
        assert torch.equal(a, b)


def test_learn_multitask_markov_returns_a_positive_scale():
    from volt_amd.train_utils import LearnGPCVMultitask
    n, T = 200, 3
    x = (torch.arange(n, dtype=torch.float32) / 252).to(DEV)
    F = torch.stack([_prices(n, 2019 + i) for i in range(T)]).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vol = LearnGPCVMultitask(x, F, train_iters=15, solver="markov")
        volc = LearnGPCVMultitask(x, F, train_iters=15, solver="markov", param="cv", K=1, train_likelihood=True)
    for v in (vol, volc):
        assert tuple(v.shape) == (T, n) and torch.isfinite(v).all() and bool((v > 0).all())


def test_stocks_driver_with_the_markov_joint_model(tmp_path):
    from volt_amd.forecast import GenerateStockPredictionsBatch
    from volt_amd.synthetic import sde_batch
    from volt_amd.train_utils import LearnGPCVMultitask
    B, T, ntrain, H, S = 3, 70, 64, 4, 5
    _, F, _ = sde_batch(B, T - 1, seed=77)
    closes = torch.as_tensor(np.asarray(F)).to(DEV)
    g = torch.Generator(device="cuda").manual_seed(1)
    debug = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(17)
        out = GenerateStockPredictionsBatch(["AAA", "BBB", "CCC"], closes, forecast_horizon=H, train_iters=3, nsample=S,
                                            ntrain=ntrain, mean="ewma", save=True, k=10, ntimes=1, vol_iters=2,
                                            par_dir=str(tmp_path), generator=g, multitask_gpcv="markov", debug=debug)
        x = torch.arange(ntrain - 1, device=DEV) * (1. / 252)
        torch.manual_seed(17)
        vol = LearnGPCVMultitask(x, debug["train_y"], train_iters=3, solver="markov")
    assert tuple(out.shape) == (B, S, H) and torch.isfinite(out).all()
    assert torch.equal(debug["vol"], vol)                        # the window's vol paths ARE the Markov joint model's


# ------------------------------------------------------------------------------------------------ failures
def test_nan_and_a_non_positive_task_pivot_raise():
    from volt_amd.forecast import GenerateStockPredictionsBatch
    from volt_amd.safe import NanError, NotPSDError
    from volt_amd.train_utils import FitGPCVMultitask
    n, T = 65, 3
    p, ref, we, wk = case(n, T)
    x, yy = dev(p["x"]), dev(p["y"])
    model, lh = _model(p)
    with torch.no_grad():
        model.variational_mean[7, 1] = float("nan")
    with pytest.raises(NanError):
        _elbo_and_grads(model, lh, x, yy, n * T)
    model, lh = _model(p)
    with torch.no_grad():                                        # K_t = f f' + diag softplus(raw_var): softplus(-200) = 0 in fp64
        model.index_kernel.covar_factor.zero_()
        model.index_kernel.raw_var[1] = -800.0
    with pytest.raises(NotPSDError, match="K_t"):
        _elbo_and_grads(model, lh, x, yy, n * T)
    bad = dict(p, raw_var=p["raw_var"].copy(), f=np.zeros(T))
    bad["raw_var"][1] = -800.0
    ws = run(bad, we, wk)
    assert ws.info.tolist() == [1, 2]                            # F is not finite; the first bad pivot is task 1's
    bad = dict(p, v=float("nan"))
    assert run(bad, we, wk).info.tolist() == [1, 0]
    with pytest.raises(ValueError, match="kernel='bm'"):
        FitGPCVMultitask(x, torch.ones(T, n + 1, device=DEV), kernel="fbm", solver="markov")
    with pytest.raises(ValueError, match='gpcv_solver="markov"'):
        GenerateStockPredictionsBatch(["a", "b"], torch.ones(2, 40, device=DEV), ntrain=30, multitask_gpcv="markov",
                                      gpcv_solver="markov")


# ------------------------------------------------------------------------------------------------ memory
def test_fit_at_65536_by_8_peaks_under_one_gib():
    """FitGPCVMultitask(solver="markov") for 3 iterations at N = 65536, T = 8: the peak allocation above the inputs stays
    under 1 GiB.  A condition, not a measurement: one [N,N] fp32 array is 16 GiB, an [N,T] array 2 - 4 MiB."""
    from volt_amd.train_utils import FitGPCVMultitask
    n, T = 65536, 8
    g = torch.Generator().manual_seed(3)
    F = torch.exp(torch.cumsum(0.01 * torch.randn(T, n + 1, generator=g, dtype=torch.float64), -1)).float().to(DEV)
    x = (torch.arange(n, dtype=torch.float32) / 252).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model, lh, losses = FitGPCVMultitask(x, F, train_iters=3, solver="markov", graph=False)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"{n} x {T}: peak allocation above the inputs {peak / 2 ** 20:.1f} MiB; losses {[float(v) for v in losses]}")
    assert len(losses) == 3 and all(math.isfinite(float(v)) for v in losses)
    assert all(torch.isfinite(q).all() for q in model.parameters())
    assert peak < 2 ** 30
