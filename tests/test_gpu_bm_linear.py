"""The linear-time Brownian-motion solver on the MI355X (csrc/bm.hip, ops.bm_step / ops.bm_solve, BMGP(solver="linear"),
TrainVolModel(solver="linear")) against the fp64 restatement of its recurrences (tests/bm_chain_ref.py, itself checked
against dense fp64 LAPACK in tests/test_bm_chain_host.py) and against the dense path.

Tolerances.  The kernels' arithmetic is fp64 whatever the I/O type, so
  * fp64 entry points: 1e-10 of the quantity's scale at N <= 1024 and 1e-8 at N = 4096 and above -- the gates
    include/volt_hip.h states for the dense fp64 step (scale: bm_chain_ref.out_scales; max |.| for a vector);
  * fp32 entry points: 2^-23 |ref| (one rounding of the output) plus that fp64 term, element by element.
Every input is an fp32-representable number, so the fp32 and fp64 runs and the reference see the same values."""
import functools

import numpy as np
import pytest
import torch

import bm_chain_ref as ref

pytestmark = pytest.mark.gpu

NOISES = (1e-4, 1e-2, 0.69)
BMAX = 130
EPS32 = 2.0 ** -23


def f64_tol(n):
    return 1e-10 if n <= 1024 else 1e-8


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a)).to(dtype).cuda()


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(n, gname, B=BMAX, seed=0):
    """Inputs (fp32-representable, as float64 arrays) and the restatement's outputs for B series over one grid: series b has
    vol 0.1 .. 0.9 and the noise level NOISES[b % 3].  Computed once, shared by the fp32 and fp64 tests and by every B (the
    series are independent: the first B rows are the case of B series)."""
    rng = np.random.default_rng(seed + n)
    x = f32(ref.grids(n)[gname])
    assert (np.diff(x) > 0).all() and x[0] >= 0
    vol = f32(rng.uniform(0.1, 0.9, B))
    s2 = f32(np.array([NOISES[b % 3] for b in range(B)]))
    r = f32(np.cumsum(rng.standard_normal((B, n)) * 0.05, axis=1) - 2.0)
    out, alpha, info = ref.bm_step_ref(x, vol, s2, r)
    assert not info.any()
    for a in (x, vol, s2, r, out, alpha):
        a.setflags(write=False)
    return x, vol, s2, r, out, alpha


def check_step(got_out, got_alpha, out, alpha, n, dtype):
    tol = f64_tol(n)
    scale = ref.out_scales(out, n)
    eps = EPS32 if dtype == torch.float32 else 0.0
    err = np.abs(got_out[:, :6] - out[:, :6])
    bound = eps * np.abs(out[:, :6]) + tol * scale
    assert (err <= bound).all(), (np.argwhere(err > bound)[:4], (err / bound).max())
    np.testing.assert_array_equal(got_out[:, 6:8].astype(np.float64), out[:, 6:8])        # the parameters the step used
    aerr = np.abs(got_alpha - alpha)
    abound = eps * np.abs(alpha) + tol * np.abs(alpha).max(1, keepdims=True)
    assert (aerr <= abound).all(), (aerr / abound).max()
    return float((err / np.maximum(scale, 1e-300)).max()), float((aerr / np.abs(alpha).max(1, keepdims=True)).max())


# ------------------------------------------------------------------------------------------------ ops.bm_step
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 399, 4096])
def test_bm_step_matches_the_restatement(n, dtype):
    from volt_amd import ops
    worst = (0.0, 0.0)
    for gname in ("uniform_zero", "uniform_dt", "irregular_zero", "irregular_dt"):
        x, vol, s2, r, out, alpha = case(n, gname)
        for B, lo in ((1, 0), (1, 1), (1, 2), (3, 0), (64, 0), (65, 0), (130, 0)):      # B = 1 at each of the noise levels
            sl = slice(lo, lo + B)
            o, a, info = ops.bm_step(dev(x, dtype), dev(vol[sl], dtype), dev(s2[sl], dtype), dev(r[sl], dtype))
            assert o.dtype == dtype and a.dtype == dtype and not info.any()
            w = check_step(o.cpu().numpy().astype(np.float64), a.cpu().numpy().astype(np.float64), out[sl], alpha[sl], n, dtype)
            worst = max(worst[0], w[0]), max(worst[1], w[1])
    print(f"bm_step N = {n} {dtype}: worst error / scale  out {worst[0]:.2e}  alpha {worst[1]:.2e}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("B,n", [(1, 1), (3, 65), (65, 399), (130, 63)])
def test_bm_step_writes_nothing_past_its_buffers_and_repeats_bitwise(B, n, dtype):
    """NaN sentinels behind out, alpha and info (and 0xFF bytes behind the workspace) survive; ten runs agree bit for bit."""
    from volt_amd import _lib, ops
    x, vol, s2, r, out, alpha = case(n, "irregular_dt")
    ws = ops.BmWorkspace(B, n, "cuda", dtype)
    nbytes = int(_lib.lib().volt_bm_workspace_bytes(B, n, 1))
    ws.buf.fill_(0xFF)
    guard = 64
    obuf = torch.full((B * 8 + guard,), float("nan"), dtype=dtype, device="cuda")
    abuf = torch.full((B * n + guard,), float("nan"), dtype=dtype, device="cuda")
    ibuf = torch.full((B + guard,), -77, dtype=torch.int32, device="cuda")
    ws.out, ws.alpha, ws.info = obuf[:B * 8].view(B, 8), abuf[:B * n].view(B, n), ibuf[:B]
    args = (dev(x, dtype), dev(vol[:B], dtype), dev(s2[:B], dtype), dev(r[:B], dtype), ws)
    o, a, info = ops.bm_step(*args)
    assert o.data_ptr() == obuf.data_ptr() and a.data_ptr() == abuf.data_ptr()
    first = (o.clone(), a.clone(), info.clone())
    check_step(o.cpu().numpy().astype(np.float64), a.cpu().numpy().astype(np.float64), out[:B], alpha[:B], n, dtype)
    for _ in range(9):
        obuf[:B * 8].fill_(float("nan"))
        abuf[:B * n].fill_(float("nan"))
        o, a, info = ops.bm_step(*args)
        assert torch.equal(o, first[0]) and torch.equal(a, first[1]) and torch.equal(info, first[2])
    assert torch.isnan(obuf[B * 8:]).all() and torch.isnan(abuf[B * n:]).all() and bool((ibuf[B:] == -77).all())
    off = ws.ptr - ws.buf.data_ptr()
    assert bool((ws.buf[off + nbytes:] == 0xFF).all()) and bool((ws.buf[:off] == 0xFF).all())
    # without VOLT_WANT_GRAD: the forward scalars only
    obuf.fill_(float("nan"))
    abuf.fill_(float("nan"))
    o, a, info = ops.bm_step(*args, want_grad=False)
    assert torch.equal(o[:, [0, 2, 3, 6, 7]], first[0][:, [0, 2, 3, 6, 7]]) and torch.isnan(o[:, [1, 4, 5]]).all()
    assert torch.isnan(abuf).all() and not info.any()


def test_bm_step_info():
    from volt_amd import ops
    n = 70
    x, vol, s2, r, out, alpha = case(n, "uniform_zero")
    rr = r[:3].copy()
    rr[1, 40] = np.nan                                            # a NaN residual is not a pivot failure: info 0, NaN out
    o, a, info = ops.bm_step(dev(x), dev(vol[:3]), dev(s2[:3]), dev(rr))
    assert info.tolist() == [0, 0, 0]
    assert torch.isnan(o[1, 0]) and torch.isnan(o[1, 2]) and torch.isfinite(o[1, 3]) and torch.isnan(a[1]).any()
    assert torch.isfinite(o[[0, 2]]).all() and torch.isfinite(a[[0, 2]]).all()
    s0 = s2[:3].copy()
    s0[2] = 0.0                                                   # s = 0 at x_0 = 0: d_0 = 0
    o, a, info = ops.bm_step(dev(x), dev(vol[:3]), dev(s0), dev(r[:3]))
    assert info.tolist() == [0, 0, 1] and torch.isnan(o[2, 0]) and torch.isnan(o[2, 3]) and torch.isfinite(o[:2]).all()
    vn = vol[:3].copy()
    vn[0] = np.nan
    _, _, info = ops.bm_step(dev(x), dev(vn), dev(s2[:3]), dev(r[:3]))
    assert info.tolist() == [1, 0, 0]                             # d_0 = NaN x_0 + s is NaN at x_0 = 0 as well


# ------------------------------------------------------------------------------------------------ against the dense path
@pytest.mark.parametrize("B,n", [(1, 399), (8, 399), (2, 4096)])
def test_linear_step_is_at_least_as_accurate_as_the_dense_fp32_step(B, n):
    """Side by side on the same fp32 inputs: the linear step's error against the dense fp64 step is at most the dense fp32
    step's own, quantity by quantity, margin 1 -- its arithmetic is fp64, so a larger error is a bug, not noise."""
    from volt_amd import ops
    x, vol, s2, r, _, _ = case(n, "uniform_dt", B=8, seed=3)
    xt, v, s, rt = dev(x), dev(vol[:B]), dev(np.full(B, NOISES[2])), dev(r[:B])
    M = torch.minimum(xt.double()[:, None], xt.double()[None, :])
    K64 = v.double().reshape(B, 1, 1) * M
    o64, a64, i64 = (t.clone() for t in ops.mll_step(K64, rt.double(), s.double()))
    o32, a32, i32 = (t.clone() for t in ops.mll_step(K64.float(), rt, s))
    ol, al, il = ops.bm_step(xt, v, s, rt)
    assert not i64.any() and not i32.any() and not il.any()
    names = ("mll", "dmll/dsigma2", "quad", "logdet", "tr", "alpha'alpha")
    for k, name in enumerate(names):
        e_lin = float((ol[:, k].double() - o64[:, k]).abs().max())
        e_dense = float((o32[:, k].double() - o64[:, k]).abs().max())
        print(f"{B} x {n} {name:13s}: linear {e_lin:.3e}  dense fp32 {e_dense:.3e}  (|ref| {float(o64[:, k].abs().max()):.3e})")
        assert e_lin <= e_dense, (name, e_lin, e_dense)
    e_lin, e_dense = float((al.double() - a64).abs().max()), float((a32.double() - a64).abs().max())
    print(f"{B} x {n} alpha        : linear {e_lin:.3e}  dense fp32 {e_dense:.3e}  (|ref| {float(a64.abs().max()):.3e})")
    assert e_lin <= e_dense


# ------------------------------------------------------------------------------------------------ ops.bm_solve
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [1, 20, 65])
def test_bm_solve_matches_the_restatement(H, dtype):
    from volt_amd import ops
    for n, B, gname in ((1, 1, "uniform_dt"), (3, 2, "irregular_zero"), (65, 3, "uniform_zero"), (399, 5, "irregular_dt"),
                        (130, 65, "uniform_dt")):
        x, vol, s2, _, _, _ = case(n, gname)
        rng = np.random.default_rng(H + n)
        R = f32(rng.standard_normal((B, n, H)))
        R[0] = f32(vol[0] * x)[:, None]                           # forecasting: x* beyond the grid, every column of K_t* equal
        X, info = ref.bm_solve_ref(x, vol[:B], s2[:B], R)
        got, ginfo = ops.bm_solve(dev(x, dtype), dev(vol[:B], dtype), dev(s2[:B], dtype), dev(R, dtype))
        assert got.dtype == dtype and tuple(got.shape) == (B, n, H) and not ginfo.any()
        err = np.abs(got.cpu().numpy().astype(np.float64) - X)
        bound = (EPS32 if dtype == torch.float32 else 0.0) * np.abs(X) + f64_tol(n) * np.abs(X).max((1, 2), keepdims=True)
        assert (err <= bound).all(), (n, B, H, (err / bound).max())
    s0 = s2[:B].copy()
    s0[1] = np.nan
    _, ginfo = ops.bm_solve(dev(x, dtype), dev(vol[:B], dtype), dev(s0, dtype), dev(R, dtype))
    assert ginfo[1] == 1 and int((ginfo != 0).sum()) == 1


# ------------------------------------------------------------------------------------------------ BMGP(solver="linear")
def _bmgp(x, y, solver, dtype=torch.float32):
    from volt_amd.gp import GaussianLikelihood
    from volt_amd.models import BMGP
    bs = torch.Size(y.shape[:-1])
    lh = GaussianLikelihood(batch_shape=bs).cuda().to(dtype)
    m = BMGP(dev(x, dtype), dev(y, dtype), lh, solver=solver).cuda().to(dtype)
    with torch.no_grad():
        if len(bs):
            m.covar_module.raw_vol.copy_(torch.linspace(-1.5, 0.5, bs[0], dtype=dtype).reshape(-1, 1))
            lh.raw_noise.copy_(torch.linspace(-3.0, 0.0, bs[0], dtype=dtype).reshape(-1, 1))
        else:
            m.covar_module.raw_vol.fill_(-0.7)
            lh.raw_noise.fill_(-2.0)
    return m, lh


def _mll_and_grads(m, lh):
    from volt_amd.gp import ExactMarginalLogLikelihood
    m.train()
    for p in (m.covar_module.raw_vol, lh.raw_noise):
        p.grad = None
    val = ExactMarginalLogLikelihood(lh, m)(m(m.train_inputs[0][:, 0]), m.train_targets)
    val.sum().backward()
    return val.detach(), m.covar_module.raw_vol.grad.clone(), lh.raw_noise.grad.clone()


def _autograd_ref(x, y, raw_vol, raw_noise):
    """fp64 CPU autograd through the dense definition, one series."""
    xt, yt = torch.tensor(x, dtype=torch.float64), torch.tensor(y, dtype=torch.float64)
    rv = torch.tensor(float(raw_vol.detach()), dtype=torch.float64, requires_grad=True)
    rn = torch.tensor(float(raw_noise.detach()), dtype=torch.float64, requires_grad=True)
    v = torch.sigmoid(rv)
    A = v * torch.minimum(xt[:, None], xt[None, :]) + (torch.nn.functional.softplus(rn) + 1e-4) * torch.eye(len(x), dtype=torch.float64)
    val = torch.distributions.MultivariateNormal(-0.5 * v ** 2 * xt, covariance_matrix=A).log_prob(yt) / len(x)
    gv, gn = torch.autograd.grad(val, (rv, rn))
    return float(val), float(gv), float(gn)


@pytest.mark.parametrize("dtype,vtol,gtol", [(torch.float32, 2e-5, 2e-3), (torch.float64, 1e-9, 1e-8)], ids=["f32", "f64"])
def test_bmgp_linear_mll_and_gradients(dtype, vtol, gtol):
    """MLL and every gradient through autograd against fp64 autograd of the dense definition.  fp32 model: the dense
    path's stated tolerances (tests/test_gpu_api.py: 2e-5 on the value, 2e-3 on a gradient -- the parameters, the mean and
    the residual are formed in fp32 by torch before the step sees them); fp64 model: the reference's own accuracy."""
    n, T = 200, 3
    x = f32(ref.grids(n)["irregular_dt"])
    y = f32(np.cumsum(np.random.default_rng(4).standard_normal((T, n)) * 0.05, axis=1) - 2.0)
    mb, lb = _bmgp(x, y, "linear", dtype)
    vb, gvb, gnb = _mll_and_grads(mb, lb)
    for t in range(T):
        m1, l1 = _bmgp(x, y[t], "linear", dtype)
        with torch.no_grad():
            m1.covar_module.raw_vol.copy_(mb.covar_module.raw_vol[t])
            l1.raw_noise.copy_(lb.raw_noise[t])
        v1, gv1, gn1 = _mll_and_grads(m1, l1)
        want = _autograd_ref(x, y[t], mb.covar_module.raw_vol[t], lb.raw_noise[t])
        for got, w, tol in ((v1, want[0], vtol), (gv1, want[1], gtol), (gn1, want[2], gtol)):
            assert abs(float(got) - w) <= tol * max(abs(w), 1.0 if tol == vtol else 1e-3), (t, float(got), w)
        # batched == per-series: the lanes of the step do not know about each other
        assert float(vb[t]) == float(v1)
        assert abs(float(gvb[t]) - float(gv1)) <= 1e-6 * abs(float(gv1)) and abs(float(gnb[t]) - float(gn1)) <= 1e-6 * abs(float(gn1))


def test_bmgp_linear_saves_one_packed_tensor_and_defers_checks():
    from volt_amd import gp
    n = 64
    x = f32(ref.grids(n)["uniform_zero"])
    m, lh = _bmgp(x, np.full(n, -2.0), "linear")
    m.train()
    mll = gp.ExactMarginalLogLikelihood(lh, m)
    val = mll(m(m.train_inputs[0][:, 0]), m.train_targets)
    fn = val.grad_fn
    while fn is not None and "ChainMLL" not in type(fn).__name__:
        fn = fn.next_functions[0][0] if fn.next_functions else None
    assert fn is not None and len(fn.saved_tensors) == 1 and tuple(fn.saved_tensors[0].shape) == (1, 8 + n)
    assert isinstance(m(m.train_inputs[0][:, 0]).lazy_covariance_matrix, gp._BrownianPrior)
    # a NaN target: NanError at once; under deferred_checks nothing is read back (a NaN residual is not a pivot failure)
    with torch.no_grad():
        lh.noise_covar.raw_noise.fill_(float("nan"))
    with pytest.raises(gp.NanError):
        mll(m(m.train_inputs[0][:, 0]), m.train_targets)
    with gp.deferred_checks(immediate=True) as chk:
        with pytest.raises(gp.NanError):
            mll(m(m.train_inputs[0][:, 0]), m.train_targets)
        chk.immediate = False
        mll(m(m.train_inputs[0][:, 0]), m.train_targets)
        assert chk.any_bad() == 1
        with pytest.raises(gp.NotPSDError):
            chk.raise_if_bad()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [20, 65])
def test_bmgp_linear_posterior(H, dtype):
    """posterior_call against the fp64 dense posterior, one series and batched, test points inside and beyond the training
    range.  fp64 model: 1e-9 of the scale.  fp32 model: alpha and K_*t are fp64 inside, so what is rounded to fp32 is
    the residual y - m (3 roundings of 2^-24 |y|), m(x*) and the output; the posterior mean is a smoother with non-negative
    weights summing to at most one, so they pass through with gain <= 1: 8 x 2^-24 max |y|.  The covariance sees
    K_t* (2 roundings), X (1) and the output (1) through the same weights at max K_**: 8 x 2^-24 max K_**.  Against solver="dense": that path's stated tolerances (tests/test_gpu_gpcv.py)."""
    n, T = 399, 3
    x = f32(ref.grids(n)["uniform_dt"])
    y = f32(np.cumsum(np.random.default_rng(8).standard_normal((T, n)) * 0.05, axis=1) - 2.0)
    inside = 0.5 * (x[10:10 + H // 2] + x[11:11 + H // 2]) if H > 20 else 0.5 * (x[200:205] + x[201:206])
    xs = f32(np.concatenate([inside, x[-1] + (1 + np.arange(H - len(inside))) / 252.0]))
    for yy in (y, y[1]):
        m, lh = _bmgp(x, yy, "linear", dtype)
        md, ld = _bmgp(x, yy, "dense", torch.float32)
        m.eval(), md.eval()
        post, postd = m(dev(xs, dtype)), md(dev(xs))
        vol = m.covar_module.vol.detach().double().cpu().reshape(-1)
        noise = lh.noise.detach().double().cpu().reshape(-1)
        y2 = np.atleast_2d(yy)
        assert post.mean.dtype == dtype and tuple(post.mean.shape) == tuple(yy.shape[:-1]) + (H,)
        assert tuple(post.covariance_matrix.shape) == tuple(yy.shape[:-1]) + (H, H)
        mean, cov = post.mean.double().cpu().reshape(-1, H), post.covariance_matrix.double().cpu().reshape(-1, H, H)
        for t in range(y2.shape[0]):
            wm, wc = ref.dense_posterior(x, float(vol[t]), float(noise[t]), y2[t], xs)
            if dtype == torch.float64:
                mtol, ctol = 1e-9 * np.abs(wm).max(), 1e-9 * np.abs(wc).max()
            else:
                mtol, ctol = 8 * 2.0 ** -24 * np.abs(y2[t]).max(), 8 * 2.0 ** -24 * float(vol[t]) * xs.max()
            assert np.abs(mean[t].numpy() - wm).max() <= mtol, (t, np.abs(mean[t].numpy() - wm).max(), mtol)
            assert np.abs(cov[t].numpy() - wc).max() <= ctol, (t, np.abs(cov[t].numpy() - wc).max(), ctol)
        dm, dc = postd.mean.double().cpu().reshape(-1, H), postd.covariance_matrix.double().cpu().reshape(-1, H, H)
        assert float((mean - dm).abs().max()) < 2e-3
        assert float((cov - dc).abs().max()) < 2e-3 * float(dc.abs().max()) + 1e-6
    assert torch.isfinite(post.sample(torch.Size((4,)))).all()


# ------------------------------------------------------------------------------------------------ trainers
def _adam_on_the_restatement(x, y, iters, lr):
    """fp64 torch.optim.Adam on -sum_b mll_b with the gradients of the restatement's closed forms; y [T,N]."""
    T, n = y.shape
    rv = torch.full((T,), float(np.log(0.2 / 0.8)), dtype=torch.float64, requires_grad=True)       # BMKernel(vol=0.2)
    rn = torch.zeros(T, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([rv, rn], lr=lr)
    for _ in range(iters):
        opt.zero_grad()
        v = torch.sigmoid(rv).detach().numpy()
        s = (torch.nn.functional.softplus(rn) + 1e-4).detach().numpy()
        out, alpha, _ = ref.bm_step_ref(x, v, s, y + 0.5 * (v * v)[:, None] * x[None, :])
        dv = ref.dvol_ref(out, v, n) + (alpha / n * (-v[:, None] * x[None, :])).sum(1)
        rv.grad = torch.tensor(-dv * v * (1 - v))
        rn.grad = torch.tensor(-out[:, 1]) * torch.sigmoid(rn.detach())
        opt.step()
    return rv.detach().numpy(), rn.detach().numpy()


@pytest.fixture(scope="module")
def trained_reference():
    from volt_amd.synthetic import sde_batch
    from volt_amd.train_utils import LR_VOL
    T, n, iters = 3, 399, 40
    x, F, vol = sde_batch(T, n, seed=21)
    x, vol = f32(x), f32(vol)
    return x, vol, iters, _adam_on_the_restatement(x, np.log(vol.astype(np.float32)).astype(np.float64), iters, LR_VOL)


@pytest.mark.parametrize("graph", [False, True, None], ids=["eager", "captured", "auto"])
def test_train_vol_model_linear_matches_fp64_adam(trained_reference, graph):
    """40 iterations, eager and captured, against fp64 Adam on the restatement: 2e-3 on the raw parameters, the bound of the
    existing vol-model trainer test (tests/test_gpu_multitask.py).  graph=None captures too (the step is launch-bound)."""
    from volt_amd import train_utils
    x, vol, iters, (rv, rn) = trained_reference
    assert train_utils._auto_graph(None, dev(vol[0]), launch_bound=True) is True
    m, lh = train_utils.TrainVolModel(dev(x), dev(vol[0]), train_iters=iters, graph=graph, solver="linear")
    assert m.solver == "linear"
    assert abs(float(m.covar_module.raw_vol) - rv[0]) <= 2e-3 and abs(float(lh.raw_noise) - rn[0]) <= 2e-3
    mb, lb = train_utils.TrainVolModelBatch(dev(x), dev(vol), train_iters=iters, graph=graph, solver="linear")
    assert float((mb.covar_module.raw_vol.detach().cpu().double().reshape(-1) - torch.tensor(rv)).abs().max()) <= 2e-3
    assert float((lb.raw_noise.detach().cpu().double().reshape(-1) - torch.tensor(rn)).abs().max()) <= 2e-3


def test_trainers_reject_an_unknown_solver():
    from volt_amd import train_utils
    x = torch.arange(1, 33, device="cuda") / 252.0
    with pytest.raises(ValueError, match="solver must be one of"):
        train_utils.TrainVolModel(x, torch.full((32,), 0.2, device="cuda"), train_iters=0, solver="banded")
    with pytest.raises(ValueError, match="not"):
        train_utils.TrainVolModelBatch(x, torch.full((2, 32), 0.2, device="cuda"), train_iters=0, kernel="fbm", solver="linear")


def test_volt_magpie_with_the_linear_vol_solver():
    """A VoltMagpie built with vol_solver="linear": SamplePrediction runs, and with the same seed MeanPrediction agrees with
    the dense model's to the dense tolerance (2e-3 on log-prices, tests/test_gpu_api.py).  One test point, the step the
    rollouts take: VoltMagpie's EWMA mean has no multi-point form (models/VoltMagpie.py)."""
    from volt_amd.gp import GaussianLikelihood, _BrownianPrior
    from volt_amd.models import VoltMagpie, VoltronGP
    from volt_amd.synthetic import sde_series
    n, H = 90, 1
    F, vol = sde_series(n, 31)
    tx = torch.arange(n, device="cuda") / 252.
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    ty, vp = dev(F)[1:].log(), dev(vol)
    lin = VoltMagpie(tx, ty, GaussianLikelihood().cuda(), vp, k=20, vol_solver="linear")
    dense = VoltMagpie(tx, ty, GaussianLikelihood().cuda(), vp, k=20)
    assert lin.vol_model.solver == "linear" and dense.vol_model.solver == "dense"
    assert float(lin.VolMLL()) == pytest.approx(float(dense.VolMLL()), rel=2e-5)
    lin.vol_model.train()
    assert isinstance(lin.vol_model(tx).lazy_covariance_matrix, _BrownianPrior)
    torch.manual_seed(2)
    s, pv = lin.SamplePrediction(test_x, return_vol=True)
    assert torch.isfinite(s).all() and torch.isfinite(pv).all() and tuple(pv.shape) == (H,)
    torch.manual_seed(7)
    a = lin.MeanPrediction(test_x, n_sample=3)
    torch.manual_seed(7)
    b = dense.MeanPrediction(test_x, n_sample=3)
    assert a.shape == b.shape and float((a - b).abs().max()) < 2e-3
    with pytest.raises(ValueError, match="vol_solver"):
        VoltronGP(tx, ty, GaussianLikelihood().cuda(), vp, vol_solver="banded")


# ------------------------------------------------------------------------------------------------ no N^2 anywhere
def test_no_quadratic_memory_at_n_65536():
    """N = 65536, B = 2: the step and the posterior at H = 20 match the O(N) restatement and the peak of allocated device
    memory grows by less than 64 MB over the calls -- one dense fp32 matrix of this size would be 17 GB."""
    from volt_amd import ops
    n, B, H = 65536, 2, 20
    x, vol, s2, r, out, alpha = case(n, "uniform_dt", B=B, seed=9)
    xt, v, s, rt = dev(x), dev(vol), dev(s2), dev(r)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    o, a, info = ops.bm_step(xt, v, s, rt)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    assert grown < 64 * 2 ** 20, grown
    assert not info.any()
    check_step(o.cpu().numpy().astype(np.float64), a.cpu().numpy().astype(np.float64), out, alpha, n, torch.float32)
    del o, a, info
    m, lh = _bmgp(x, r, "linear")
    m.eval()
    xs = f32(x[-1] + (1 + np.arange(H)) / 252.0)
    xsd = dev(xs)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    post = m(xsd)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    assert grown < 64 * 2 ** 20, grown
    # the posterior from the restatement: alpha and A^-1 K_t*, then the two products in fp64
    vol64, noise64 = m.covar_module.vol.detach().double().cpu().numpy().reshape(-1), lh.noise.detach().double().cpu().numpy().reshape(-1)
    resid = f32((dev(r) - m.mean_module(dev(x))).detach().cpu().numpy())             # what the model hands the step
    _, al, _ = ref.bm_step_ref(x, vol64, noise64, resid)
    Kts = vol64[:, None, None] * np.minimum(x[None, :, None], xs[None, None, :])
    X, _ = ref.bm_solve_ref(x, vol64, noise64, Kts)
    wm = -0.5 * (vol64 ** 2)[:, None] * xs[None, :] + np.einsum("tnh,tn->th", Kts, al)
    wc = vol64[:, None, None] * np.minimum(xs[:, None], xs[None, :])[None] - np.einsum("tnh,tnk->thk", Kts, X)
    got_m, got_c = post.mean.double().cpu().numpy(), post.covariance_matrix.double().cpu().numpy()
    assert np.abs(got_m - wm).max() <= 8 * 2.0 ** -24 * np.abs(r).max()
    assert np.abs(got_c - wc).max() <= 8 * 2.0 ** -24 * (vol64.max() * xs.max())


def test_volt_train_keeps_the_linear_vol_solver():
    """Volt.Train refits the vol forecaster (Volt.py:103-104) and attaches the new model: built with vol_solver="linear" it is
    still linear afterwards -- its prior lazy, its posterior from the linear solve -- and Forecast runs on it."""
    import warnings
    from volt_amd.gp import _BrownianPrior
    from volt_amd.models.Volt import Volt
    from volt_amd.synthetic import sde_series
    n, H, S = 130, 6, 8
    F, vol = sde_series(n, 5)
    tx = torch.arange(n + 1, device="cuda") / 252.
    m = Volt(tx, dev(F).log(), mean="ewma", vol_path=dev(vol), k=10, vol_solver="linear")
    assert m.vol_solver == "linear" and m.vol_model.solver == "linear"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.Train(gpcv_iters=5, vol_mod_iters=5, data_mod_iters=4)          # GPCV -> vol model -> data model
    vm = m.vol_model
    assert vm.solver == "linear"
    vm.train()
    assert isinstance(vm(vm.train_inputs[0][:, 0]).lazy_covariance_matrix, _BrownianPrior)
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    out = m.Forecast(test_x, nsample=S)
    assert tuple(out.shape) == (S, H) and torch.isfinite(out).all()
    dense = Volt(tx, dev(F).log(), mean="ewma", vol_path=dev(vol), k=10)
    assert dense.vol_solver == "dense" and dense.vol_model.solver == "dense"
