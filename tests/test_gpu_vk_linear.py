"""The linear-time step of the volatility-kernel data model on the MI355X (volt_vk_step_*, csrc/bm.hip; ops.vk_step,
gp._VolPrior / _ChainMLL, VoltronGP / VoltMagpie / Volt(data_solver="linear"), the data-model trainers' solver="linear")
against the fp64 restatement of its recurrences (tests/vk_chain_ref.py, itself checked against the oracle and dense fp64
LAPACK in tests/test_vk_chain_host.py), against the dense path and against the fp64 oracle.

Tolerances of the raw step: those of tests/test_gpu_bm_linear.py (check_step there, restated here) -- the arithmetic is fp64
whatever the I/O type, so fp64 entry points: 1e-10 of the quantity's scale at N <= 1024, 1e-8 at N = 4096; fp32 entry points:
2^-23 |ref| (one rounding of the output) plus that fp64 term.  Every input is an fp32-representable number, so the fp32 and
fp64 runs and the reference see the same values."""
import functools
import warnings

import numpy as np
import pytest
import torch

import bm_chain_ref as bm
import vk_chain_ref as ref
from oracle import volt_oracle as vo
from volt_amd.synthetic import sde_batch, sde_series

pytestmark = pytest.mark.gpu

BMAX = 130
EPS32 = 2.0 ** -23


def f64_tol(n):
    return 1e-10 if n <= 1024 else 1e-8


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a)).to(dtype).cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(n, B=BMAX, seed=0):
    """B series with B DIFFERENT grids (vk_chain_ref.mixed_case) and the restatement's outputs.  Computed once, shared by the
    fp32 and fp64 tests and by every batch size (the series are independent: rows lo .. lo + B are the case of B series)."""
    V, s2, r = ref.mixed_case(B, n, seed)
    assert (np.diff(V, axis=1) >= 0).all() and (V[:, 0] >= 0).all()
    assert B < 2 or len({V[b].tobytes() for b in range(B)}) == B               # no two series share a grid
    out, alpha, info = ref.vk_step_ref(V, s2, r)
    assert not info.any()
    for a in (V, s2, r, out, alpha):
        a.setflags(write=False)
    return V, s2, r, out, alpha


def check_step(got_out, got_alpha, out, alpha, n, dtype):
    """tests/test_gpu_bm_linear.check_step; returns the largest error / bound over out and over alpha."""
    tol = f64_tol(n)
    scale = bm.out_scales(out, n)
    eps = EPS32 if dtype == torch.float32 else 0.0
    err = np.abs(got_out[:, :6] - out[:, :6])
    bound = eps * np.abs(out[:, :6]) + tol * scale
    assert (err <= bound).all(), (np.argwhere(err > bound)[:4], (err / bound).max())
    np.testing.assert_array_equal(got_out[:, 6:8], out[:, 6:8])                # sigma2 as used, and the scale 1
    aerr = np.abs(got_alpha - alpha)
    abound = eps * np.abs(alpha) + tol * np.abs(alpha).max(1, keepdims=True)
    assert (aerr <= abound).all(), (aerr / abound).max()
    return float((err / bound).max()), float((aerr / np.maximum(abound, 1e-300)).max())


# ------------------------------------------------------------------------------------------------ 1: ops.vk_step
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 129, 399])
def test_vk_step_matches_the_restatement(n, dtype):
    from volt_amd import ops
    V, s2, r, out, alpha = case(n)
    if n >= 64:
        assert ref.zero_increments(V[2::3]) > 0                                # the zero-increment family is really in the mix
    worst = (0.0, 0.0)
    for B, lo in ((1, 0), (1, 1), (1, 2), (3, 0), (3, 7), (64, 0), (65, 0), (65, 65), (130, 0)):
        sl = slice(lo, lo + B)
        o, a, info = ops.vk_step(dev(V[sl], dtype), dev(s2[sl], dtype), dev(r[sl], dtype))
        assert o.dtype == dtype and a.dtype == dtype and tuple(o.shape) == (B, 8) and tuple(a.shape) == (B, n) and not info.any()
        w = check_step(host(o), host(a), out[sl], alpha[sl], n, dtype)
        worst = max(worst[0], w[0]), max(worst[1], w[1])
    print(f"vk_step N = {n} {dtype}: largest error / bound  out {worst[0]:.3f}  alpha {worst[1]:.3f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_vk_step_two_long_series(dtype):
    from volt_amd import ops
    n = 4096
    V, s2, r, out, alpha = case(n, B=2, seed=3)
    o, a, info = ops.vk_step(dev(V, dtype), dev(s2, dtype), dev(r, dtype))
    assert not info.any()
    w = check_step(host(o), host(a), out, alpha, n, dtype)
    print(f"vk_step 2 x {n} {dtype}: largest error / bound  out {w[0]:.3f}  alpha {w[1]:.3f}")


def test_vk_step_validates_shapes():
    from volt_amd import ops
    V, s2, r = (torch.zeros(3, 8, device="cuda") for _ in range(3))
    with pytest.raises(ValueError, match="resid must be"):
        ops.vk_step(V, s2[:, 0], r[0])
    with pytest.raises(ValueError, match="V must be"):
        ops.vk_step(V[:, :7], s2[:, 0], r)
    with pytest.raises(ValueError, match="V must be"):
        ops.vk_step(V[None], s2[:, 0], r)
    with pytest.raises(ValueError, match="disagree on B"):
        ops.vk_step(V[:2], s2[:, 0], r)


# ------------------------------------------------------------------------------------------------ 2: memory safety, repeatability
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("B,n", [(1, 1), (3, 65), (65, 399), (130, 63)])
def test_vk_step_writes_nothing_past_its_buffers_and_repeats_bitwise(B, n, dtype):
    """NaN sentinels behind out and alpha, -77 behind info, 0xFF bytes on both sides of the workspace survive; V is a strided
    view (bsv = N + 37) inside a NaN-filled buffer, so a read outside a series' row shows; ten runs agree bit for bit."""
    from volt_amd import _lib, ops
    V, s2, r, out, alpha = case(n)
    ws = ops.BmWorkspace(B, n, "cuda", dtype)
    nbytes = int(_lib.lib().volt_bm_workspace_bytes(B, n, 1))
    ws.buf.fill_(0xFF)
    guard = 64
    obuf = torch.full((B * 8 + guard,), float("nan"), dtype=dtype, device="cuda")
    abuf = torch.full((B * n + guard,), float("nan"), dtype=dtype, device="cuda")
    ibuf = torch.full((B + guard,), -77, dtype=torch.int32, device="cuda")
    ws.out, ws.alpha, ws.info = obuf[:B * 8].view(B, 8), abuf[:B * n].view(B, n), ibuf[:B]
    bsv = n + 37
    vbuf = torch.full((guard + B * bsv,), float("nan"), dtype=dtype, device="cuda")
    Vv = vbuf[guard:].view(B, bsv)[:, :n]
    Vv.copy_(dev(V[:B], dtype))
    assert Vv.stride(0) == bsv and (B == 1 or not Vv.is_contiguous())
    args = (Vv, dev(s2[:B], dtype), dev(r[:B], dtype), ws)
    o, a, info = ops.vk_step(*args)
    assert o.data_ptr() == obuf.data_ptr() and a.data_ptr() == abuf.data_ptr()
    first = (o.clone(), a.clone(), info.clone())
    check_step(host(o), host(a), out[:B], alpha[:B], n, dtype)
    for _ in range(9):
        obuf[:B * 8].fill_(float("nan"))
        abuf[:B * n].fill_(float("nan"))
        o, a, info = ops.vk_step(*args)
        assert torch.equal(o, first[0]) and torch.equal(a, first[1]) and torch.equal(info, first[2])
    assert torch.isnan(obuf[B * 8:]).all() and torch.isnan(abuf[B * n:]).all() and bool((ibuf[B:] == -77).all())
    off = ws.ptr - ws.buf.data_ptr()
    assert bool((ws.buf[off + nbytes:] == 0xFF).all()) and bool((ws.buf[:off] == 0xFF).all())
    # without VOLT_WANT_GRAD: the forward scalars only
    obuf.fill_(float("nan"))
    abuf.fill_(float("nan"))
    o, a, info = ops.vk_step(*args, want_grad=False)
    assert torch.equal(o[:, [0, 2, 3, 6, 7]], first[0][:, [0, 2, 3, 6, 7]]) and torch.isnan(o[:, [1, 4, 5]]).all()
    assert torch.isnan(abuf).all() and not info.any()


# ------------------------------------------------------------------------------------------------ 3: one shared grid
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("B,n", [(1, 1), (3, 65), (65, 399), (130, 63)])
def test_vk_step_with_a_shared_grid_equals_bm_step(B, n, dtype):
    """bsv = 0: the Brownian-motion step on x = V with vol = 1.  The two kernels are instantiations of one template and share
    the chain, the sums and the backward sweep; delta is the same fp64 difference of the same two stored values: bitwise."""
    from volt_amd import ops
    V, s2, r, _, _ = case(n)
    x = dev(V[1] if n > 1 else V[0], dtype)
    if n > 1:
        x = torch.unique_consecutive(x)                                        # (bm_step's documented grid is strictly increasing)
    m = x.numel()
    s, rr = dev(s2[:B], dtype), dev(r[:B, :m], dtype)
    ob, ab, ib = (t.clone() for t in ops.bm_step(x, torch.ones(B, device="cuda", dtype=dtype), s, rr))
    ov, av, iv = ops.vk_step(x, s, rr)
    assert torch.equal(ov, ob) and torch.equal(av, ab) and torch.equal(iv, ib)
    want = ref.vk_step_ref(host(x), host(s), host(rr))
    check_step(host(ov), host(av), want[0], want[1], m, dtype)


# ------------------------------------------------------------------------------------------------ 4: info
def test_vk_step_info():
    from volt_amd import ops
    n = 70
    V, s2, r, out, alpha = case(n)
    rr = r[:3].copy()
    rr[1, 40] = np.nan                                            # a NaN residual is not a pivot failure: info 0, NaN out
    o, a, info = ops.vk_step(dev(V[:3]), dev(s2[:3]), dev(rr))
    assert info.tolist() == [0, 0, 0]
    assert torch.isnan(o[1, 0]) and torch.isnan(o[1, 2]) and torch.isfinite(o[1, 3]) and torch.isnan(a[1]).any()
    assert torch.isfinite(o[[0, 2]]).all() and torch.isfinite(a[[0, 2]]).all()
    V0, s0 = V[:3].copy(), s2[:3].copy()
    V0[:, 0] = 0.0
    s0[2] = 0.0                                                   # s = 0 at V_0 = 0: d_0 = 0
    o, a, info = ops.vk_step(dev(V0), dev(s0), dev(r[:3]))
    assert info.tolist() == [0, 0, 1] and torch.isnan(o[2, 0]) and torch.isnan(o[2, 3]) and torch.isfinite(o[:2]).all()
    Vn = V[:3].copy()
    Vn[1, 33] = np.nan                                            # a NaN in ONE series' grid
    o, a, info = ops.vk_step(dev(Vn), dev(s2[:3]), dev(r[:3]))
    assert info[0] == 0 and info[2] == 0 and info[1] != 0
    assert torch.isfinite(o[[0, 2]]).all() and torch.isfinite(a[[0, 2]]).all()
    check_step(host(o[[0, 2]]), host(a[[0, 2]]), out[[0, 2]], alpha[[0, 2]], n, torch.float32)
    sn = s2[:3].copy()
    sn[0] = np.nan
    _, _, info = ops.vk_step(dev(V[:3]), dev(sn), dev(r[:3]))
    assert info.tolist() == [1, 0, 0]


# ------------------------------------------------------------------------------------------------ 5: against the dense step
@pytest.mark.parametrize("B,n", [(1, 399), (8, 399), (2, 1024)])
def test_linear_step_is_at_least_as_accurate_as_the_dense_fp32_step(B, n):
    """Side by side on the same fp32 V and residual at sigma2 = 0.69: the linear step's error against the dense fp64 step on the
    same K is at most the dense fp32 step's own, quantity by quantity, margin 1 -- its arithmetic is fp64, so a larger error
    is a bug, not noise."""
    from volt_amd import ops
    V, _, r, _, _ = case(n, B=8, seed=5)
    Vt, s, rt = dev(V[:B]), dev(np.full(B, ref.NOISES[2])), dev(r[:B])
    K = ops.fill(Vt)
    o64, a64, i64 = (t.clone() for t in ops.mll_step(K.double(), rt.double(), s.double()))
    o32, a32, i32 = (t.clone() for t in ops.mll_step(K, rt, s))
    ol, al, il = ops.vk_step(Vt, s, rt)
    assert not i64.any() and not i32.any() and not il.any()
    names = ("mll", "dmll/dsigma2", "quad", "logdet", "tr", "alpha'alpha")
    bad = []
    for k, name in enumerate(names):
        e_lin = float((ol[:, k].double() - o64[:, k]).abs().max())
        e_dense = float((o32[:, k].double() - o64[:, k]).abs().max())
        print(f"{B} x {n} {name:13s}: linear {e_lin:.3e}  dense fp32 {e_dense:.3e}  (|ref| {float(o64[:, k].abs().max()):.3e})")
        if not e_lin <= e_dense:
            bad.append((name, e_lin, e_dense))
    e_lin, e_dense = float((al.double() - a64).abs().max()), float((a32.double() - a64).abs().max())
    print(f"{B} x {n} alpha        : linear {e_lin:.3e}  dense fp32 {e_dense:.3e}  (|ref| {float(a64.abs().max()):.3e})")
    assert not bad, bad
    assert e_lin <= e_dense


# ------------------------------------------------------------------------------------------------ 6: models
def _model(cls, tx, y, vol, solver, mean, k=10):
    from volt_amd.gp import GaussianLikelihood
    from volt_amd.train_utils import _set_mean, _train_noise_and_mean
    bs = torch.Size(y.shape[:-1])
    lh = GaussianLikelihood(batch_shape=bs).cuda()
    kw = {"k": k} if cls.__name__ == "VoltMagpie" else {}
    m = cls(tx, y, lh, vol, data_solver=solver, **kw).cuda()
    _set_mean(m, mean, tx, y, k, 0.5, bs)
    _train_noise_and_mean(m, lh)
    T = bs[0] if len(bs) else 1
    with torch.no_grad():
        lh.raw_noise.copy_(torch.linspace(-1.0, 0.5, T).reshape(lh.raw_noise.shape))
        if mean == "constant":
            m.mean_module.constant.copy_(torch.linspace(2.0, 2.4, T).reshape(m.mean_module.constant.shape))
        elif mean == "loglinear":
            m.mean_module.weights.copy_(torch.linspace(-0.4, 0.6, T).reshape(m.mean_module.weights.shape))
    return m, lh


def _mll_and_grads(m, lh, tx, y):
    from volt_amd.gp import ExactMarginalLogLikelihood
    m.train()
    params = [lh.raw_noise] + list(m.mean_module.parameters())
    for p in params:
        p.grad = None
    val = ExactMarginalLogLikelihood(lh, m)(m(tx), y)
    val.sum().backward()
    return [val.detach().double().cpu().reshape(-1)] + [p.grad.detach().double().cpu().reshape(val.numel(), -1) for p in params]


def _oracle_mll_and_grads(m, lh, x, y, vol, mean):
    """fp64: the oracle's mll, d/d raw_noise and d/d mean, chained by hand through the constant / log-linear mean."""
    T, n = y.shape
    K = vo.volatility_kernel(np.repeat(x[None], T, 0)[..., None], vol[..., None])
    raw = host(lh.raw_noise).reshape(-1)
    if mean == "constant":
        c = host(m.mean_module.constant).reshape(T, 1)
        mu, jac = np.broadcast_to(c, (T, n)), [np.ones((T, n))]
    else:
        w, b = host(m.mean_module.weights).reshape(T, 1), host(m.mean_module.bias).reshape(T, 1)
        lin = w * x[None].astype(np.float64) + b
        assert lin.min() > 1.0                                                 # (the clamp at 1e-6 is not active)
        mu, jac = np.log(lin), [x[None] / lin, 1.0 / lin]
    o = vo.mll_and_grads(K, y, mu, raw)
    return [o["mll"], o["d_raw"].reshape(T, 1)] + [(o["d_mean"] * j).sum(1).reshape(T, 1) for j in jac]


@pytest.mark.parametrize("cls_name,mean", [("VoltMagpie", "constant"), ("VoltMagpie", "loglinear"), ("VoltronGP", "constant"),
                                           ("VoltronGP", "loglinear")])
def test_linear_data_model_mll_and_gradients(cls_name, mean):
    """MLL 2e-5 (relative), gradients 1e-3 of the largest entry: the dense path's stated bounds (README; tests/test_gpu_api.py),
    against the fp64 oracle on the reference's K.  Against the dense model on the same inputs: both sit within those bounds
    of the oracle, so within twice them of each other.  Batched = per-series: the value bitwise, gradients to 1e-6."""
    from volt_amd import models
    from volt_amd.gp import _VolPrior, _dense
    cls = getattr(models, cls_name)
    T, n = 3, 130
    x, F, vol = sde_batch(T, n, seed=40)
    tx, y, vp = dev(x), dev(F[:, 1:]).log(), dev(vol)
    lin, llh = _model(cls, tx, y, vp, "linear", mean)
    den, dlh = _model(cls, tx, y, vp, "dense", mean)
    assert lin.data_solver == "linear" and den.data_solver == "dense"
    assert isinstance(lin.train_cov, _VolPrior) and torch.is_tensor(den.train_cov)
    lin.train()
    assert lin(tx).lazy_covariance_matrix is lin.train_cov
    got, dgot = _mll_and_grads(lin, llh, tx, y), _mll_and_grads(den, dlh, tx, y)
    want = _oracle_mll_and_grads(lin, llh, x, host(y), vol, mean)
    for i, (g, d, w) in enumerate(zip(got, dgot, want)):
        g, d, w = g.numpy().reshape(w.shape), d.numpy().reshape(w.shape), np.asarray(w)
        tol = 2e-5 * np.abs(w) if i == 0 else 1e-3 * np.abs(w).max()
        print(f"{cls_name} {mean} quantity {i}: linear-oracle {np.abs(g - w).max():.3e}  dense-oracle {np.abs(d - w).max():.3e}  "
              f"bound {np.max(tol):.3e}")
        assert (np.abs(g - w) <= tol).all(), (i, g, w)
        assert (np.abs(g - d) <= 2 * tol).all(), (i, g, d)
    for t in range(T):
        m1, l1 = _model(cls, tx, y[t], vp[t], "linear", mean)
        with torch.no_grad():
            for p1, pb in zip([l1.raw_noise] + list(m1.mean_module.parameters()), [llh.raw_noise] + list(lin.mean_module.parameters())):
                p1.copy_(pb[t].reshape(p1.shape))
        one = _mll_and_grads(m1, l1, tx, y[t])
        assert float(one[0]) == float(got[0][t])
        for g1, gb in zip(one[1:], got[1:]):
            assert float((g1.reshape(-1) - gb[t].reshape(-1)).abs().max()) <= 1e-6 * float(g1.abs().max())
    # UpdateVolPath: the lazy prior is rebuilt, and the result moves as the dense model's does
    vp2 = vp * torch.linspace(0.7, 1.6, n, device="cuda")
    lin.UpdateVolPath(vp2)
    den.UpdateVolPath(vp2)
    assert isinstance(lin.train_cov, _VolPrior) and torch.equal(lin.train_cov.evaluate(), _dense(den.train_cov))
    got2, dgot2 = _mll_and_grads(lin, llh, tx, y), _mll_and_grads(den, dlh, tx, y)
    want2 = _oracle_mll_and_grads(lin, llh, x, host(y), host(vp2).astype(np.float32), mean)
    assert float((got2[0] - got[0]).abs().min()) > 1e-4                 # the result moved
    for i, (g, d, w) in enumerate(zip(got2, dgot2, want2)):
        g, d, w = g.numpy().reshape(w.shape), d.numpy().reshape(w.shape), np.asarray(w)
        tol = 2e-5 * np.abs(w) if i == 0 else 1e-3 * np.abs(w).max()
        assert (np.abs(g - w) <= tol).all() and (np.abs(g - d) <= 2 * tol).all(), (i, g, d, w)


def test_linear_data_model_saves_one_packed_tensor_and_defers_checks():
    from volt_amd import gp
    from volt_amd.models import VoltMagpie
    n = 64
    F, vol = sde_series(n, 3)
    tx, y = torch.arange(n, device="cuda") / 252., dev(F)[1:].log()
    m, lh = _model(VoltMagpie, tx, y, dev(vol), "linear", "constant")
    m.train()
    mll = gp.ExactMarginalLogLikelihood(lh, m)
    val = mll(m(tx), y)
    fn = val.grad_fn
    while fn is not None and "ChainMLL" not in type(fn).__name__:
        fn = fn.next_functions[0][0] if fn.next_functions else None
    assert fn is not None and len(fn.saved_tensors) == 1 and tuple(fn.saved_tensors[0].shape) == (1, 8 + n)
    # a forward for any other x fills densely, as before
    other = m(tx + 1.0 / 252).lazy_covariance_matrix
    assert not isinstance(other, gp._VolPrior) and tuple(other.shape) == (n, n)
    with torch.no_grad():
        lh.noise_covar.raw_noise.fill_(float("nan"))
    with pytest.raises(gp.NanError):                                          # NanError before NotPSDError
        mll(m(tx), y)
    with gp.deferred_checks(immediate=True) as chk:
        with pytest.raises(gp.NanError):
            mll(m(tx), y)
        chk.immediate = False
        mll(m(tx), y)
        assert chk.any_bad() == 1
        with pytest.raises(gp.NotPSDError):
            chk.raise_if_bad()


def test_predictions_and_rollouts_on_a_linear_model_equal_the_dense_models():
    """GeneratePrediction (the model method and the rollout_utils function) and Rollouts build what they need from
    log_vol_path and never read train_cov: identical draws give identical samples."""
    from volt_amd.models import VoltMagpie, VoltronGP
    from volt_amd.rollout_utils import Rollouts
    n, H, S = 90, 6, 5
    F, vol = sde_series(n, 31)
    tx = torch.arange(n, device="cuda") / 252.
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    prices, y, vp = dev(F), dev(F)[1:].log(), dev(vol)
    pv = dev(np.full(H, vol[-1], dtype=np.float32))
    outs = {}
    for solver in ("linear", "dense"):
        m, _ = _model(VoltronGP, tx, y, vp, solver, "loglinear")
        torch.manual_seed(11)
        outs[solver, "gp"] = m.GeneratePrediction(test_x, pv, 3)
        g = torch.Generator().manual_seed(5)
        pred_vol = (vp[-1].log() + 0.05 * torch.randn(S, H, generator=g).cumsum(-1).cuda()).exp()
        z = torch.randn(S, H, generator=g).cuda()
        for engine in ("bordered", "dense"):
            mm2, _ = _model(VoltMagpie, tx, y, vp, solver, "ewma", k=20)
            outs[solver, engine] = Rollouts(tx, prices, test_x, mm2, nsample=S, pred_vol=pred_vol, z=z, engine=engine)
    for key in ("gp", "bordered", "dense"):
        a, b = outs["linear", key], outs["dense", key]
        assert torch.isfinite(a).all() and a.shape == b.shape
        assert torch.equal(a, b), (key, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------ 7: trainers
def _adam(params, grads_fn, iters, lr):
    """fp64 torch.optim.Adam on the loss whose (value, gradients) grads_fn(params as floats) returns; the last loss too."""
    ps = [torch.tensor(float(p), dtype=torch.float64, requires_grad=True) for p in params]
    opt = torch.optim.Adam(ps, lr=lr)
    loss = None
    for _ in range(iters):
        opt.zero_grad()
        loss, grads = grads_fn([float(p) for p in ps])
        for p, g in zip(ps, grads):
            p.grad = torch.tensor(float(g), dtype=torch.float64)
        opt.step()
    return [float(p) for p in ps], loss


def _noise_only(V, resid, n):
    def fn(p):
        s = float(vo.noise_from_raw(p[0]))
        out, _, _ = ref.vk_step_ref(V, [s], resid[None])
        return -out[0, 0], [-out[0, 1] / (1.0 + np.exp(-p[0]))]
    return fn


def _noise_and_loglinear(V, x, y, n):
    def fn(p):
        raw, w, b = p
        s = float(vo.noise_from_raw(raw))
        lin = w * x + b
        out, alpha, _ = ref.vk_step_ref(V, [s], (y - np.log(lin))[None])
        return -out[0, 0], [-out[0, 1] / (1.0 + np.exp(-raw)), -(alpha[0] / n * x / lin).sum(), -(alpha[0] / n / lin).sum()]
    return fn


ITERS, KTAPS, SEED = 40, 20, 5


@pytest.fixture(scope="module")
def trained_reference():
    """1 x 399 and 3 x 130: the data, the fp32 V the device integrates (the numbers the dense fill would copy into K) and fp64
    Adam on the restatement for the EWMA-mean model (the noise trains) and the log-linear one (noise, slope, intercept)."""
    from volt_amd import ops
    from volt_amd.train_utils import LR_DATA, TrainDataModel
    n = 399
    F, vol = sde_series(n, 21)
    x = (np.arange(n) / 252.).astype(np.float32)
    y = np.log(F[1:]).astype(np.float32)
    V = host(ops.cumtrapz(dev(vol), dev(x), square=True))
    ew = vo.ewma_mean(x, x, y, KTAPS).astype(np.float64)
    magpie = _adam([1e-5], _noise_only(V, y.astype(np.float64) - ew, n), ITERS, LR_DATA)
    torch.manual_seed(SEED)                                                    # the log-linear mean's slope starts at a random draw
    m0, _ = TrainDataModel(dev(x), dev(F)[1:], None, None, dev(vol), train_iters=0, solver="linear")
    w0, b0 = float(m0.mean_module.weights), float(m0.mean_module.bias)
    data = _adam([1e-5, w0, b0], _noise_and_loglinear(V, x.astype(np.float64), y.astype(np.float64), n), ITERS, LR_DATA)
    B, nb = 3, 130
    xb, Fb, volb = sde_batch(B, nb, seed=21)
    yb = np.log(Fb[:, 1:]).astype(np.float32)
    Vb = host(ops.cumtrapz(dev(volb), dev(xb), square=True))
    batch = [_adam([1e-5], _noise_only(Vb[b], yb[b].astype(np.float64) - vo.ewma_mean(xb, xb, yb[b], KTAPS), nb), ITERS, LR_DATA)
             for b in range(B)]
    return dict(x=x, F=F, vol=vol, magpie=magpie, data=data, w0=w0, xb=xb, Fb=Fb, volb=volb, batch=batch)


def _last_loss(model, lh, tx, y):
    from volt_amd.gp import ExactMarginalLogLikelihood
    with torch.no_grad():
        model.train()
        return -ExactMarginalLogLikelihood(lh, model)(model(tx), y).double().cpu().reshape(-1)


@pytest.mark.parametrize("graph", [False, True, None], ids=["eager", "captured", "auto"])
def test_data_model_trainers_linear_match_fp64_adam(trained_reference, graph):
    """40 Adam iterations, eager, captured and graph=None (which captures: the step is launch-bound at every N), against fp64
    Adam on the restatement: 2e-3 on the parameters and on the loss, the bound of the Brownian-motion trainer's test."""
    from volt_amd import train_utils
    from volt_amd.gp import _VolPrior
    R = trained_reference
    tx, prices, vp = dev(R["x"]), dev(R["F"]), dev(R["vol"])
    assert train_utils._auto_graph(None, prices[1:].log(), launch_bound=True) is True
    # VoltMagpie, EWMA mean: the noise trains
    (raw_ref,), _ = R["magpie"]
    m, lh = train_utils.TrainVoltMagpieModel(tx, prices[1:], None, None, vp, train_iters=ITERS, k=KTAPS, graph=graph, solver="linear")
    assert m.data_solver == "linear" and isinstance(m.train_cov, _VolPrior)
    print(f"TrainVoltMagpieModel graph={graph}: raw_noise {float(lh.raw_noise):.6f}  fp64 Adam {raw_ref:.6f}")
    assert abs(float(lh.raw_noise) - raw_ref) <= 2e-3
    want = _noise_only(host(m.train_cov.x), host(prices[1:].log() - m.mean_module(tx)), 399)([float(lh.raw_noise)])[0]
    assert abs(float(_last_loss(m, lh, tx, prices[1:].log())) - want) <= 2e-3 * max(1.0, abs(want))
    # VoltronGP, log-linear mean: noise, slope and intercept train
    (raw_ref, w_ref, b_ref), _ = R["data"]
    torch.manual_seed(SEED)
    m, lh = train_utils.TrainDataModel(tx, prices[1:], None, None, vp, train_iters=ITERS, graph=graph, solver="linear")
    assert m.data_solver == "linear" and isinstance(m.train_cov, _VolPrior)
    got = (float(lh.raw_noise), float(m.mean_module.weights), float(m.mean_module.bias))
    print(f"TrainDataModel graph={graph}: (raw_noise, slope, intercept) {got}  fp64 Adam {(raw_ref, w_ref, b_ref)}  start slope {R['w0']:.4f}")
    assert max(abs(g - w) for g, w in zip(got, (raw_ref, w_ref, b_ref))) <= 2e-3
    y64 = np.log(R["F"][1:]).astype(np.float32).astype(np.float64)
    want = _noise_and_loglinear(host(m.train_cov.x), R["x"].astype(np.float64), y64, 399)(list(got))[0]
    assert abs(float(_last_loss(m, lh, tx, prices[1:].log())) - want) <= 2e-3 * max(1.0, abs(want))


@pytest.mark.parametrize("graph", [False, None], ids=["eager", "auto"])
def test_train_volt_magpie_batch_linear(trained_reference, graph):
    from volt_amd import train_utils
    from volt_amd.gp import _VolPrior
    R = trained_reference
    tx, prices, vp = dev(R["xb"]), dev(R["Fb"]), dev(R["volb"])
    m, lh, losses = train_utils.TrainVoltMagpieBatch(tx, prices[:, 1:], vp, train_iters=ITERS, k=KTAPS, graph=graph, solver="linear")
    assert m.data_solver == "linear" and isinstance(m.train_cov, _VolPrior) and tuple(m.train_cov.shape) == (3, 130, 130)
    raw = host(lh.raw_noise).reshape(-1)
    for b, ((raw_ref,), loss_ref) in enumerate(R["batch"]):
        print(f"TrainVoltMagpieBatch graph={graph} series {b}: raw_noise {raw[b]:.6f}  fp64 Adam {raw_ref:.6f}")
        assert abs(raw[b] - raw_ref) <= 2e-3
        assert abs(float(losses[b]) - loss_ref) <= 2e-3 * max(1.0, abs(loss_ref))     # the loss of the last iteration's forward


def test_volt_train_keeps_the_linear_data_solver():
    from volt_amd.gp import _VolPrior
    from volt_amd.models.Volt import Volt
    n, H, S = 130, 6, 8
    F, vol = sde_series(n, 5)
    tx = torch.arange(n + 1, device="cuda") / 252.
    m = Volt(tx, dev(F).log(), mean="ewma", vol_path=dev(vol), k=10, data_solver="linear")
    assert m.data_solver == "linear" and isinstance(m.train_cov, _VolPrior)
    V0 = m.train_cov.x.clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.Train(gpcv_iters=5, vol_mod_iters=5, data_mod_iters=4)          # GPCV -> vol model -> data model
    assert m.data_solver == "linear" and isinstance(m.train_cov, _VolPrior)
    assert tuple(m.train_cov.x.shape) == (n,) and not torch.equal(m.train_cov.x, V0)      # rebuilt from the fitted vol path
    m.train()
    assert m(m.train_inputs[0][:, 0]).lazy_covariance_matrix is m.train_cov
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    out = m.Forecast(test_x, nsample=S)
    assert tuple(out.shape) == (S, H) and torch.isfinite(out).all()
    assert Volt(tx, dev(F).log(), mean="ewma", vol_path=dev(vol), k=10).data_solver == "dense"


def test_stocks_driver_with_the_linear_data_solver_writes_the_reference_layout(tmp_path):
    from volt_amd.forecast import GenerateStockPredictionsBatch
    from volt_amd.gp import _VolPrior
    B, T, ntrain, H, S = 3, 70, 64, 4, 5
    x, F, vol = sde_batch(B, T - 1, seed=77)
    closes = dev(F)
    g = torch.Generator(device="cuda").manual_seed(1)
    debug = {}
    out = GenerateStockPredictionsBatch(["AAA", "BBB", "CCC"], closes, forecast_horizon=H, train_iters=3, nsample=S,
                                        ntrain=ntrain, mean="ewma", save=True, k=10, ntimes=2, vol_iters=2,
                                        par_dir=str(tmp_path), generator=g, debug=debug, data_solver="linear")
    assert tuple(out.shape) == (B, S, H) and torch.isfinite(out).all()
    assert debug["model"].data_solver == "linear" and isinstance(debug["model"].train_cov, _VolPrior)
    files = sorted(p.name for p in (tmp_path / "BBB").iterdir())
    assert len(files) == 2 and all(f.startswith("volt_ewma10_") and f.endswith(".pt") for f in files)
    saved = torch.load(tmp_path / "CCC" / files[-1])
    assert tuple(saved.shape) == (S, H) and torch.equal(saved, out[2])


# ------------------------------------------------------------------------------------------------ 8: no N^2 anywhere
@pytest.mark.parametrize("dtype,n", [(torch.float32, 40961), (torch.float32, 65536), (torch.float64, 20481)], ids=["f32", "f32-65536", "f64"])
def test_cumtrapz_beyond_one_lds_pass_is_bit_exact(dtype, n):
    """A series longer than the one-pass kernel holds in LDS (160 KB) goes through the chunked kernel: the same products, the
    same running fp64 sum, every prefix rounded once -- bit for bit the oracle's (and the reference's CPU) result."""
    from volt_amd import ops
    npdt = np.float32 if dtype == torch.float32 else np.float64
    rng = np.random.default_rng(n)
    vol = rng.uniform(0.05, 0.9, (2, n)).astype(npdt)
    x = (np.arange(n) / 252.).astype(npdt)
    got = ops.cumtrapz(dev(vol, dtype), dev(x, dtype), square=True)
    want = vo.cumtrapz(vol * vol, x)
    assert got.dtype == dtype and np.array_equal(got.cpu().numpy(), want)


def test_no_quadratic_memory_at_n_65536():
    """2 x 65536: construction, step and backward match the O(N) restatement and the peak of allocated device memory grows by
    less than 64 MB -- one dense fp32 matrix of this size would be 17 GB."""
    from volt_amd.gp import ExactMarginalLogLikelihood, GaussianLikelihood, _VolPrior
    from volt_amd.models import VoltMagpie
    n, B = 65536, 2
    rng = np.random.default_rng(9)
    vol = ref.f32(np.stack([ref.vol_path("smooth", n, rng, 0.2), ref.vol_path("lognormal", n, rng, 0.6)]))
    y = ref.resid(B, n, rng)
    tx, yt, vp = torch.arange(n, device="cuda") / 252., dev(y), dev(vol)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    lh = GaussianLikelihood(batch_shape=torch.Size([B])).cuda()
    m = VoltMagpie(tx, yt, lh, vp, k=25, vol_solver="linear", data_solver="linear").cuda()
    assert isinstance(m.train_cov, _VolPrior) and tuple(m.train_cov.shape) == (B, n, n)
    m.train()
    with torch.no_grad():
        lh.raw_noise.copy_(torch.tensor([[0.0], [-3.0]]))
    val = ExactMarginalLogLikelihood(lh, m)(m(tx), yt)
    val.sum().backward()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    assert grown < 64 * 2 ** 20, grown
    resid = host(yt - m.mean_module(tx))
    s = host(lh.noise).reshape(-1)
    out, _, info = ref.vk_step_ref(host(m.train_cov.x), s, resid)
    assert not info.any()
    got, graw = host(val), host(lh.raw_noise.grad).reshape(-1)
    want_g = out[:, 1] / (1.0 + np.exp(-host(lh.raw_noise).reshape(-1)))
    scale = bm.out_scales(out, n)
    assert (np.abs(got - out[:, 0]) <= EPS32 * np.abs(out[:, 0]) + 1e-8 * scale[:, 0]).all(), (got, out[:, 0])
    assert (np.abs(graw - want_g) <= 4 * EPS32 * np.abs(want_g) + 1e-8 * scale[:, 1]).all(), (graw, want_g)
