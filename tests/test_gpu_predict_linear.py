"""Forecasting from the volatility-kernel data model in linear time on the MI355X (predict_solver="linear"):
volt_vk_forms_* (csrc/bm.hip) and ops.vk_forms against the fp64 restatement of the two-chain sweep, gp._safe_forms' ladder,
rollout_utils._posterior_draw_linear beside _posterior_draw against the fp64 oracle, train_block_terms / rollout_series
(solve="chain"), the models and drivers with predict_solver="linear" against the dense ones on identical draws, and the peak
memory at N = 65536.  The restatements (tests/vk_forms_ref.py) are checked against dense fp64 LAPACK and the oracle in
tests/test_vk_forms_host.py, where the negative controls for these bounds also live.

Bounds of the raw entry: the VK step's (tests/test_gpu_vk_linear.py) -- the arithmetic is fp64 whatever the I/O type, so 1e-10 of
each quantity's scale at N <= 1024 and 1e-8 at N = 4096.  The outputs of BOTH entries are doubles, so the fp32 entry gets no
2^-23 |ref| term: only its inputs' rounding, which is zero here (every input is an fp32-representable number)."""
import functools
import warnings

import numpy as np
import pytest
import torch

import vk_chain_ref as vk
import vk_forms_ref as ref
from volt_amd.synthetic import rollout_inputs, sde_batch, sde_series

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
    """B series on B different grids (vk_chain_ref.mixed_case), the jitter of a series its noise level, and the restatement's
    forms.  Computed once; rows lo .. lo + B are the case of B series."""
    V, s2, r = vk.mixed_case(B, n, seed)
    out, info = ref.forms_ref(V, s2, r)
    assert not info.any()
    for a in (V, s2, r, out):
        a.setflags(write=False)
    return V, s2, r, out


def check_forms(got, want, V, r, n):
    """|got - want| <= f64_tol(n) * scale per quantity; returns the largest error / bound."""
    bound = f64_tol(n) * ref.forms_scales(V, r, want)
    err = np.abs(got - want)
    assert (err <= bound).all(), (np.argwhere(err > bound)[:4], (err / bound).max())
    return float((err / bound).max())


# ------------------------------------------------------------------------------------------------ 1: ops.vk_forms
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 63, 64, 65, 129, 399])
def test_vk_forms_matches_the_restatement(n, dtype):
    from volt_amd import ops
    V, s2, r, want = case(n)
    worst = 0.0
    for B, lo in ((1, 0), (1, 2), (3, 0), (3, 7), (64, 0), (65, 0), (65, 65), (130, 0)):
        sl = slice(lo, lo + B)
        out, info = ops.vk_forms(dev(V[sl], dtype), dev(s2[sl], torch.float64), dev(r[sl], dtype))
        assert out.dtype == torch.float64 and tuple(out.shape) == (B, 4) and info.dtype == torch.int32 and not info.any()
        worst = max(worst, check_forms(host(out), want[sl], V[sl], r[sl], n))
    # one grid for all series (bsv = 0), and one jitter for all
    shared, _ = ref.forms_ref(V[1], s2[1], r[:65])
    out, info = ops.vk_forms(dev(V[1], dtype), float(s2[1]), dev(r[:65], dtype))
    assert not info.any()
    worst = max(worst, check_forms(host(out), shared, np.broadcast_to(V[1], (65, n)), r[:65], n))
    print(f"vk_forms N = {n} {dtype}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_vk_forms_two_long_series(dtype):
    from volt_amd import ops
    n = 4096
    V, s2, r, want = case(n, B=2, seed=3)
    out, info = ops.vk_forms(dev(V, dtype), dev(s2, torch.float64), dev(r, dtype))
    assert not info.any()
    print(f"vk_forms 2 x {n} {dtype}: largest error / bound {check_forms(host(out), want, V, r, n):.3f}")


@pytest.mark.parametrize("n", [1, 33, 399])
def test_vk_forms_at_zero_jitter_is_the_closed_form(n):
    """jitter = 0 is legal: rho = V[N-1] and tau = r[N-1] to the bound, and the restatement at j = 0 likewise."""
    from volt_amd import ops
    V, _, r, _ = case(n)
    keep = [b for b in range(12) if (np.diff(V[b], prepend=0.0) > 0).all()]   # (the flat family has zero increments: j = 0 fails there)
    assert len(keep) >= 6
    V, r = V[keep], r[keep]
    want, winfo = ref.forms_ref(V, 0.0, r)
    for dtype in (torch.float32, torch.float64):
        out, info = ops.vk_forms(dev(V, dtype), 0.0, dev(r, dtype))
        assert not info.any() and not winfo.any()
        check_forms(host(out), want, V, r, n)
        assert (np.abs(host(out)[:, 0] - V[:, -1]) <= f64_tol(n) * V[:, -1]).all()
        assert (np.abs(host(out)[:, 1] - r[:, -1]) <= f64_tol(n) * np.abs(r).max(1)).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("B,n", [(1, 1), (3, 65), (65, 399), (130, 63)])
def test_vk_forms_writes_nothing_past_its_buffers_and_repeats_bitwise(B, n, dtype):
    """Through the C entry: NaN sentinels behind out, -77 behind info; V is a strided view (bsv = N + 37) inside a NaN-filled
    buffer, so a read outside a series' row shows; ten runs agree bit for bit.  ops.vk_forms on the same strided view gives the
    same bits (it passes the stride on instead of copying)."""
    from volt_amd import _lib, ops
    V, s2, r, want = case(n)
    guard = 64
    obuf = torch.full((B * 4 + guard,), float("nan"), dtype=torch.float64, device="cuda")
    ibuf = torch.full((B + guard,), -77, dtype=torch.int32, device="cuda")
    bsv = n + 37
    vbuf = torch.full((guard + B * bsv,), float("nan"), dtype=dtype, device="cuda")
    Vv = vbuf[guard:].view(B, bsv)[:, :n]
    Vv.copy_(dev(V[:B], dtype))
    assert Vv.stride(0) == bsv and (B == 1 or not Vv.is_contiguous())
    jit, rr = dev(s2[:B], torch.float64), dev(r[:B], dtype)
    fn = _lib.lib().volt_vk_forms_f32 if dtype == torch.float32 else _lib.lib().volt_vk_forms_f64

    def run():
        obuf[:B * 4].fill_(float("nan"))
        _lib.check(fn(Vv.data_ptr(), bsv if B > 1 else 0, jit.data_ptr(), rr.data_ptr(), obuf.data_ptr(), ibuf.data_ptr(), B, n,
                      _lib.stream_ptr()), "volt_vk_forms")
        return obuf[:B * 4].view(B, 4).clone(), ibuf[:B].clone()
    first = run()
    check_forms(host(first[0]), want[:B], V[:B], r[:B], n)
    assert not first[1].any()
    for _ in range(9):
        o, i = run()
        assert torch.equal(o, first[0]) and torch.equal(i, first[1])
    assert torch.isnan(obuf[B * 4:]).all() and bool((ibuf[B:] == -77).all())
    o, i = ops.vk_forms(Vv, jit, rr)
    assert torch.equal(o, first[0]) and torch.equal(i, first[1])


def test_vk_forms_info_is_per_series():
    from volt_amd import ops
    n = 70
    V, s2, r, want = case(n)
    keep = [b for b in range(12) if (np.diff(V[b], prepend=0.0) > 0).all()][:3]
    V3, r3 = V[keep].copy(), r[keep]
    V3[1, 41] = V3[1, 40]                                          # ONE flat step in ONE series: d_41 = 0 at jitter 0
    out, info = ops.vk_forms(dev(V3), 0.0, dev(r3))
    assert info.tolist() == [0, 42, 0] and torch.isnan(out[1]).all() and torch.isfinite(out[[0, 2]]).all()
    good, ginfo = ref.forms_ref(V3, 0.0, r3)
    assert ginfo.tolist() == [0, 42, 0]
    check_forms(host(out[[0, 2]]), good[[0, 2]], V3[[0, 2]], r3[[0, 2]], n)
    out, info = ops.vk_forms(dev(V3), torch.tensor([0.0, 1e-6, 0.0], device="cuda", dtype=torch.float64), dev(r3))     # a rung for that series alone
    assert not info.any()
    check_forms(host(out), ref.forms_ref(V3, [0.0, 1e-6, 0.0], r3)[0], V3, r3, n)
    Vn = V3.copy()
    Vn[2, 33] = np.nan                                             # a NaN in ONE series' grid
    out, info = ops.vk_forms(dev(Vn), 1e-4, dev(r3))
    assert info.tolist()[:2] == [0, 0] and info[2] != 0 and torch.isfinite(out[:2]).all() and torch.isnan(out[2]).all()
    rn = r3.copy()
    rn[0, 12] = np.nan                                             # a NaN residual is not a pivot failure
    out, info = ops.vk_forms(dev(V3), 1e-4, dev(rn))
    assert not info.any() and torch.isfinite(out[0, [0, 3]]).all() and torch.isnan(out[0, [1, 2]]).all()


def test_vk_forms_validates_shapes():
    from volt_amd import ops
    V, r = (torch.zeros(3, 8, device="cuda") for _ in range(2))
    with pytest.raises(ValueError, match="resid must be"):
        ops.vk_forms(V, 0.0, r[0])
    with pytest.raises(ValueError, match="V must be"):
        ops.vk_forms(V[:, :7], 0.0, r)
    with pytest.raises(ValueError, match="disagree on B"):
        ops.vk_forms(V[:2], 0.0, r)


@pytest.mark.parametrize("B,n", [(3, 65), (65, 399), (2, 4096)])
def test_vk_forms_quadratic_form_and_logdet_are_the_vk_steps(B, n):
    """With jitter = sigma2, out[:, 2] and out[:, 3] are the r'A^-1 r and logdet ops.vk_step returns on the same inputs (the
    same pivot chain): to the bound for the fp64 step, plus one fp32 rounding of the step's outputs for the fp32 step.  The two
    kernels run the same pivot, z chain and log-determinant (csrc/chain.h), so the fp64 step's two numbers are the forms' bit for bit."""
    from volt_amd import ops
    V, s2, r, want = case(n) if n != 4096 else case(n, B=2, seed=3)
    V, s2, r, want = V[:B], s2[:B], r[:B], want[:B]
    scale = f64_tol(n) * ref.forms_scales(V, r, want)[:, 2:]
    for dtype, eps in ((torch.float64, 0.0), (torch.float32, EPS32)):
        out, info = ops.vk_forms(dev(V, dtype), dev(s2, torch.float64), dev(r, dtype))
        o, _, sinfo = ops.vk_step(dev(V, dtype), dev(s2, dtype), dev(r, dtype), want_grad=False)
        assert not info.any() and not sinfo.any()
        err = np.abs(host(out)[:, 2:] - host(o)[:, 2:4])
        assert (err <= scale + eps * np.abs(want[:, 2:])).all(), (dtype, (err / scale).max())
        if dtype == torch.float64:
            assert host(out)[:, 2:].tobytes() == host(o)[:, 2:4].tobytes(), (host(out)[:, 2:], host(o)[:, 2:4])


# ------------------------------------------------------------------------------------------------ 2: the ladder
def test_safe_forms_applies_the_jitter_ladder():
    from volt_amd import gp
    n = 70
    V, _, r, _ = case(n)
    keep = [b for b in range(12) if (np.diff(V[b], prepend=0.0) > 0).all()][:3]
    V3, r3 = V[keep].copy(), r[keep]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                             # plain first: silent, jitter 0
        out, used = gp._safe_forms(dev(V3), dev(r3), 1e-4)
    assert used == 0.0
    check_forms(host(out), ref.forms_ref(V3, 0.0, r3)[0], V3, r3, n)
    V3[1, 41] = V3[1, 40]
    for dtype, jitter, rung in ((torch.float32, 1e-4, 1e-4), (torch.float32, None, 1e-6), (torch.float64, None, 1e-8)):
        with pytest.warns(gp.NumericalWarning, match=f"A not p.d., added jitter of {rung:.1e} to the diagonal"):
            out, used = gp._safe_forms(dev(V3, dtype), dev(r3, dtype), jitter)
        assert used == rung                                        # the whole batch moves to the rung
        check_forms(host(out), ref.forms_ref(V3, rung, r3)[0], V3, r3, n)
    Vn = V3.copy()
    Vn[0, 5] = np.nan
    with pytest.raises(gp.NanError):
        gp._safe_forms(dev(Vn), dev(r3), 1e-4)
    Vd = V3.copy()
    Vd[2, 30:] -= 1.0                                              # a DEcreasing grid: delta = -1, no rung up to 1e-2 helps
    with pytest.raises(gp.NotPSDError, match="after repeatedly adding jitter up to 1.0e-02"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gp._safe_forms(dev(Vd), dev(r3), 1e-4)


# ------------------------------------------------------------------------------------------------ 3: the draw
def _draw_args(x, y, vol, test_x, pv, z, per_sample=False):
    S, T = pv.shape
    N = x.shape[0]
    full_x = dev(np.concatenate([x, test_x]))
    full_vol = torch.cat((dev(vol).unsqueeze(0).repeat(S, 1), dev(pv)), -1)
    td = dev(y - ref.linear_mean(x)).reshape(1, N, 1)
    if per_sample:
        td = td.repeat(S, 1, 1)
    tm = dev(ref.linear_mean(test_x)).reshape(1, T, 1)
    return full_x, full_vol, N, td, tm, dev(z).reshape(S, T, 1)


@pytest.mark.parametrize("N,T,S", ref.DRAW_SHAPES)
def test_linear_draw_is_at_least_as_accurate_as_the_dense_fp32_draw(N, T, S):
    """_posterior_draw_linear beside _posterior_draw on the same inputs and draws, against the fp64 oracle: per output the linear
    error is at most the dense fp32 error + 2^-23 |ref| (one rounding of the fp32 output; the comparative criterion of
    test_linear_step_is_at_least_as_accurate_as_the_dense_fp32_step), and both meet the 2e-3 pathwise bound of README row a7.
    The negative control of tests/test_vk_forms_host.py against THIS criterion: the train-only CumTrapz misses it by > 10 x."""
    from volt_amd.kernels import VolatilityKernel
    from volt_amd.rollout_utils import _posterior_draw, _posterior_draw_linear
    x, y, vol, test_x, pv, z, want = ref.draw_case(N, T, S)
    args = _draw_args(x, y, vol, test_x, pv, z)
    k = VolatilityKernel().cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                            # (the dense fp32 factor may take a rung; the linear one may not)
        dense = host(_posterior_draw(k, *args, 1e-4).squeeze(-1))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lin_t = _posterior_draw_linear(k, *args, 1e-4)
    assert lin_t.dtype == torch.float32 and tuple(lin_t.shape) == (S, T, 1)
    lin = host(lin_t.squeeze(-1))
    e_lin, e_dense = np.abs(lin - want), np.abs(dense - want)
    bound = e_dense + EPS32 * np.abs(want)
    print(f"draw N = {N} T = {T} S = {S}: max error linear {e_lin.max():.3e}  dense fp32 {e_dense.max():.3e}  "
          f"largest linear / bound {(e_lin / bound).max():.3f}  largest linear / (2^-23 |ref|) {(e_lin / (EPS32 * np.abs(want))).max():.3f}")
    assert (e_lin <= bound).all(), (np.argwhere(e_lin > bound)[:4], (e_lin / bound).max())
    assert e_lin.max() <= 2e-3 and e_dense.max() <= 2e-3
    bad = ref.draw_ref(x, y, np.log(vol.astype(np.float64)), test_x, pv, z, ref.linear_mean, train_only=True)
    assert (np.abs(bad - want) / bound).max() > 10
    # per-sample grids: samples 1 .. S-1 get a history of their own, one step of 2^-20 away in one vol (which moves the truth by
    # ~1e-10): S grids in one launch -- sample 0 to the bit, every sample within the criterion
    a = _draw_args(x, y, vol, test_x, pv, z, per_sample=True)
    fv = a[1].clone()
    fv[1:, 0] *= 1.0 + 2.0 ** -20
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        per = host(_posterior_draw_linear(k, a[0].unsqueeze(0).repeat(S, 1), fv, *a[2:], 1e-4).squeeze(-1))
    assert np.array_equal(per[0], lin[0]) and (np.abs(per - want) <= bound + 1e-9).all()


@pytest.mark.parametrize("theta", [None, 0.3], ids=["plain", "theta"])
def test_linear_draw_with_per_sample_histories_and_theta(theta):
    """What the dense Rollouts engine hands the draw after its first step: S different histories [S,N], T = 1, with and
    without the mean reversion -- against the fp64 oracle on the same numbers, within 2^-23 |ref|: everything up to the one
    rounding of the fp32 output is fp64 here (T = 1: no fp32 factor), and the fp32 residual y - m is exact (y / 2 <= m <= 2 y)."""
    from volt_amd.kernels import VolatilityKernel
    from volt_amd.rollout_utils import _posterior_draw_linear
    from oracle import volt_oracle as vo
    N, S = 95, 6
    rng = np.random.default_rng(4)
    x = (np.arange(N) / 252.).astype(np.float32)
    test_x = (x[-1:] + x[1]).astype(np.float32)
    y = (2.3 + np.cumsum(0.012 * rng.standard_normal((S, N)), -1)).astype(np.float32)
    lv = (np.log(0.2) + np.cumsum(0.05 * rng.standard_normal((S, N)), -1)).astype(np.float32)
    vol = np.exp(lv.astype(np.float64)).astype(np.float32)
    pv = (0.2 * np.exp(0.1 * rng.standard_normal((S, 1)))).astype(np.float32)
    z = rng.standard_normal((S, 1, 1)).astype(np.float32)
    kw = dict(latent_mean=None if theta is None else 2.25, theta=0.5 if theta is None else theta)
    tx = np.repeat(x[None], S, 0)
    want = vo.generate_prediction(tx, y, np.log(vol.astype(np.float64)), test_x, pv, z, ref.linear_mean, dtype=np.float64, **kw)
    full_x = torch.cat((dev(tx), dev(test_x).unsqueeze(0).repeat(S, 1)), -1)
    full_vol = torch.cat((dev(vol), dev(pv)), -1)
    td = dev(y - ref.linear_mean(tx)).unsqueeze(-1)
    tm = dev(ref.linear_mean(test_x)).reshape(1, 1, 1)
    lat = None if theta is None else torch.tensor(2.25, device="cuda")
    got = host(_posterior_draw_linear(VolatilityKernel().cuda(), full_x, full_vol, N, td, tm, dev(z), 1e-4, lat, kw["theta"]))
    err = np.abs(got.reshape(S, 1) - want)
    print(f"per-sample histories, theta = {theta}: max error {err.max():.3e}")
    assert (err <= EPS32 * np.abs(want)).all()


def test_linear_draw_on_a_flat_step_warns_and_matches_the_conditional_at_its_rung():
    from volt_amd import gp
    from volt_amd.kernels import VolatilityKernel
    from volt_amd.rollout_utils import _posterior_draw_linear
    x, y, vol, test_x, pv, z, want = ref.flat_case()
    args = _draw_args(x, y, vol, test_x, pv, z)
    k = VolatilityKernel().cuda()
    with pytest.warns(gp.NumericalWarning, match="A not p.d., added jitter of 1.0e-04 to the diagonal"):
        got = host(_posterior_draw_linear(k, *args, 1e-4).squeeze(-1))
    err = np.abs(got - want)
    print(f"flat step: max error against the fp64 conditional at the rung {err.max():.3e}")
    assert (err <= EPS32 * np.abs(want).max()).all()
    voln = np.array(vol)
    voln[17] = np.nan
    with pytest.raises(gp.NanError):
        _posterior_draw_linear(k, *_draw_args(x, y, voln, test_x, pv, z), 1e-4)
    with pytest.raises(TypeError, match="volatility kernel"):
        _posterior_draw_linear(torch.nn.Identity(), *args, 1e-4)


# ------------------------------------------------------------------------------------------------ 4: the bordered engine
@pytest.mark.parametrize("G,n", [(1, 399), (2, 4096)])
def test_train_block_terms_chain_is_at_least_as_close_to_the_closed_form_as_factor(G, n):
    """rho and tau of the three routes on the engine's own U and residual: |chain - closed| <= |factor - closed| per series,
    and both within tests/test_gpu_contract.py's bounds (rho 1e-6 relative, tau 1e-6 max |r| + 1e-7)."""
    from volt_amd import ops, rollout_engine as re_
    x, F, vol = sde_batch(G, n, seed=12)
    k = 25
    tx = dev(x)
    test_x = tx[-1:] + tx[1]
    logy = dev(F)[:, 1:].log()
    U = ops.cumtrapz(torch.cat((dev(vol), dev(vol[:, -1:])), -1), torch.cat((tx, test_x)), square=True)[:, :n].contiguous()
    r_tr = (logy - ops.ewma(logy, k)[:, :-1]).contiguous()
    rho_c, tau_c = re_.train_block_terms(U, r_tr, "closed")
    rho_f, tau_f = re_.train_block_terms(U, r_tr, "factor")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rho_l, tau_l = re_.train_block_terms(U, r_tr, "chain")
    assert rho_l.dtype == torch.float64 and tuple(rho_l.shape) == (G,) and tuple(tau_l.shape) == (G,)
    e = {name: ((rho - rho_c).abs(), (tau - tau_c).abs()) for name, rho, tau in (("chain", rho_l, tau_l), ("factor", rho_f, tau_f))}
    print(f"{G} x {n}: |rho - closed| chain {float(e['chain'][0].max()):.3e} factor {float(e['factor'][0].max()):.3e};  "
          f"|tau - closed| chain {float(e['chain'][1].max()):.3e} factor {float(e['factor'][1].max()):.3e}")
    assert bool((e["chain"][0] <= e["factor"][0]).all()) and bool((e["chain"][1] <= e["factor"][1]).all())
    for name in ("chain", "factor"):
        assert float((e[name][0] / rho_c.abs()).max()) < 1e-6
        assert float(e[name][1].max()) < 1e-6 * float(r_tr.abs().max()) + 1e-7


def test_rollouts_chain_route_matches_closed_form():
    """The shape of test_rollouts_factor_route_matches_closed_form, its 1e-5, info == 0."""
    from volt_amd import rollout_engine as re_
    n, S, H, k = 399, 64, 40, 25
    F, vol = sde_series(n, 11)
    pv, z = rollout_inputs(vol[-1], S, H, seed=5)
    tx = torch.arange(n, device="cuda") / 252.
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    args = (tx, torch.log(dev(F)[1:])[None], torch.log(dev(vol))[None], test_x, dev(pv)[None], dev(z)[None], 0, k)
    a, ia = re_.rollout_series(*args, solve="closed")
    b, ib = re_.rollout_series(*args, solve="chain")
    assert int((ia != 0).sum()) == 0 and int((ib != 0).sum()) == 0
    assert float((a - b).abs().max()) < 1e-5
    with pytest.raises(ValueError, match="unknown train-block solve"):
        re_.rollout_series(*args, solve="banded")


# ------------------------------------------------------------------------------------------------ 5: models and drivers
def _model(cls, tx, y, vol, predict_solver, k=20, **kw):
    from volt_amd.gp import GaussianLikelihood
    extra = {"k": k} if cls.__name__ == "VoltMagpie" else {}
    m = cls(tx, y, GaussianLikelihood().cuda(), vol, predict_solver=predict_solver, **extra, **kw).cuda()
    if cls.__name__ == "VoltronGP":
        with torch.no_grad():
            m.mean_module.weights.fill_(0.3)
            m.mean_module.bias.fill_(2.2)
    return m


@pytest.mark.parametrize("cls_name", ["VoltMagpie", "VoltronGP"])
def test_models_with_the_linear_predict_solver_match_the_dense_models(cls_name):
    """GeneratePrediction, SamplePrediction, the rollout_utils function and Rollouts on both engines: predict_solver="linear"
    against predict_solver="dense" on identical draws, within 2e-3 (README row a7: each is within that of the oracle's fp32
    run); Rollouts leaves both models in the same mutated state.  The data solver is independent of it."""
    from volt_amd import models
    from volt_amd.gp import _VolPrior
    from volt_amd.rollout_utils import GeneratePrediction, Rollouts
    cls = getattr(models, cls_name)
    n, H, S = 90, 6, 5
    F, vol = sde_series(n, 31)
    tx = torch.arange(n, device="cuda") / 252.
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    prices, y, vp = dev(F), dev(F)[1:].log(), dev(vol)
    pv = dev(np.full(H, vol[-1], dtype=np.float32))
    g = torch.Generator().manual_seed(5)
    pred_vol = (vp[-1].log() + 0.05 * torch.randn(S, H, generator=g).cumsum(-1).cuda()).exp()
    z = torch.randn(S, H, generator=g).cuda()
    # (the EWMA mean answers a multi-point x with its whole moving average, EWMA.py:46-54: as in the reference, VoltMagpie's
    # joint prediction is one point at a time; VoltronGP's linear mean takes the H points at once)
    Hm = H if cls_name == "VoltronGP" else 1
    mx = test_x[:Hm]
    outs, states = {}, {}
    for solver in ("linear", "dense"):
        m = _model(cls, tx, y, vp, solver)
        assert m.predict_solver == solver and m.data_solver == "dense" and torch.is_tensor(m.train_cov)
        torch.manual_seed(11)
        outs[solver, "method"] = m.GeneratePrediction(mx, pv[:Hm], 3)
        torch.manual_seed(11)
        outs[solver, "method1"] = m.GeneratePrediction(test_x[:1], pv[:1])
        m.vol_model.eval()
        torch.manual_seed(12)
        outs[solver, "sample"] = m.SamplePrediction(mx, n_sample=2)
        torch.manual_seed(12)
        outs[solver, "mean"] = m.MeanPrediction(mx, n_sample=2)
        fargs = (tx, prices, mx, pred_vol[:, :Hm], m)
        outs[solver, "function"] = GeneratePrediction(*fargs, z=z[:, :Hm].unsqueeze(-1))
        outs[solver, "function_override"] = GeneratePrediction(*fargs, z=z[:, :Hm].unsqueeze(-1),
                                                               solver="dense" if solver == "linear" else "linear")
        for engine in ("bordered", "dense"):
            m2 = _model(cls, tx, y, vp, solver)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                outs[solver, engine] = Rollouts(tx, prices, test_x, m2, nsample=S, pred_vol=pred_vol, z=z, engine=engine)
            states[solver, engine] = (m2.train_x, m2.train_y, m2.log_vol_path, m2.mean_module.train_x, m2.mean_module.train_y)
    assert tuple(outs["linear", "method"].shape) == (Hm, 3) and tuple(outs["linear", "method1"].shape) == (1,)
    for key in ("method", "method1", "sample", "mean", "function", "bordered", "dense"):
        a, b = outs["linear", key], outs["dense", key]
        assert torch.isfinite(a).all() and a.shape == b.shape
        err = float((a - b).abs().max())
        print(f"{cls_name} {key}: max |linear - dense| = {err:.3e}")
        assert err < 2e-3, key
        if key in ("method", "function", "dense"):
            assert not torch.equal(a, b), key                                  # another route, not the dense one renamed
    # solver= overrides the model's predict_solver: the override of one model is the other model's own route, bit for bit
    assert torch.equal(outs["linear", "function_override"], outs["dense", "function"])
    assert torch.equal(outs["dense", "function_override"], outs["linear", "function"])
    for engine in ("bordered", "dense"):
        for a, b in zip(states["linear", engine], states["dense", engine]):
            assert a.shape == b.shape and float((a - b).abs().max()) < 2e-3
        assert states["linear", engine][0].shape[-1] == n + H - 1
    # independent of the data solver: a linear-trained model predicts the same (prediction never reads train_cov)
    m = _model(cls, tx, y, vp, "linear", data_solver="linear")
    assert isinstance(m.train_cov, _VolPrior) and m.predict_solver == "linear"
    torch.manual_seed(11)
    assert torch.equal(m.GeneratePrediction(mx, pv[:Hm], 3), outs["linear", "method"])


def test_volt_forecast_with_the_linear_predict_solver():
    from volt_amd.models.Volt import Volt
    n, H, S = 130, 6, 8
    F, vol = sde_series(n, 5)
    tx = torch.arange(n + 1, device="cuda") / 252.
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    pv, z = rollout_inputs(vol[-1], S, H, seed=3)
    outs = {}
    for solver in ("linear", "dense"):
        for mr in (False, True):
            m = Volt(tx, dev(F).log(), mean="ewma", vol_path=dev(vol), k=10, predict_solver=solver)
            assert m.predict_solver == solver
            outs[solver, mr] = m.Forecast(test_x, nsample=S, mean_revert=mr, pred_vol=dev(pv), z=dev(z))
    for mr in (False, True):
        a, b = outs["linear", mr], outs["dense", mr]
        assert tuple(a.shape) == (S, H) and torch.isfinite(a).all()
        assert float((a - b).abs().max()) < 2e-3
    assert float((outs["linear", True] - outs["linear", False]).abs().max()) > 1e-4      # (theta did something)
    assert Volt(tx, dev(F).log(), mean="ewma", vol_path=dev(vol), k=10).predict_solver == "dense"


@pytest.mark.parametrize("mean", ["ewma", "constant"])
def test_stocks_driver_with_the_linear_predict_solver(mean, tmp_path):
    """The Rollouts branch (ewma: solve="chain") and the standard-mean branch (constant: one vk_forms launch for all tickers):
    the reference layout on disk, and the samples equal the per-series functions (the model built with predict_solver="linear")
    on the window's own vol path, vol forecast and draws within 2e-4, as test_batched_driver_matches_per_series_functions
    requires of the dense driver -- whichever route the per-series model takes."""
    from volt_amd import gp
    from volt_amd.forecast import GenerateStockPredictionsBatch, realised_vol
    from volt_amd.models import VoltMagpie
    from volt_amd.rollout_utils import GeneratePrediction, Rollouts
    B, T, ntrain, H, S, k = 3, 90, 80, 6, 7, 10
    x, F, vol = sde_batch(B, T - 1, seed=91)
    closes = dev(F)
    g = torch.Generator(device="cuda").manual_seed(4)
    dbg = {}
    out = GenerateStockPredictionsBatch(["A", "B", "C"], closes, forecast_horizon=H, train_iters=5, nsample=S, ntrain=ntrain,
                                        mean=mean, k=k, ntimes=1, vol_iters=2, vol_fn=realised_vol, generator=g, debug=dbg,
                                        save=True, par_dir=str(tmp_path), predict_solver="linear")
    assert tuple(out.shape) == (B, S, H) and torch.isfinite(out).all()
    files = sorted(p.name for p in (tmp_path / "B").iterdir())
    assert len(files) >= 1 and all(f.startswith(f"volt_{mean}{k}_") and f.endswith(".pt") for f in files)
    saved = torch.load(tmp_path / "C" / files[-1])
    assert tuple(saved.shape) == (S, H) and torch.equal(saved, out[2])
    train_x = torch.arange(ntrain - 1, device="cuda") / 252.
    test_x = torch.arange(H, device="cuda") / 252. + train_x[-1] + train_x[1]
    for b in range(B):
        ty = dbg["train_y"][b]
        for solver, tol in (("linear", 2e-4), ("dense", 2e-4)):                # the reference's per-ticker body, either route
            m = VoltMagpie(train_x, ty[1:].log(), gp.GaussianLikelihood().cuda(), dbg["vol"][b], k=k, predict_solver=solver)
            if mean == "ewma":
                want = Rollouts(train_x, ty, test_x, m, nsample=S, pred_vol=dbg["pred_vol"][b], z=dbg["z"][b])
            else:
                m.mean_module = gp.ConstantMean().cuda()
                m.mean_module.constant.data = dbg["model"].mean_module.constant.data[b].clone()
                want = GeneratePrediction(train_x, ty, test_x, dbg["pred_vol"][b], m, z=dbg["z"][b]).detach().cpu()
            print(f"{mean} series {b}: max |driver - per-series {solver}| = {float((out[b] - want).abs().max()):.3e}")
            np.testing.assert_allclose(out[b].numpy(), want.numpy(), atol=tol, rtol=0)
    with pytest.raises(ValueError, match="solver must be one of"):
        GenerateStockPredictionsBatch(["A", "B", "C"], closes, forecast_horizon=H, train_iters=1, nsample=S, ntrain=ntrain,
                                      mean=mean, k=k, ntimes=1, vol_iters=1, vol_fn=realised_vol, predict_solver="banded")


# ------------------------------------------------------------------------------------------------ 6: no N^2 anywhere
def test_no_quadratic_memory_at_n_65536():
    """2 x 65536 with a linear data model: the model method GeneratePrediction (H = 20, 8 draws per point) and
    rollout_series(solve="chain") (S = 8, H = 20) each grow the peak of allocated device memory by less than 64 MB above
    their inputs -- one dense fp32 train block of this size would be 17 GB -- and return finite samples."""
    from volt_amd import rollout_engine as re_
    from volt_amd.gp import GaussianLikelihood, _VolPrior
    from volt_amd.models import VoltronGP
    n, B, H, S = 65536, 2, 20, 8
    rng = np.random.default_rng(9)
    vol = vk.f32(np.stack([vk.vol_path("smooth", n, rng, 0.2), vk.vol_path("lognormal", n, rng, 0.6)]))
    y = vk.resid(B, n, rng) + 4.0
    tx, yt, vp = torch.arange(n, device="cuda") / 252., dev(y), dev(vol)
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    lh = GaussianLikelihood(batch_shape=torch.Size([B])).cuda()
    m = VoltronGP(tx, yt, lh, vp, vol_solver="linear", data_solver="linear", predict_solver="linear").cuda()
    with torch.no_grad():
        m.mean_module.weights.fill_(0.01)
        m.mean_module.bias.fill_(2.0)
    assert isinstance(m.train_cov, _VolPrior)
    pv = dev(np.repeat(vol[:, -1:], H, 1))
    pvs, z = rollout_inputs(vol[:, -1], S, H, seed=2)
    pvs, z = dev(pvs), dev(z)
    torch.manual_seed(3)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = m.GeneratePrediction(test_x, pv, S)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"GeneratePrediction at 2 x 65536: peak above the inputs {grown / 2 ** 20:.1f} MB")
    assert tuple(out.shape) == (B, H, S) and torch.isfinite(out).all()
    assert grown < 64 * 2 ** 20, grown
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    samples, info = re_.rollout_series(tx, yt, vp.log(), test_x, pvs, z, 0, 25, solve="chain")
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"rollout_series(solve='chain') at 2 x 65536: peak above the inputs {grown / 2 ** 20:.1f} MB")
    assert tuple(samples.shape) == (B, S, H) and torch.isfinite(samples).all() and not info.any()
    assert grown < 64 * 2 ** 20, grown
