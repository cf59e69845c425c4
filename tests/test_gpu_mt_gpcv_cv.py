"""The multi-task GPCV step with the copula-process ("cv") likelihood, one warp per task, on the MI355X:
volt_gpcv_mt_cv_step_f32 (csrc/gpcv_mt_cv.hip + csrc/gpcv_mt.hip), VariationalELBO over MultitaskVariationalGP with a
``batch_shape=[T]`` likelihood, the "cv" start-up, FitGPCVMultitask / LearnGPCVMultitask(param="cv") and the stocks driver's
``multitask_gpcv`` / ``gpcv_options``.

The oracle is the fp64 restatement of tests/mt_gpcv_cv_ref.py (checked against the dense NT x NT definition in
tests/test_mt_gpcv_cv_host.py), the inputs are its named Cases, and the bounds are the project's own
(tests/test_gpu_mt_gpcv.py, tests/test_gpu_gpcv_cv.py): the 13 scalars and F 5e-5 max(1, |ref|); grad_M, grad_Lx, grad_Lt,
grad_c, grad_covar_factor, grad_raw_var 2e-3 of the array's largest reference entry; grad_K 5e-3; grad_a, grad_b, grad_c
2e-3 of each array's largest reference entry over all tasks.  tests/test_mt_gpcv_cv_host.py holds the fp32 CPU evaluation
of the restatement to half of each bound at the same inputs.  The largest error / bound per group is printed before it
is asserted."""
import math
import warnings

import pytest
import torch

import gpcv_cv_ref as CV
import mt_gpcv_cv_ref as C
import mt_gpcv_ref as R
from volt_amd.synthetic import sde_series

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTPUTS = ("out", "grad_M", "grad_c", "grad_Lx", "grad_Lt", "grad_covar_factor", "grad_raw_var", "grad_K", "grad_abc")


def _f(t):
    return t.float().to(DEV)


def _gh(Q=75):
    gx, gw = R.gauss_hermite(Q)
    return _f(gx), _f(gw)


def _abc(raws):
    """The step's abc [T,3,K]: the transformed a, b, c of every task (fp64, on the CPU)."""
    return torch.stack(CV.constrain(*(raws[k] for k in C.RAW_KEYS)), 1)


def _run(cs, w_ell=None, ws=None):
    from volt_amd import ops
    c = C.make(cs)
    p, (we, wk) = c["p"], C.weights(cs)
    ws = ops.gpcv_mt_step(_f(c["K"]), _f(p["m"]), _f(p["c"]), _f(p["Lx"]), _f(p["Lt"]), _f(p["F"]), _f(p["raw_var"]), _f(c["y"]),
                          *_gh(cs.Q), ws, want_dk=cs.dk, w_ell=we if w_ell is None else w_ell, w_kl=wk, abc=_f(_abc(c["raws"])))
    torch.cuda.synchronize()
    return ws


def _grads(ws):
    g = {"m": ws.grad_M, "Lx": ws.grad_Lx, "Lt": ws.grad_Lt, "F": ws.grad_covar_factor, "raw_var": ws.grad_raw_var,
         "c": ws.grad_c, "lik_a": ws.grad_abc[:, 0], "lik_b": ws.grad_abc[:, 1], "lik_c": ws.grad_abc[:, 2]}
    if ws.grad_K is not None:
        g["K"] = ws.grad_K
    return {k: v.double().cpu() for k, v in g.items()}


def _check(cs, ws):
    assert ws.info.tolist() == [0, 0, 0], (cs, ws.info.tolist())
    g = _grads(ws)
    assert bool(torch.isfinite(ws.out).all()) and [k for k, v in g.items() if not bool(torch.isfinite(v).all())] == [], cs
    r = C.ratios(cs, ws.out.double().cpu()[:13], g)
    print(f"MTCV ({cs.N},{cs.T}) K={cs.K} {cs.kernel} x0={cs.x0} Q={cs.Q} clamp={cs.clamp} largest error/bound:",
          " ".join(f"{k}={v:.2e}" for k, v in C.group_max(r).items()))
    assert R.over(r) == {}, cs                                                        # item by item: NaN does not pass
    assert float(ws.out[13]) == pytest.approx(R.JITTER) and not ws.out[14:].any()
    assert not ws.grad_Lx.triu(1).any() and not ws.grad_Lt.triu(1).any()
    return r


# -------------------------------------------------------------------------------------------- the step against the oracle
_id = lambda c: f"{c.N}x{c.T}-K{c.K}-{c.kernel}-x{c.x0}" + (f"-Q{c.Q}" if c.Q != 75 else "")


@pytest.mark.parametrize("cs", C.STEP_CASES, ids=_id)
def test_step_matches_oracle(cs):
    _check(cs, _run(cs))


@pytest.mark.parametrize("N", C.EDGE_N)
def test_edge_shapes(N):
    """N around the pass's 16-row workgroups, T around the eight waves of a workgroup, the 256 | 1024 threads of the task
    algebra and the task limit, T > N included."""
    for cs in C.EDGE_CASES:
        if cs.N == N:
            _check(cs, _run(cs))


@pytest.mark.parametrize("cs", C.Q_CASES, ids=_id)
def test_node_counts(cs):
    """Q = 1 (63 idle lanes), 20, 75 (two trips of the node loop, the second with 11 lanes)."""
    _check(cs, _run(cs))


def test_weights_other_than_the_models():
    ws = _run(C.W_CASE)
    _check(C.W_CASE, ws)
    o = ws.out.double().cpu()
    assert abs(float(o[12] - (0.37 * o[0] - 2.5 * o[1]))) <= 1e-6 * abs(float(o[12]))


@pytest.mark.parametrize("cs", C.REDUCE_CASES, ids=_id)
def test_both_sides_of_the_reductions_staging_edge(cs):
    """256 and 257 workgroup partials per task against the 256 threads of the fixed-order reduction: ell and grad_abc against
    the O(N T Q K) part of the restatement (the N^3 part of this shape is tests/test_gpu_mt_gpcv.py's ground)."""
    c = C.make(cs)
    ws = _run(cs)
    assert ws.info.tolist() == [0, 0, 0]
    e, g = C.ell_and_abc_grads(c["p"], c["y"], c["raws"])
    r = {"ell": abs(float(ws.out[0]) - float(e)) / (R.TOL_SCALAR * max(1.0, abs(float(e))))}
    for i, k in enumerate(C.ABC_KEYS):
        want = g[k] / cs.N                                                           # grad_abc = w_ell d ell / d(a,b,c)
        r["grad_" + k] = float((ws.grad_abc[:, i].double().cpu() - want).abs().max() / want.abs().max()) / C.TOL_ABC
    print(f"MTCV reduce ({cs.N},{cs.T}) error/bound:", " ".join(f"{k}={v:.2e}" for k, v in r.items()))
    assert R.over(r) == {}


# ------------------------------------------------------------------------------------------------- the clamp and the floor
def test_clamped_scales():
    """tril(Lx) x CLAMP_FACTOR: more than 5 % of the nodes sit under the min_scale clamp (no gradient through them)."""
    cs = C.CLAMP_CASE
    share = C.reference(cs)[0]["clamped"]
    print("MTCV clamp: share of nodes under min_scale", f"{share:.3f}")
    assert share > 0.05
    _check(cs, _run(cs))


def test_floored_variances():
    """Every third row of Lx and row 1 of Lt x 1e-4: those rows of grad_Lx (floored at every t) and that row of grad_Lt
    (floored at every n) are bitwise those of a w_ell = 0 run -- the variance derivative is zero where the variance is
    floored -- and the others are not."""
    cs = C.FLOOR_CASE
    c = C.make(cs)
    floored = R._var(c["p"]) < R.MIN_VAR
    rows, task = floored.all(1), floored.all(0)
    print("MTCV floor: floored share", float(floored.double().mean()), "rows", int(rows.sum()), "tasks", task.tolist())
    assert float(floored.double().mean()) > 0.05 and int(rows.sum()) >= cs.N // 3 and task.tolist() == [False, True, False]
    assert int(((R._var(c["p"]) / R.MIN_VAR - 1).abs() < 1e-3).sum()) == 0          # no variance at the threshold
    ws = _run(cs)
    _check(cs, ws)
    gLx, gLt = ws.grad_Lx.cpu(), ws.grad_Lt.cpu()
    kl = _run(cs, w_ell=0.0)
    assert bool(torch.isfinite(kl.grad_Lx).all()) and bool(torch.isfinite(kl.grad_Lt).all())
    assert torch.equal(gLx[rows], kl.grad_Lx.cpu()[rows]) and not torch.equal(gLx[~rows], kl.grad_Lx.cpu()[~rows])
    assert torch.equal(gLt[task], kl.grad_Lt.cpu()[task]) and not torch.equal(gLt[~task], kl.grad_Lt.cpu()[~task])
    assert not kl.grad_abc.any()


# ------------------------------------------------------------------------------------------------------------ cross-checks
def test_one_task_equals_the_single_task_cv_step():
    """T = 1 with K_t = S_t = 1 is ops.gpcv_cv_step on the same inputs: twice the oracle bounds, as
    tests/test_gpu_mt_gpcv.py::test_one_task_equals_the_single_task_step."""
    from volt_amd import ops
    N, Kc = 399, 5
    p, x, y = R.case(N, 1, seed=7)
    p["F"] = torch.zeros(1, 1, dtype=torch.float64)
    p["raw_var"] = torch.tensor([math.log(math.e - 1)], dtype=torch.float64)
    p["Lt"] = torch.ones(1, 1, dtype=torch.float64)
    abc = _f(_abc(C.draw_raws(1, Kc, 3)))
    K = _f(R.data_cov(x, p["raw_vol"]))
    gx, gw = _gh()
    ws = ops.gpcv_mt_step(K, _f(p["m"]), _f(p["c"]), _f(p["Lx"]), _f(p["Lt"]), _f(p["F"]), _f(p["raw_var"]), _f(y), gx, gw,
                          w_ell=1.0 / N, w_kl=1.0 / N, abc=abc)
    m, c = _f(p["m"][:, 0]).reshape(1, N), _f(p["c"])
    st = ops.gpcv_cv_step(K.unsqueeze(0), m - c, m, _f(p["Lx"]).unsqueeze(0), _f(y[:, 0]).reshape(1, N), abc, gx, gw,
                          w_ell=1.0 / N, w_kl=1.0 / N)
    torch.cuda.synchronize()
    assert ws.info.tolist() == [0, 0, 0] and int(st.info.abs().sum()) == 0
    F1, F0 = float(ws.out[12]), float(st.out[0, 9])
    d = {"F": abs(F1 - F0) / max(1.0, abs(F0)),
         "grad_M": float((ws.grad_M[:, 0] - st.grad_m[0]).abs().max() / st.grad_m[0].abs().max()),
         "grad_Lx": float((ws.grad_Lx - st.grad_Lq[0]).abs().max() / st.grad_Lq[0].abs().max()),
         "grad_mu": abs(float(ws.grad_c[0]) - float(st.grad_mu[0].sum())) / max(1.0, abs(float(st.grad_mu[0].sum())))}
    for i, k in enumerate("abc"):
        d["grad_" + k] = float((ws.grad_abc[0, i] - st.grad_abc[0, i]).abs().max() / st.grad_abc[0, i].abs().max())
    print("MTCV T = 1 vs ops.gpcv_cv_step, largest differences:", {k: f"{v:.2e}" for k, v in d.items()})
    assert d["F"] <= 2 * 5e-5
    assert all(d[k] <= 2 * 2e-3 for k in d if k != "F"), d


def test_exp_limit_equals_the_exp_step():
    """a = e^20, b = 1, c = -20 for every task: scale(f) = e^20 softplus(f - 20) = exp f to 1e-8 at these f.  Against
    ops.gpcv_mt_step: out to 5e-5, gradients to 2e-3; out[1:12] does not depend on the likelihood and is the same launches on
    the same buffers: bitwise."""
    from volt_amd import ops
    N, T = 399, 8
    p, x, y = R.case(N, T, seed=100 + N + T)
    args = (_f(R.data_cov(x, p["raw_vol"])), _f(p["m"]), _f(p["c"]), _f(p["Lx"]), _f(p["Lt"]), _f(p["F"]), _f(p["raw_var"]), _f(y),
            *_gh())
    abc = torch.tensor([math.exp(20.0), 1.0, -20.0], device=DEV).reshape(1, 3, 1).repeat(T, 1, 1)
    ex = ops.gpcv_mt_step(*args, want_dk=True, w_ell=1.0 / N, w_kl=1.0 / (N * T))
    cv = ops.gpcv_mt_step(*args, want_dk=True, w_ell=1.0 / N, w_kl=1.0 / (N * T), abc=abc)
    torch.cuda.synchronize()
    assert ex.info.tolist() == [0, 0, 0] and cv.info.tolist() == [0, 0, 0]
    assert torch.equal(ex.out[1:12], cv.out[1:12])
    eo = float(((ex.out - cv.out).abs() / ex.out.abs().clamp_min(1.0)).max())
    d = {n: float((getattr(ex, n) - getattr(cv, n)).abs().max() / getattr(ex, n).abs().max()) for n in OUTPUTS[1:8]}
    print("MTCV exp limit: out", f"{eo:.2e}", {k: f"{v:.2e}" for k, v in d.items()})
    assert eo <= 5e-5 and all(v <= 2e-3 for v in d.values()), d


# ------------------------------------------------------------------------------------------------------ guards and repeats
PAD = 64


class _Guarded:
    """A tensor of ``shape`` inside a larger buffer filled with NaN (floats) or -77 (ints)."""

    def __init__(self, shape, dtype=torch.float32):
        self.n = math.prod(shape)
        self.fill = float("nan") if dtype == torch.float32 else -77
        self.buf = torch.full((self.n + 2 * PAD,), self.fill, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + self.n].view(shape)

    def intact(self):
        edge = torch.cat([self.buf[:PAD], self.buf[PAD + self.n:]]).view(torch.int32)
        return bool((edge == torch.full((1,), self.fill, dtype=self.buf.dtype, device=DEV).view(torch.int32)).all())


def _inputs(N, T, Kc, seed=11):
    p, x, y = R.case(N, T, seed=seed)
    gx, gw = _gh()
    return dict(K=_f(R.data_cov(x, p["raw_vol"])), M=_f(p["m"]), c=_f(p["c"]), Lx=_f(p["Lx"]), Lt=_f(p["Lt"]),
                cf=_f(p["F"]).reshape(-1), rv=_f(p["raw_var"]), y=_f(y), abc=_f(_abc(C.draw_raws(T, Kc, seed))).contiguous(),
                gx=gx, gw=gw)


def _workspace(N, T, want_dk, Kc, poison=False):
    from volt_amd import _lib, ops
    nbytes = _lib.lib().volt_gpcv_mt_cv_workspace_bytes(N, T, int(want_dk), Kc)
    buf, ptr = ops._scratch(nbytes, DEV)
    buf.fill_(255 if poison else 0)
    with torch.cuda.device(buf.device):
        _lib.check(_lib.lib().volt_mll_workspace_init_f32(ptr, 1, N, 1, _lib.stream_ptr()), "volt_mll_workspace_init")
    return buf, ptr


def _raw_step(inp, N, T, want_dk, ws=None, poison=False, outs=None):
    """volt_gpcv_mt_cv_step_f32 through the ctypes binding, every output inside sentinels."""
    from volt_amd import _lib
    Kc = inp["abc"].shape[2]
    if ws is None:
        ws = _workspace(N, T, want_dk, Kc, poison)
    if outs is None:
        shapes = dict(out=(16,), grad_M=(N, T), grad_c=(T,), grad_Lx=(N, N), grad_Lt=(T, T), grad_covar_factor=(T,),
                      grad_raw_var=(T,), grad_K=(N, N), grad_abc=(T, 3, Kc))
        outs = {k: _Guarded(shapes[k]) for k in OUTPUTS if want_dk or k != "grad_K"}
        outs["info"] = _Guarded((3,), torch.int32)
    K = inp["K"]
    assert K.stride(1) == 1 and all(inp[k].is_contiguous() for k in ("M", "c", "Lx", "Lt", "cf", "rv", "y", "abc", "gx", "gw"))
    ptr = lambda k: outs[k].t.data_ptr() if k in outs else None
    with torch.cuda.device(torch.device(DEV)):
        _lib.check(_lib.lib().volt_gpcv_mt_cv_step_f32(
            K.data_ptr(), K.stride(0), R.JITTER, inp["M"].data_ptr(), inp["c"].data_ptr(), inp["Lx"].data_ptr(),
            inp["Lt"].data_ptr(), inp["cf"].data_ptr(), inp["rv"].data_ptr(), inp["y"].data_ptr(), inp["abc"].data_ptr(), Kc,
            inp["gx"].data_ptr(), inp["gw"].data_ptr(), inp["gx"].numel(), R.MIN_VAR, R.MIN_SCALE, 1.0 / N, 1.0 / (N * T),
            *[ptr(k) for k in OUTPUTS], ptr("info"), ws[1], N, T, _lib.WS_INITIALISED, _lib.stream_ptr()), "volt_gpcv_mt_cv_step")
    torch.cuda.synchronize()
    return outs, ws


def _same(a, b):
    return [k for k in a if k != "info" and not (torch.equal(a[k].t, b[k].t) and bool(torch.isfinite(a[k].t).all()))]


@pytest.mark.parametrize("want_dk", [False, True])
@pytest.mark.parametrize("N,T,Kc", [(129, 3, 5), (257, 17, 8)])
def test_guards(N, T, Kc, want_dk):
    """(1) nothing is written before or behind any output, grad_abc among them; (2) K as a view with ldk = N + 37 inside
    NaN, NaN in its strict upper triangle; (3) NaN above the diagonals of Lx and Lt; (4) a workspace whose every byte was 0xFF
    before volt_mll_workspace_init_f32 -- each bitwise the plain run."""
    inp = _inputs(N, T, Kc)
    base, _ = _raw_step(inp, N, T, want_dk)
    assert base["info"].t.tolist() == [0, 0, 0]
    assert [k for k, g in base.items() if not g.intact()] == []
    assert all(bool(torch.isfinite(base[k].t).all()) for k in base if k != "info")

    big = torch.full((N, N + 37), float("nan"), device=DEV)
    low = torch.ones(N, N, device=DEV).tril().bool()
    big[:, :N] = torch.where(low, inp["K"], big[:, :N])
    got, _ = _raw_step({**inp, "K": big[:, :N]}, N, T, want_dk)
    assert got["info"].t.tolist() == [0, 0, 0] and _same(base, got) == [], "strided K inside NaN"

    nan_above = lambda L: torch.where(torch.ones_like(L).tril().bool(), L, torch.full_like(L, float("nan")))
    got, _ = _raw_step({**inp, "Lx": nan_above(inp["Lx"]), "Lt": nan_above(inp["Lt"])}, N, T, want_dk)
    assert got["info"].t.tolist() == [0, 0, 0] and _same(base, got) == [], "NaN above the diagonals of Lx / Lt"

    got, _ = _raw_step(inp, N, T, want_dk, poison=True)
    assert got["info"].t.tolist() == [0, 0, 0] and _same(base, got) == [], "NaN-filled workspace"
    assert [k for k, g in got.items() if not g.intact()] == []


@pytest.mark.parametrize("N,T,Kc", [(399, 8, 5), (1024, 8, 8)])
def test_step_is_bitwise_repeatable(N, T, Kc):
    inp = _inputs(N, T, Kc)
    first, ws = _raw_step(inp, N, T, True)
    keep = {k: g.t.clone() for k, g in first.items()}
    for rep in range(29):
        again, _ = _raw_step(inp, N, T, True, ws=ws, outs=first)
        assert [k for k in keep if not torch.equal(keep[k], again[k].t)] == [], rep
    assert keep["info"].tolist() == [0, 0, 0] and all(bool(torch.isfinite(v).all()) for v in keep.values())


# ------------------------------------------------------------------------------------------------------------- the model
def _public(N, T, Kc, kernel="bm", seed=3):
    """A model on the device holding the parameters of R.case, a [T,Kc] likelihood holding C.draw_raws, and their ELBO."""
    from volt_amd.kernels import BMKernel, FBMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import MultitaskVariationalGP
    from volt_amd.variational import VariationalELBO
    p, x, y = R.case(N, T, seed=seed)
    raws = C.draw_raws(T, Kc, seed + 1)
    model = MultitaskVariationalGP(x.float().to(DEV), T, covar_module={"bm": BMKernel, "fbm": FBMKernel}[kernel]())
    lh = VolatilityGaussianLikelihood(K=Kc, batch_shape=torch.Size([T])).to(DEV)
    with torch.no_grad():
        model.variational_mean.copy_(p["m"])
        model.variational_covar_root.copy_(p["Lx"])
        model.variational_task_covar_root.copy_(p["Lt"])
        model.index_kernel.covar_factor.copy_(p["F"])
        model.index_kernel.raw_var.copy_(p["raw_var"])
        model.data_kernel.raw_vol.copy_(p["raw_vol"])
        for t, b in enumerate(model.mean_module.base_means):
            b.constant.fill_(float(p["c"][t]))
        for k in C.RAW_KEYS:
            getattr(lh, k).copy_(raws[k])
    return model, lh, VariationalELBO(lh, model, N * T), p, x, y, raws


@pytest.mark.parametrize("kernel", ["bm", "fbm"])
def test_variational_elbo_backward_against_fp64_autograd(kernel):
    """elbo(model(x), y).backward(): every model parameter and the likelihood's raw_a, raw_b, raw_c (through the
    constraints) against fp64 autograd on the restatement; expected_log_prob agrees with the step's ell."""
    from volt_amd.variational import num_gauss_hermite_locs
    N, T, Kc = 300, 3, 5
    model, lh, elbo, p, x, y, raws = _public(N, T, Kc, kernel)
    terms, grads = C.value_and_grads(C.struct, p, x, y, raws, kernel=kernel)
    rg = C.raw_grads(p, x, y, raws, kernel=kernel)
    xd, yd = model.inducing_points, y.float().to(DEV)
    with num_gauss_hermite_locs(75):
        val = elbo(model(xd), yd)
        val.backward()
        elp = lh.expected_log_prob(yd, model(xd)).detach()
    assert abs(float(val.detach()) - float(terms["F"])) <= 5e-5 * max(1.0, abs(float(terms["F"])))
    ref = {"variational_mean": grads["m"], "variational_covar_root": grads["Lx"], "variational_task_covar_root": grads["Lt"],
           "index_kernel.covar_factor": grads["F"], "index_kernel.raw_var": grads["raw_var"],
           "data_kernel.raw_vol": grads["raw_vol"]}
    ref.update({f"mean_module.base_means.{t}.constant": grads["c"][t].reshape(1) for t in range(T)})
    cmax = float(grads["c"].abs().max())
    for n, prm in list(model.named_parameters()) + list(lh.named_parameters()):
        assert prm.grad is not None and prm.grad.shape == prm.shape, n
        r = rg[n] if n in rg else ref[n]
        den = cmax if "constant" in n else float(r.abs().max())
        err = float((prm.grad.double().cpu() - r).abs().max()) / den
        print("MTCV elbo", kernel, n, f"{err:.2e}")
        assert err < 2e-3, n
    assert tuple(elp.shape) == (N, T)
    assert abs(float(elp.sum()) - float(elbo._mt_ws.out[0])) <= 5e-5 * max(1.0, abs(float(terms["ell"])))
    assert abs(float(elp.sum()) - float(terms["ell"])) <= 5e-5 * max(1.0, abs(float(terms["ell"])))


def test_error_kinds(monkeypatch):
    """NaN in abc: NanError; a non-PD prior: NotPSDError naming the piece; an internal code: VoltHipError.  (Crafted inputs
    and a patched info code; numerical conditions the step reports.)"""
    from volt_amd import gp, ops
    from volt_amd._lib import VoltHipError
    from volt_amd.gp import NanError, NotPSDError
    from volt_amd.variational import num_gauss_hermite_locs
    N, T, Kc = 200, 3, 5

    class DenseKernel(gp.Kernel):
        def __init__(self, K):
            super().__init__()
            self.K = torch.nn.Parameter(K)

        def forward(self, x1, x2=None, **kw):
            return self.K

    with num_gauss_hermite_locs(75):
        model, lh, elbo, p, x, y, _ = _public(N, T, Kc)
        yd = y.float().to(DEV)
        with torch.no_grad():
            lh.raw_b[1, 2] = float("nan")
        with pytest.raises(NanError):
            elbo(model(model.inducing_points), yd)
        assert elbo._mt_ws.info.tolist() == [0, 0, 1]
        model, lh, elbo, p, x, y, _ = _public(N, T, Kc)
        K = R.data_cov(x, p["raw_vol"]).float()
        K[57, 57] = -1.0
        model.data_kernel = DenseKernel(K).to(DEV)
        with pytest.raises(NotPSDError, match="prior covariance K_x"):
            elbo(model(model.inducing_points), yd)
        model, lh, elbo, p, x, y, _ = _public(N, T, Kc)
        real = ops.gpcv_mt_step

        def internal(*a, **kw):
            ws = real(*a, **kw)
            ws.info[0] = -(2 ** 31)
            return ws
        monkeypatch.setattr(ops, "gpcv_mt_step", internal)
        with pytest.raises(VoltHipError, match="internal error"):
            elbo(model(model.inducing_points), yd)


# ------------------------------------------------------------------------------------------------ start-up and the trainers
def _price_matrix(n, T, seed):
    return torch.stack([torch.tensor(sde_series(n, seed + i)[0]) for i in range(T)])


@pytest.mark.parametrize("tag", ["n60_t3", "n90_t2"])
@pytest.mark.parametrize("param", ["exp", "cv"])
def test_start_up_matches_the_reference_code(tag, param):
    """initialize_variational_parameters on the device against the reference class's own method executed in fp64
    (tests/golden/mt_gpcv_cv.npz): mean and constants 1e-5, covariance 2e-3."""
    import os
    import numpy as np
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import MultitaskVariationalGP
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "mt_gpcv_cv.npz"))
    g = lambda k: torch.tensor(G[f"{tag}_{k}"])
    x, yy = g("x"), g("y")
    N, T = yy.shape
    torch.manual_seed(9)
    model = MultitaskVariationalGP(x.float().to(DEV), T, covar_module=BMKernel())
    lh = VolatilityGaussianLikelihood(K=1, batch_shape=torch.Size([T]), param=param).to(DEV)
    if param == "cv":
        with torch.no_grad():
            for k in C.RAW_KEYS:
                getattr(lh, k).copy_(g(k))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.initialize_variational_parameters(lh, x.float().to(DEV), y=yy.float().to(DEV))
    mean, root, const = g(f"{param}_f64_mean"), g(f"{param}_f64_root"), g(f"{param}_f64_const")
    e_mean = float((model.variational_mean.detach().cpu().double() - mean).abs().max())
    consts = torch.stack([b.constant.detach().cpu().double().reshape(()) for b in model.mean_module.base_means])
    S = model.variational_covar_root.detach().cpu().double()
    cov_h, cov_r = S @ S.T, root @ root.T
    e_cov = float((cov_h - cov_r).abs().max() / cov_r.abs().max())
    print(f"MTCV start-up {tag} {param}: mean {e_mean:.2e} const {float((consts - const).abs().max()):.2e} cov {e_cov:.2e}")
    assert e_mean < 1e-5 and float((consts - const).abs().max()) < 1e-5 and e_cov < 2e-3


def _start(m0, lh0):
    s = {"m": m0.variational_mean, "Lx": m0.variational_covar_root, "Lt": m0.variational_task_covar_root,
         "c": torch.cat([b.constant.reshape(1) for b in m0.mean_module.base_means]),
         "raw_vol": m0.data_kernel.raw_vol, "F": m0.index_kernel.covar_factor, "raw_var": m0.index_kernel.raw_var}
    return {k: v.detach().cpu() for k, v in s.items()}, {k: getattr(lh0, k).detach().cpu() for k in C.RAW_KEYS}


def test_fit_cv_tracks_fp64_adam_eager_and_captured(monkeypatch):
    """60 Adam iterations of FitGPCVMultitask(param="cv", K=1, train_likelihood=True) at (399, 4), eager and graph=True,
    against fp64 Adam on the restatement from the same start: the shapes and bounds of
    tests/test_gpu_mt_gpcv.py::test_fit_tracks_fp64_adam_eager_and_captured.
    Captured equals eager bitwise -- for the same update: graph=True steps with optim.FusedAdam and graph=False with
    torch.optim.Adam (train_utils._adam), two implementations of one formula whose fp32 roundings differ, so the eager run
    of this comparison is a third fit, eager with FusedAdam.  Every parameter and the likelihood's raws must be identical:
    capturing and replaying the "cv" step changes no bit."""
    from volt_amd import train_utils
    from volt_amd.optim import FusedAdam
    from volt_amd.train_utils import FitGPCVMultitask
    n, T, iters = 399, 4, 60
    F = _price_matrix(n, T, 2021)
    x = torch.arange(n, dtype=torch.float32) / 252
    kw = dict(param="cv", K=1, train_likelihood=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(21)
        m0, lh0, _ = FitGPCVMultitask(x.to(DEV), F.to(DEV), train_iters=0, **kw)
        start, raws = _start(m0, lh0)
        torch.manual_seed(21)
        model, lh, losses = FitGPCVMultitask(x.to(DEV), F.to(DEV), train_iters=iters, graph=False, **kw)
        torch.manual_seed(21)
        model_g, lh_g, losses_g = FitGPCVMultitask(x.to(DEV), F.to(DEV), train_iters=iters, graph=True, **kw)
        monkeypatch.setattr(train_utils, "_adam", lambda params, lr, graph: FusedAdam(params, lr=lr))
        torch.manual_seed(21)
        model_e, lh_e, losses_e = FitGPCVMultitask(x.to(DEV), F.to(DEV), train_iters=iters, graph=False, **kw)
        monkeypatch.undo()
    yy = R.scaled_returns(x.double(), F.double())
    want, ps, rs = C.fit(x.double(), yy, start, raws, iters)
    want = torch.tensor(want, dtype=torch.float64)
    got = torch.stack(losses).cpu().double()
    assert got.shape == want.shape
    band = ((got - want).abs() / want.abs().clamp_min(1.0))
    print("MTCV fit: max loss deviation", f"{float(band.max()):.2e}", "first", f"{abs(float(got[0] - want[0])) / abs(float(want[0])):.2e}",
          "loss", float(want[0]), "->", float(want[-1]))
    assert float(band.max()) < 5e-4
    assert abs(float(got[0] - want[0])) < 1e-4 * abs(float(want[0]))
    assert float(want[-1]) < float(want[0])
    last_g = float(losses_g[-1])
    assert abs(last_g - float(want[-1])) < 5e-4 * max(1.0, abs(float(want[-1])))
    assert float((model.variational_mean.detach().cpu().double() - ps["m"]).abs().max()) < 5e-3
    assert not torch.equal(lh.raw_a.detach().cpu(), raws["raw_a"])                  # the likelihood was trained
    assert abs(last_g - float(got[-1])) < 2 * 5e-4 * max(1.0, abs(float(want[-1])))
    assert torch.equal(losses_e[-1], losses_g[-1])
    for (n1, a), (n2, b) in zip(list(model_e.named_parameters()) + list(lh_e.named_parameters()),
                                list(model_g.named_parameters()) + list(lh_g.named_parameters())):
        assert n1 == n2 and torch.equal(a.detach(), b.detach()), n1                 # captured == eager, bitwise


def test_learn_cv_matches_the_restatements_predictive_scale():
    """LearnGPCVMultitask(param="cv") returns the mean over ten joint draws of max(scale_t(F), 1e-3): against the restatement
    at the fitted parameters on the same base draws, to 2e-3."""
    from volt_amd.train_utils import FitGPCVMultitask, LearnGPCVMultitask
    n, T = 200, 3
    F = _price_matrix(n, T, 2023)
    x = torch.arange(n, dtype=torch.float32) / 252
    kw = dict(train_iters=5, param="cv", graph=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(5)
        vol = LearnGPCVMultitask(x.to(DEV), F.to(DEV), **kw)
        torch.manual_seed(5)                             # (the fit draws on the CPU only: the device's generator is where
        model, lh, _ = FitGPCVMultitask(x.to(DEV), F.to(DEV), **kw)                  # LearnGPCVMultitask's rsample found it)
        E = torch.randn(10, n, T, device=DEV)
    p, raws = _start(model, lh)
    want = C.pred_scale({k: v.double() for k, v in p.items()}, E.double().cpu(), {k: v.double() for k, v in raws.items()})
    err = float((vol.double().cpu() - want).abs().max() / want.abs().max())
    print("MTCV learn: predictive scale error", f"{err:.2e}")
    assert tuple(vol.shape) == (T, n) and bool(torch.isfinite(vol).all()) and float(vol.min()) >= 1e-3
    assert err < 2e-3


def test_default_trainers_are_the_exp_loop_bitwise():
    from volt_amd.train_utils import FitGPCVMultitask, LearnGPCVMultitask
    n, T = 129, 3
    F = _price_matrix(n, T, 2025).to(DEV)
    x = (torch.arange(n, dtype=torch.float32) / 252).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        runs = []
        for kw in ({}, dict(param="exp")):
            torch.manual_seed(3)
            model, _, losses = FitGPCVMultitask(x, F, train_iters=5, **kw)
            torch.manual_seed(3)
            runs.append(([q.detach().clone() for q in model.parameters()], torch.stack(losses), LearnGPCVMultitask(x, F, train_iters=5, **kw)))
    (pa, la, va), (pb, lb, vb) = runs
    assert all(torch.equal(a, b) for a, b in zip(pa, pb)) and torch.equal(la, lb) and torch.equal(va, vb)


# ------------------------------------------------------------------------------------------------------- the stocks driver
@pytest.mark.parametrize("opts", [None, {"param": "cv", "K": 1, "train_likelihood": True}], ids=["exp", "cv"])
def test_stocks_driver_takes_its_vol_paths_from_the_joint_model(opts):
    from volt_amd.forecast import GenerateStockPredictionsBatch
    from volt_amd.train_utils import LearnGPCVMultitask
    B, ntrain, H, S, iters = 3, 60, 5, 8, 4
    closes = _price_matrix(ntrain + 1, B, 2027).float().to(DEV)
    debug = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(17)
        samples = GenerateStockPredictionsBatch(["a", "b", "c"], closes, forecast_horizon=H, train_iters=iters, nsample=S,
                                                ntrain=ntrain, k=20, ntimes=1, debug=debug, multitask_gpcv=True,
                                                gpcv_options=opts)
        x = torch.arange(ntrain - 1, device=DEV) * (1. / 252)
        torch.manual_seed(17)
        vol = LearnGPCVMultitask(x, debug["train_y"], train_iters=iters, **(opts or {}))
    assert tuple(samples.shape) == (B, S, H) and bool(torch.isfinite(samples).all())
    assert torch.equal(debug["vol"], vol)
