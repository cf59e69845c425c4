"""volt_gpcv_mt_step_f32 (csrc/gpcv_mt.hip) on the MI355X where tests/test_gpu_mt_gpcv.py does not reach: priors whose
Cholesky factor is not rank-one (so that L^-1 and L^-T are full triangles and every tile of the step's seven GEMMs
carries weight), the floored-variance and clamped-scale branches of the quadrature pass, the edges of the step's own
constants (16 quadrature rows, 64-column partial sums, the 256 -> 1024-thread switch of the task algebra at T = 16 | 17,
T = 64, T > N), and guards: sentinels around every output, a strided K inside NaN, NaN above the diagonals, a NaN-filled
workspace, repeats, the K_t pivot report.

The oracle is the fp64 Kronecker-structured restatement of tests/mt_gpcv_ref.py with the prior passed in (``reference``),
the inputs are its named Cases, and the bounds are tests/test_gpu_mt_gpcv.py's (``ratios``: scalars and F 5e-5 max(1, |ref|),
gradients 2e-3 of the largest reference entry, grad_K 5e-3; clamp cases add grad_Lx and grad_M row by row).
tests/test_mt_gpcv_host.py holds the fp32 CPU evaluation of the restatement to half of each of them at the same inputs.
Every error / bound ratio is printed before it is asserted."""
import math

import pytest
import torch

import mt_gpcv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTPUTS = ("out", "grad_M", "grad_c", "grad_Lx", "grad_Lt", "grad_covar_factor", "grad_raw_var", "grad_K")


def _f(t):
    return t.float().to(DEV)


def _gh(Q=75):
    gx, gw = R.gauss_hermite(Q)
    return _f(gx), _f(gw)


def _run(cs, want_dk=True, w_ell=None):
    """The step at a Case's inputs through ops.gpcv_mt_step, the prior passed in as K."""
    from volt_amd import ops
    c = R.make(cs)
    p, (we, wk) = c["p"], R.weights(cs)
    ws = ops.gpcv_mt_step(_f(c["K"]), _f(p["m"]), _f(p["c"]), _f(p["Lx"]), _f(p["Lt"]), _f(p["F"]), _f(p["raw_var"]), _f(c["y"]),
                          *_gh(cs.Q), want_dk=want_dk, w_ell=we if w_ell is None else w_ell, w_kl=wk)
    torch.cuda.synchronize()
    return ws


def _grads(ws):
    g = {"m": ws.grad_M, "Lx": ws.grad_Lx, "Lt": ws.grad_Lt, "F": ws.grad_covar_factor, "raw_var": ws.grad_raw_var,
         "c": ws.grad_c, "K": ws.grad_K}
    return {k: v.double().cpu() for k, v in g.items()}


def _check(cs, ws):
    """All 13 scalars, the seven gradients (d/d raw_vol on the model's prior) and grad_K against the oracle."""
    assert ws.info.tolist() == [0, 0, 0], (cs, ws.info.tolist())
    g = _grads(ws)
    assert bool(torch.isfinite(ws.out).all()) and [k for k, v in g.items() if not bool(torch.isfinite(v).all())] == [], cs
    r = R.ratios(cs, ws.out.double().cpu()[:13], g)
    print(f"MTK {cs.prior} ({cs.N},{cs.T}) x0={cs.x0} clamp={cs.clamp} Q={cs.Q} error/bound:",
          " ".join(f"{k}={v:.2e}" for k, v in r.items()))
    assert R.over(r) == {}, cs                                                         # item by item: NaN does not pass
    assert float(ws.out[13]) == pytest.approx(R.JITTER) and not ws.out[14:].any()
    assert not ws.grad_Lx.triu(1).any() and not ws.grad_Lt.triu(1).any()              # exactly zero above the diagonals
    return r


# ------------------------------------------------------------------------------------------------------- full-rank priors
@pytest.mark.parametrize("cs", R.GENERIC_CASES, ids=lambda c: f"{c.prior}-{c.N}x{c.T}")
def test_step_matches_oracle_on_generic_priors(cs):
    _check(cs, _run(cs))


@pytest.mark.parametrize("kind", ["rbf", "wishart"])
def test_one_task_equals_the_single_task_step_on_a_generic_prior(kind):
    """tests/test_gpu_mt_gpcv.py's test_one_task_equals_the_single_task_step (same gate: twice the oracle tolerances) on a
    prior whose factor is full: the T = 1 route of V = R'L^-T, A' = V Y' against gpcv_step's own solves."""
    from volt_amd import ops
    N = 399
    p, x, y = R.case(N, 1, seed=7)
    p["F"] = torch.zeros(1, 1, dtype=torch.float64)
    p["raw_var"] = torch.tensor([math.log(math.e - 1)], dtype=torch.float64)
    p["Lt"] = torch.ones(1, 1, dtype=torch.float64)
    K = _f(R.prior(kind, N, seed=N + 1))
    gx, gw = _gh()
    ws = ops.gpcv_mt_step(K, _f(p["m"]), _f(p["c"]), _f(p["Lx"]), _f(p["Lt"]), _f(p["F"]), _f(p["raw_var"]), _f(y), gx, gw,
                          want_dk=True, w_ell=1.0 / N, w_kl=1.0 / N)
    m, c = _f(p["m"][:, 0]).reshape(1, N), _f(p["c"])
    st = ops.gpcv_step(K.unsqueeze(0), m - c, m, _f(p["Lx"]).unsqueeze(0), _f(y[:, 0]).reshape(1, N), gx, gw, want_dk=True,
                       w_ell=1.0 / N, w_kl=1.0 / N)
    torch.cuda.synchronize()
    assert ws.info.tolist() == [0, 0, 0] and int(st.info.abs().sum()) == 0
    F1, F0 = float(ws.out[12]), float(st.out[0, 9])
    d = {"F": abs(F1 - F0) / max(1.0, abs(F0)),
         "grad_M": float((ws.grad_M[:, 0] - st.grad_m[0]).abs().max() / st.grad_m[0].abs().max()),
         "grad_Lx": float((ws.grad_Lx - st.grad_Lq[0]).abs().max() / st.grad_Lq[0].abs().max()),
         "grad_mu": abs(float(ws.grad_c[0]) - float(st.grad_mu[0].sum())) / max(1.0, abs(float(st.grad_mu[0].sum()))),
         "grad_K": float((ws.grad_K - st.grad_K[0]).abs().max() / st.grad_K[0].abs().max())}
    print(f"MTK T = 1 vs ops.gpcv_step on {kind}, largest differences:", {k: f"{v:.2e}" for k, v in d.items()})
    assert d["F"] <= 2 * 5e-5
    assert d["grad_M"] <= 2 * 2e-3 and d["grad_Lx"] <= 2 * 2e-3 and d["grad_mu"] <= 2 * 2e-3 and d["grad_K"] <= 2 * 5e-3


# --------------------------------------------------------------------------------------------------- the floor and the clamp
@pytest.mark.parametrize("cs", R.CLAMP_CASES, ids=lambda c: f"{c.prior}-{c.clamp}-{c.N}x{c.T}")
def test_floored_variances_and_clamped_scales(cs):
    """The ``floored`` (var < min_var) and ``!live`` (exp f <= min_scale) branches of the quadrature pass.  The rows of Lx
    differ by 10^3 .. 10^4 in scale here, so grad_Lx and grad_M are also held row by row (2e-3 of the row's largest
    reference entry; the fp32 CPU restatement stays under 5 % of that, tests/test_mt_gpcv_host.py).  Where the likelihood
    cannot contribute -- a row of Lx floored at every t, an (n, t) clamped at every node -- the gradient is bitwise the one
    of a second run with w_ell = 0, and agrees with the KL-only reference."""
    c = R.make(cs)
    s = R.clamp_stats(c["p"], c["y"])
    print(f"MTK clamp {cs.clamp}: floored {s['floored']:.3f} clamped {s['clamped']:.3f} margins {s['near_scale']} {s['near_var']}")
    assert s["near_scale"] == 0 and s["near_var"] == 0
    assert s["clamped"] > 0.05 and (s["floored"] > 0.05 or cs.clamp == "a")
    if (cs.N, cs.T) == (200, 3):
        assert s["floored"] == pytest.approx(R.CLAMP_SHARES[cs.clamp][0], abs=5e-4)
        assert s["clamped"] == pytest.approx(R.CLAMP_SHARES[cs.clamp][1], abs=5e-4)
    ws = _run(cs)
    _check(cs, ws)
    if cs.clamp == "a":
        return
    rows, nt = s["floored_rows"], s["all_clamped"]
    assert int(rows.sum()) >= cs.N // 3 and int(nt.sum()) > 0
    gLx, gM = ws.grad_Lx.cpu(), ws.grad_M.cpu()
    kl = _run(cs, w_ell=0.0)
    assert bool(torch.isfinite(kl.grad_Lx).all()) and bool(torch.isfinite(kl.grad_M).all())
    assert torch.equal(gLx[rows], kl.grad_Lx.cpu()[rows]) and not torch.equal(gLx[~rows], kl.grad_Lx.cpu()[~rows])
    assert torch.equal(gM[nt], kl.grad_M.cpu()[nt]) and not torch.equal(gM[~nt], kl.grad_M.cpu()[~nt])
    r = R.kl_only_ratios(cs, gLx, gM)
    print(f"MTK clamp {cs.clamp} vs the KL-only reference, error/bound:", " ".join(f"{k}={v:.2e}" for k, v in r.items()))
    assert R.over(r) == {}, cs


# ----------------------------------------------------------------------------------------------------------- edge shapes
@pytest.mark.parametrize("N,T", R.EDGE_SHAPES)
def test_edge_shapes(N, T):
    """N and T around 16 (quadrature rows; the task algebra's 256 | 1024 threads), 64 (partial-sum columns, the largest T)
    and 128 (the tile), T > N included; the model's prior on grids that start at 0 and at 1/252, wishart from N = 15."""
    for cs in R.edge_cases(N, T):
        _check(cs, _run(cs))


@pytest.mark.parametrize("cs", R.Q_CASES, ids=lambda c: f"Q{c.Q}")
def test_node_counts(cs):
    _check(cs, _run(cs))


def test_weights_other_than_the_models():
    """w_ell = 0.37, w_kl = 2.5: out[12] and every gradient are those of w_ell ell - w_kl KL (ell and KL themselves are not
    weighted)."""
    ws = _run(R.W_CASE)
    _check(R.W_CASE, ws)
    o = ws.out.double().cpu()
    assert abs(float(o[12] - (0.37 * o[0] - 2.5 * o[1]))) <= 1e-6 * abs(float(o[12]))


# ----------------------------------------------------------------------------------------------------------------- guards
PAD = 64                                      # words of sentinel before and behind every output


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


def _inputs(N, T, seed=11):
    p, x, y = R.case(N, T, seed=seed)
    gx, gw = _gh()
    return dict(K=_f(R.prior("wishart", N, seed=N + T)), M=_f(p["m"]), c=_f(p["c"]), Lx=_f(p["Lx"]), Lt=_f(p["Lt"]),
                cf=_f(p["F"]).reshape(-1), rv=_f(p["raw_var"]), y=_f(y), gx=gx, gw=gw)


def _workspace(N, T, want_dk, poison=False):
    """Scratch of the test's own, initialised as ops.GpcvMtWorkspace does: zero-filled, or every byte 0xFF (NaN) first."""
    from volt_amd import _lib, ops
    nbytes = _lib.lib().volt_gpcv_mt_workspace_bytes(N, T, int(want_dk))
    buf, ptr = ops._scratch(nbytes, DEV)
    buf.fill_(255 if poison else 0)
    with torch.cuda.device(buf.device):
        _lib.check(_lib.lib().volt_mll_workspace_init_f32(ptr, 1, N, 1, _lib.stream_ptr()), "volt_mll_workspace_init")
    return buf, ptr


def _raw_step(inp, N, T, want_dk, ws=None, poison=False, outs=None):
    """volt_gpcv_mt_step_f32 through the ctypes binding, every output inside sentinels.  Returns ({name: _Guarded}, info)."""
    from volt_amd import _lib
    if ws is None:
        ws = _workspace(N, T, want_dk, poison)
    if outs is None:
        shapes = dict(out=(16,), grad_M=(N, T), grad_c=(T,), grad_Lx=(N, N), grad_Lt=(T, T), grad_covar_factor=(T,),
                      grad_raw_var=(T,), grad_K=(N, N))
        outs = {k: _Guarded(shapes[k]) for k in OUTPUTS if want_dk or k != "grad_K"}
        outs["info"] = _Guarded((3,), torch.int32)
    K = inp["K"]
    assert K.stride(1) == 1 and all(inp[k].is_contiguous() for k in ("M", "c", "Lx", "Lt", "cf", "rv", "y", "gx", "gw"))
    ptr = lambda k: outs[k].t.data_ptr() if k in outs else None
    with torch.cuda.device(torch.device(DEV)):
        _lib.check(_lib.lib().volt_gpcv_mt_step_f32(
            K.data_ptr(), K.stride(0), R.JITTER, inp["M"].data_ptr(), inp["c"].data_ptr(), inp["Lx"].data_ptr(),
            inp["Lt"].data_ptr(), inp["cf"].data_ptr(), inp["rv"].data_ptr(), inp["y"].data_ptr(), inp["gx"].data_ptr(),
            inp["gw"].data_ptr(), inp["gx"].numel(), R.MIN_VAR, R.MIN_SCALE, 1.0 / N, 1.0 / (N * T), *[ptr(k) for k in OUTPUTS],
            ptr("info"), ws[1], N, T, _lib.WS_INITIALISED, _lib.stream_ptr()), "volt_gpcv_mt_step")
    torch.cuda.synchronize()
    return outs, ws


def _same(a, b):
    """Bitwise, output by output (NaN would compare unequal: every output must be finite as well)."""
    bad = [k for k in a if k != "info" and not (torch.equal(a[k].t, b[k].t) and bool(torch.isfinite(a[k].t).all()))]
    return bad


GUARD_SHAPES = [(129, 3), (257, 17), (399, 8)]


@pytest.mark.parametrize("want_dk", [False, True])
@pytest.mark.parametrize("N,T", GUARD_SHAPES)
def test_guards(N, T, want_dk):
    """At inputs of a full-rank prior: (1) nothing is written before or behind any output; (2) K as a view with
    ldk = N + 37 inside NaN, NaN in its strict upper triangle; (3) NaN, not junk, above the diagonals of Lx and Lt; (4) a
    workspace whose every byte was 0xFF (NaN) before volt_mll_workspace_init_f32 -- each bitwise the plain run."""
    inp = _inputs(N, T)
    base, _ = _raw_step(inp, N, T, want_dk)
    assert base["info"].t.tolist() == [0, 0, 0]
    assert set(base) == set(OUTPUTS[:8 if want_dk else 7]) | {"info"}
    assert [k for k, g in base.items() if not g.intact()] == []
    assert all(bool(torch.isfinite(base[k].t).all()) for k in base if k != "info")
    assert not base["grad_Lx"].t.triu(1).any() and not base["grad_Lt"].t.triu(1).any()

    big = torch.full((N, N + 37), float("nan"), device=DEV)
    low = torch.ones(N, N, device=DEV).tril().bool()
    big[:, :N] = torch.where(low, inp["K"], big[:, :N])
    assert big[:, :N].stride(0) == N + 37 and bool(torch.isnan(big[:, :N][~low]).all()) and torch.equal(big[:, :N][low], inp["K"][low])
    got, _ = _raw_step({**inp, "K": big[:, :N]}, N, T, want_dk)
    assert got["info"].t.tolist() == [0, 0, 0] and _same(base, got) == [], "strided K inside NaN"

    nan_above = lambda L: torch.where(torch.ones_like(L).tril().bool(), L, torch.full_like(L, float("nan")))
    got, _ = _raw_step({**inp, "Lx": nan_above(inp["Lx"]), "Lt": nan_above(inp["Lt"])}, N, T, want_dk)
    assert got["info"].t.tolist() == [0, 0, 0] and _same(base, got) == [], "NaN above the diagonals of Lx / Lt"
    assert not got["grad_Lx"].t.triu(1).any() and not got["grad_Lt"].t.triu(1).any()

    got, _ = _raw_step(inp, N, T, want_dk, poison=True)
    assert got["info"].t.tolist() == [0, 0, 0] and _same(base, got) == [], "NaN-filled workspace"
    assert [k for k, g in got.items() if not g.intact()] == []


def test_step_is_bitwise_repeatable_at_an_odd_shape():
    N, T = 257, 17
    inp = _inputs(N, T)
    first, ws = _raw_step(inp, N, T, True)
    keep = {k: g.t.clone() for k, g in first.items()}
    for rep in range(9):
        again, _ = _raw_step(inp, N, T, True, ws=ws, outs=first)
        assert [k for k in keep if not torch.equal(keep[k], again[k].t)] == [], rep
    assert keep["info"].tolist() == [0, 0, 0] and all(bool(torch.isfinite(v).all()) for v in keep.values())


@pytest.mark.parametrize("j", [0, 16, 63])
def test_task_pivot_is_reported_with_its_index(j):
    """K_t = f f' + diag(softplus(raw_var)) with f_j = 0 and softplus(raw_var_j) underflowing to 0: its pivot j is the first
    non-positive one.  info[1] = j + 1, info[0] = 0 (K_x is fine), info[2] = 1.  (A numerical condition the step reports.)"""
    N, T = 33, 64
    inp = _inputs(N, T)
    inp["rv"][j] = -800.0
    inp["cf"][j] = 0.0
    outs, _ = _raw_step(inp, N, T, False)
    assert outs["info"].t.tolist() == [0, j + 1, 1]
    assert [k for k, g in outs.items() if not g.intact()] == []
