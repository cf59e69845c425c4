"""The dense GPCV ELBO step (csrc/gpcv.hip: volt_gpcv_step_f32 / volt_gpcv_cv_step_f32 through ops.gpcv_step / ops.gpcv_cv_step) on
the MI355X at its edges, floors, clamps and unequal weights, against the fp64 oracle -- the cases, inputs, references and the
comparison of tests/gpcv_dense_cases.py, whose conditions and negative controls tests/test_gpcv_dense_cases_host.py checks on
the CPU.  Then what no oracle is needed for: K through a stride, sentinels around every buffer and ten repeats, a workspace
used again (after other inputs, after a failed series), what a failed series leaves behind, and ops.mll_grad_k -- which
shares gpcv_dk_kernel -- at the sizes around its 128 pad and 256-column blocks.

Tolerances are the project's existing ones for this step (tests/test_gpu_gpcv.py, tests/test_gpu_gpcv_cv.py), unchanged:
scalars and F 5e-5 max(1, |ref|); grad_m, grad_Lq and each of grad_a, grad_b, grad_c 2e-3 of the reference's max per series;
sum grad_mu 2e-3 max(1, |ref|); grad_K 5e-3; mll_grad_k 1e-3 of its largest entry.  Exactly zero where the reference is.
Every case prints its largest error / bound per quantity before it asserts.

Measured on the MI355X, largest error / bound over the 93 cases (the printed DENSE lines): scalars and F 0.35 (1 x 2049; 0.16 at
1 x 1025; <= 0.043 in SIZES, 0.029 in KC, 0.022 in QUAD, 0.0065 in KINDS, 0.0062 in WEIGHTS); grad_m 0.020 and grad_Lq 0.017
(both 1 x 2049; <= 0.0055 and <= 0.0015 elsewhere); sum grad_mu 0.0011 (KINDS, clamped); grad_K 0.0080 (1 x 1025; <= 0.0018
elsewhere); grad_a, grad_b, grad_c <= 0.0002.  No case had to be dropped: n = 1 meets every bound (scalars 0.006).  The series
beside a failed one: scalars 0.0059, gradients <= 0.0012.  mll_grad_k: 4.9e-8 (n = 1) to 9.7e-7 (n = 128) of its largest
entry, bound 1e-3.  The whole file takes 5 s."""
import math

import numpy as np
import pytest
import torch

import gpcv_dense_cases as D
import spd_families

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("out", "grad_m", "grad_mu", "grad_Lq", "grad_K", "grad_abc", "info")


def _dev(c, key):
    return torch.stack([s[key].to(torch.float32) for s in D.inputs(c)]).to(DEV)


def device_inputs(c):
    """What the step takes, fp32 on the device: K, resid = m - mu, m, Lq, y, abc (or None), the quadrature table."""
    K, m, Lq, y = (_dev(c, k) for k in ("K", "m", "Lq", "y"))
    mu = torch.stack([s["c"].to(torch.float32).expand(c.n) for s in D.inputs(c)]).to(DEV)
    ghx, ghw = (t.to(torch.float32).to(DEV) for t in D.gauss_hermite(c.Q))
    return dict(K=K, resid=m - mu, m=m, Lq=Lq, y=y, abc=_dev(c, "abc") if c.Kc else None, ghx=ghx, ghw=ghw)


def step(c, d, ws=None, **kw):
    from volt_amd import ops
    we, wk = D.weights(c)
    kw = {**dict(want_dk=c.want_dk, w_ell=we, w_kl=wk), **kw}
    if c.Kc:
        ws = ops.gpcv_cv_step(d["K"], d["resid"], d["m"], d["Lq"], d["y"], d["abc"], d["ghx"], d["ghw"], ws, **kw)
    else:
        ws = ops.gpcv_step(d["K"], d["resid"], d["m"], d["Lq"], d["y"], d["ghx"], d["ghw"], ws, **kw)
    torch.cuda.synchronize()
    return ws


def outputs(ws):
    """Copies of everything the step wrote, by name (None where the workspace has no such output)."""
    return {k: (None if getattr(ws, k) is None else getattr(ws, k).clone()) for k in NAMES}


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in NAMES)


def host(o, series=None):
    pick = (lambda t: t) if series is None else (lambda t: t[series])
    return {k: (None if v is None else pick(v.double().cpu())) for k, v in o.items()}


def no_case(group, n, B, **kw):
    """Inputs of the cases' recipe at a shape of this file's own."""
    return D._case(group, n, B, **kw)


# ------------------------------------------------------------------------------------------------ 1. every case against the oracle
@pytest.mark.parametrize("c", D.ALL_CASES, ids=[D.case_id(c) for c in D.ALL_CASES])
def test_dense_step_matches_the_oracle(c):
    d = device_inputs(c)
    ws = step(c, d)
    assert ws.info.tolist() == [0] * c.B
    got = host(outputs(ws))
    r = D.ratios(got, D.oracle(c))
    print("DENSE", D.case_id(c), D.fmt(r))
    assert D.passes(r), r
    assert float((got["out"][:, 10] - D.JITTER).abs().max()) < 1e-9 and not got["out"][:, 11].any()
    assert not torch.triu(ws.grad_Lq, 1).any()                                     # exactly zero above the diagonal
    if c.weights == "0,1":
        assert torch.equal(ws.grad_m, -ws.grad_mu)
        assert c.Kc == 0 or not ws.grad_abc.any()
    if c.weights == "1,0":
        assert not ws.grad_mu.any() and not ws.grad_K.any()
    if c.kind == "all_clamped":
        # no node is live: the likelihood has a closed form and no gradient -- what is left is the KL's, bit for bit what the
        # step gives without the likelihood (w_ell = 0)
        for b, s in enumerate(D.inputs(c)):
            want = D.all_clamped_ell(s, c)
            assert abs(float(got["out"][b, 0]) - want) <= D.SCALAR_TOL * max(1.0, abs(want)), (b, float(got["out"][b, 0]), want)
        assert torch.equal(ws.grad_m, -ws.grad_mu)
        assert c.Kc == 0 or not ws.grad_abc.any()
        first = outputs(ws)
        kl_only = outputs(step(c, d, w_ell=0.0))
        assert all(torch.equal(first[k], kl_only[k]) for k in ("grad_m", "grad_mu", "grad_Lq", "grad_K"))


# ------------------------------------------------------------------------------------------------ 2. K through a stride
@pytest.mark.parametrize("Kc", [0, 5])
@pytest.mark.parametrize("n,B", [(130, 3), (257, 2)])
def test_k_through_a_stride_gives_the_same_bits(n, B, Kc):
    """variational.py hands the step K.expand(B, n, n) (batch stride 0); a view with ldk > N is legal by the header."""
    c = no_case("STRIDE", n, B, Kc=Kc)
    d = device_inputs(c)
    K0 = d["K"][0].contiguous()
    shared = K0.expand(B, n, n)
    assert shared.stride(0) == 0
    a = outputs(step(c, {**d, "K": shared}))
    b = outputs(step(c, {**d, "K": shared.contiguous()}))
    assert a["info"].tolist() == [0] * B and same_bits(a, b)
    big = torch.full((B, n + 8, n + 8), float("nan"), device=DEV)
    big[:, :n, :n] = d["K"]
    view = big[:, :n, :n]
    assert view.stride(1) == n + 8 and view.stride(0) == (n + 8) ** 2 and view.stride(2) == 1
    a = outputs(step(c, {**d, "K": view}))
    b = outputs(step(c, {**d, "K": view.contiguous()}))
    assert a["info"].tolist() == [0] * B and same_bits(a, b)
    assert bool(torch.isfinite(a["out"]).all())


# ------------------------------------------------------------------------------------------------ 3. sentinels and repeats
PAD = 64                                                                           # 256 bytes of floats / ints


class Guarded:
    """`count` elements inside a NaN- (float) or pattern- (int) filled allocation, PAD elements of it on either side; the
    payload starts at a 256-byte boundary."""
    INT = 0x5A5A5A5A

    def __init__(self, count, dtype=torch.float32):
        fill = float("nan") if dtype == torch.float32 else self.INT
        self.buf = torch.full((count + 3 * PAD,), fill, dtype=dtype, device=DEV)
        self.off = PAD + (-(self.buf.data_ptr() // 4 + PAD)) % PAD
        self.count, self.dtype = count, dtype
        assert self.ptr % 256 == 0 and self.off >= PAD and self.off + count + PAD <= self.buf.numel()

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    @property
    def payload(self):
        return self.buf[self.off:self.off + self.count]

    def guards_intact(self):
        g = torch.cat([self.buf[:self.off], self.buf[self.off + self.count:]])
        return bool(torch.isnan(g).all()) if self.dtype == torch.float32 else bool((g == self.INT).all())


@pytest.mark.parametrize("want_dk", [False, True])
@pytest.mark.parametrize("Kc", [0, 5])
@pytest.mark.parametrize("n,B", [(1, 1), (65, 3), (129, 2)])
def test_sentinels_and_ten_repeats_through_the_c_abi(n, B, Kc, want_dk):
    from volt_amd import _lib
    L = _lib.lib()
    c = no_case("ABI", n, B, Kc=Kc, want_dk=want_dk)
    d = device_inputs(c)
    we, wk = D.weights(c)
    nbytes = int(L.volt_gpcv_cv_workspace_bytes(B, n, int(want_dk), Kc) if Kc else L.volt_gpcv_workspace_bytes(B, n, int(want_dk)))
    assert nbytes > 0 and nbytes % 4 == 0
    g = dict(out=Guarded(B * 12), grad_m=Guarded(B * n), grad_mu=Guarded(B * n), grad_Lq=Guarded(B * n * n),
             grad_K=Guarded(B * n * n) if want_dk else None, grad_abc=Guarded(B * 3 * Kc) if Kc else None,
             info=Guarded(B, torch.int32), ws=Guarded(nbytes // 4))
    st = _lib.stream_ptr()
    _lib.check(L.volt_mll_workspace_init_f32(g["ws"].ptr, B, n, 1, st), "volt_mll_workspace_init")
    p = lambda k: g[k].ptr if g[k] is not None else None
    prior = (d["K"].data_ptr(), n, n * n, float(D.JITTER), d["resid"].data_ptr(), d["m"].data_ptr(), d["Lq"].data_ptr(),
             d["y"].data_ptr())
    quad = (d["ghx"].data_ptr(), d["ghw"].data_ptr(), c.Q, float(D.MIN_VAR), float(D.MIN_SCALE), we, wk)
    grads = (p("out"), p("grad_m"), p("grad_mu"), p("grad_Lq"), p("grad_K"))
    tail = (p("info"), p("ws"), B, n, _lib.WS_INITIALISED, st)
    names = [k for k in ("out", "grad_m", "grad_mu", "grad_Lq", "grad_K", "grad_abc") if g[k] is not None]
    runs = []
    for _ in range(10):
        for k in names:
            g[k].payload.fill_(float("nan"))
        g["info"].payload.fill_(Guarded.INT)
        if Kc:
            _lib.check(L.volt_gpcv_cv_step_f32(*prior, d["abc"].data_ptr(), Kc, *quad, *grads, p("grad_abc"), *tail),
                       "volt_gpcv_cv_step")
        else:
            _lib.check(L.volt_gpcv_step_f32(*prior, *quad, *grads, *tail), "volt_gpcv_step")
        torch.cuda.synchronize()
        runs.append({k: g[k].buf.clone() for k in names + ["info"]})
    for k in names + ["info", "ws"]:
        assert g[k].guards_intact(), k
    assert g["info"].payload.tolist() == [0] * B
    for k in names:
        assert bool(torch.isfinite(g[k].payload).all()), k
        assert all(torch.equal(runs[0][k].view(torch.int32), r[k].view(torch.int32)) for r in runs[1:]), k
    assert all(torch.equal(runs[0]["info"], r["info"]) for r in runs[1:])
    assert not torch.triu(g["grad_Lq"].payload.view(B, n, n), 1).any()
    # and they are the step's results: what ops gives on the same inputs
    ws = step(c, d)
    for k in names:
        assert torch.equal(g[k].payload.view(getattr(ws, k).shape), getattr(ws, k)), k


# ------------------------------------------------------------------------------------------------ 4. a workspace used again
def _not_pd(K):
    K = K.clone()
    K[1].diagonal().sub_(5.0)
    return K


@pytest.mark.parametrize("Kc", [0, 5])
def test_a_workspace_used_again(Kc):
    """One GpcvWorkspace through three different inputs of one shape, a step with a K that is not positive definite, and a
    good input again: after each good step every output is bitwise what a fresh workspace gives."""
    from volt_amd import ops
    cases = [c for c in D.KINDS if c.prior == "bm" and c.Kc == Kc]
    assert [c.kind for c in cases] == ["floored", "clamped", "all_clamped"]
    n, B = cases[0].n, cases[0].B
    ws = ops.GpcvWorkspace(B, n, True, torch.device(DEV), Kc=Kc)
    ds = [device_inputs(c) for c in cases]
    for c, d in zip(cases, ds):
        got = outputs(step(c, d, ws))
        assert got["info"].tolist() == [0] * B
        assert same_bits(got, outputs(step(c, d))), c.kind
    bad = outputs(step(cases[0], {**ds[0], "K": _not_pd(ds[0]["K"])}, ws))
    assert bad["info"][1] > 0 and bad["info"][0] == 0 and bad["info"][2] == 0
    for c, d in ((cases[1], ds[1]), (cases[0], ds[0])):
        got = outputs(step(c, d, ws))
        assert got["info"].tolist() == [0] * B
        assert same_bits(got, outputs(step(c, d))), ("after the failed step", c.kind)


# ------------------------------------------------------------------------------------------------ 5. a failed series
@pytest.mark.parametrize("Kc", [0, 5])
def test_a_failed_series_and_its_neighbours(Kc):
    """K[1] - 5 I is not positive definite.  info[1] is the first failed pivot of the unblocked fp64 Cholesky of
    K[1] + jitter I (tests/pivot_cases.py, the reference of tests/test_pivot_cases_host.py); the series beside it meet the
    oracle's bounds; of the failed series KL and F are not finite, grad_m and grad_mu NaN throughout, and ell -- which does
    not involve K -- is still the oracle's (include/volt_hip.h, volt_gpcv_step_f32)."""
    import pivot_cases
    c = no_case("FAILED", 130, 3, Kc=Kc)
    d = device_inputs(c)
    K = _not_pd(d["K"])
    want, pivot = pivot_cases.first_failed_pivot(K[1].double().cpu().numpy() + float(np.float32(D.JITTER)) * np.eye(c.n))
    assert want >= 1 and pivot < -1.0                                              # far from zero: fp32 fails there too
    ws = step(c, {**d, "K": K})
    assert ws.info.tolist() == [0, want, 0]
    ref = D.oracle(c)
    r = D.ratios(host(outputs(ws), [0, 2]), [ref[0], ref[2]])
    print("DENSE-FAILED neighbours", D.case_id(c), D.fmt(r))
    assert D.passes(r), r
    out = ws.out.double().cpu()
    print("DENSE-FAILED out[1]", out[1].tolist())
    assert bool(torch.isnan(ws.grad_m[1]).all()) and bool(torch.isnan(ws.grad_mu[1]).all())
    assert not math.isfinite(float(out[1, 1])) and not math.isfinite(float(out[1, 9]))
    ell = ref[1]["out"]["ell"]
    assert abs(float(out[1, 0]) - ell) <= D.SCALAR_TOL * max(1.0, abs(ell))
    lds = ref[1]["out"]["logdet_s"]
    assert abs(float(out[1, 4]) - lds) <= D.SCALAR_TOL * max(1.0, abs(lds))


# ------------------------------------------------------------------------------------------------ 6. ops.mll_grad_k
@pytest.mark.parametrize("n", [1, 127, 128, 129, 255, 256, 257])
def test_mll_grad_k_around_the_pad_and_the_column_blocks(n):
    """d mll / d K = 1/2 (alpha alpha' - K_s^-1) / N on "wishart", B = 2, against fp64 LAPACK: 1e-3 of its largest entry
    (tests/test_gpu_dense_generic.py's bound for it)."""
    from volt_amd import ops
    B = 2
    A = spd_families.wishart(B, n, seed=5)
    r = spd_families.rhs(B, n, seed=5)
    ref = spd_families.reference(A, r, keep_y=True)
    K = torch.as_tensor(A, dtype=torch.float32).to(DEV)
    ws = ops.MllWorkspace(B, n, True, K.device)
    _o, alpha, info = ops.mll_step(K, torch.as_tensor(r, dtype=torch.float32).to(DEV), torch.zeros(B, device=DEV), ws)
    assert int(info.abs().sum()) == 0
    want = 0.5 * (ref["alpha"][:, :, None] * ref["alpha"][:, None, :] - ref["Y"] @ np.swapaxes(ref["Y"], -1, -2)) / n
    got = ops.mll_grad_k(ws).double().cpu().numpy()
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print("DENSE-GRADK", n, f"{err:.2e}")
    assert got.shape == (B, n, n) and err <= 1e-3
