"""The Kronecker multi-task step on the MI355X, kernel by kernel (csrc/kron.hip, csrc/kron_chain.hip, csrc/kron_shared.h): both
prologues and all four epilogues through the C ABI with a strided Y, guard bands and bitwise repeats; the warm start from the Q
of a very different S; and the whole step (ops.kron_mll_step, ops.kron_bm_step) in the eigenvalue regimes of
tests/kron_cases.py -- tied, clustered, one dominant direction, noise-dominated (kappa << 1), softplus's linear branch, tiny vol.

References: the dense fp64 definition (test_gpu_multitask.oracle_mll), its fp64 restatement (tests/kron_chain_ref.py; equal to
the oracle to 1e-10 in every regime, tests/test_kron_cases_host.py) and, for fp32, a yardstick -- the restatement with a vendor
fp32 Cholesky per direction in place of the step -- and a floor -- the restatement with nothing but the fp32 rounding of the
step's interface (kron_cases.yardstick / interface_floor).

Gates of the step (section d).  fp64: 1e-9 of max(1, |.|) per quantity.  fp32, per quantity:
max(project bound, 3 x the yardstick's error), project bounds 5e-5 of max(1, |mll|) and 2e-3 of each gradient's max (the 3x is
the convention of tests/test_gpu_lownoise.py).  Measured worst ratios kernel error / gate are in the README's row
"the Kronecker step kernel by kernel" and in test_step_across_regimes' docstring."""
import numpy as np
import pytest
import torch

import kron_cases as kc
import kron_chain_ref as kref
from test_gpu_multitask import make_case, model_params, oracle_mll, oracle_posterior

pytestmark = pytest.mark.gpu

ORDER = ("raw_vol", "covar_factor", "raw_var", "raw_task_noises", "raw_noise")      # the order the C ABI takes the parameters in
DTYPES = pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
NAN = float("nan")


@pytest.fixture(scope="module")
def va():
    assert torch.cuda.is_available()
    import volt_amd
    return volt_amd


def _sfx(dt):
    return "_f32" if dt == torch.float32 else "_f64"


class Guarded:
    """n elements of ``dtype`` on the device between two 256-byte bands of NaN (int32: NaN's bit pattern)."""

    def __init__(self, n, dtype):
        base = torch.float32 if dtype == torch.int32 else dtype
        self.n, self.pad = n, 256 // torch.empty(0, dtype=base).element_size()
        self.raw = torch.full((n + 2 * self.pad,), NAN, dtype=base, device="cuda")
        body = self.raw[self.pad:self.pad + n]
        self.body = body.view(torch.int32) if dtype == torch.int32 else body
        self.ptr = self.body.data_ptr()
        assert self.ptr % 256 == 0

    def intact(self):
        return bool(torch.isnan(self.raw[:self.pad]).all()) and bool(torch.isnan(self.raw[self.pad + self.n:]).all())

    def bits(self):
        """The whole buffer, bands included, as integers: equal bits, NaN or not."""
        return self.raw.view(torch.int32 if self.raw.dtype == torch.float32 else torch.int64).clone()

    def numpy(self):
        return self.body.cpu().numpy().astype(np.float64 if self.body.dtype != torch.int32 else np.int64)


def _device_case(p, x, Y, dt):
    """The parameters 1-D and contiguous in the C ABI's order, x, and Y as columns 2 .. 2 + T of an [N, T + 5] buffer whose
    other columns hold NaN: ldy = T + 5."""
    N, T = Y.shape
    prm = [p[k].to(dt).reshape(-1).contiguous().cuda() for k in ORDER]
    Ybuf = torch.full((N, T + 5), NAN, dtype=dt, device="cuda")
    Ybuf[:, 2:2 + T] = Y.to(dt).cuda()
    return prm, x.to(dt).contiguous().cuda(), Ybuf


class _PrologueBuffers:
    def __init__(self, N, T, dt):
        from volt_amd import _lib
        self.N, self.T, self.dt = N, T, dt
        self.resid, self.sigma2 = Guarded(T * N, dt), Guarded(T, dt)
        self.state = Guarded(int(_lib.lib().volt_kron_state_bytes(T)) // 8, torch.float64)
        self.info = Guarded(1, torch.int32)
        self.all = (self.resid, self.sigma2, self.state, self.info)

    def reset(self, state_fill=0.0):
        self.resid.body.fill_(NAN)
        self.sigma2.body.fill_(NAN)
        self.state.body.fill_(state_fill)                      # no stamp: the warm entry starts cold
        self.info.body.fill_(-99)

    def call(self, warm, prm, xc, Ybuf):
        from volt_amd import _lib
        N, T = self.N, self.T
        fn = getattr(_lib.lib(), "volt_kron_prologue" + ("_warm" if warm else "") + _sfx(self.dt))
        Yv = Ybuf[:, 2:2 + T]
        assert tuple(Ybuf.shape) == (N, T + 5) and Ybuf.stride(0) == T + 5 and xc.numel() == N
        _lib.check(fn(*(t.data_ptr() for t in prm), xc.data_ptr(), Yv.data_ptr(), Ybuf.stride(0), self.resid.ptr, self.sigma2.ptr,
                      self.state.ptr, self.info.ptr, N, T, _lib.stream_ptr()), "volt_kron_prologue")

    def bits(self):
        return [g.bits() for g in self.all]

    def intact(self):
        return all(g.intact() for g in self.all)


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def _split_state(state, T):
    """vol, lambda [T], d [T], W [T,T], Q [T,T] of the prologue's state (include/volt_hip.h)."""
    return (float(state[0]), state[8:8 + T], state[8 + T:8 + 2 * T], state[8 + 2 * T:8 + 2 * T + T * T].reshape(T, T),
            state[8 + 2 * T + T * T:8 + 2 * T + 2 * T * T].reshape(T, T))


def _check_prologue(dt, pro, want_R, resid, sigma2, state, info, what):
    """Section (a)'s checks on one prologue result (numpy, fp64 views of the kernels' outputs; resid [T,N]).
      vol, d: 1e-14 relative to prologue_ref -- both sides are chains of at most one exp, one log1p and three roundings in fp64,
          each within 2 ulp (the device library's documented bounds): 8 ulp = 1.8e-15, gated at 1e-14;
      lam, Q: kron_cases.eig_checks against the host's fp64 S (relative to |S|; no entrywise comparison with eigh);
      W == Q / sqrt(d) and sigma2 == 1 / (vol lam) rounded to the type: the same correctly rounded IEEE operations on both sides;
      reconstruct_R against Y - mu: 1e-12 of max(1, max |R|) in fp64.  fp32: resid_j is the fp64 value rounded once, relative
          error u = 2^-24, and R[n,t] = sum_j resid_j[n] sqrt(kappa_j) Q[t,j] sqrt(d_t) is linear in resid, so
          |dR[n,t]| <= u sum_j |resid_j[n]| sqrt(kappa_j) |Q[t,j]| sqrt(d_t) = u (|Z| |Q|')[n,t] sqrt(d_t), Z = resid' diag(sqrt(kappa)),
          entry by entry, on top of the fp64 term (which also covers taking |Z| from the rounded resid: u^2)."""
    T = pro["lam"].shape[0]
    vol, lam, d, W, Q = _split_state(state, T)
    assert int(info[0]) >= 0, (what, info)
    assert abs(vol - pro["vol"]) <= 1e-14 * pro["vol"], (what, vol, pro["vol"])
    assert (np.abs(d - pro["d"]) <= 1e-14 * pro["d"]).all(), (what, d, pro["d"])
    kc.eig_checks(pro["S"], lam, Q)
    assert np.array_equal(W, Q / np.sqrt(d)[:, None]), what
    s2 = 1.0 / (vol * lam)
    assert np.array_equal(sigma2, s2.astype(np.float32).astype(np.float64) if dt == torch.float32 else s2), (what, sigma2, s2)
    got = kc.reconstruct_R(resid, lam, vol, Q, d)
    bound = 1e-12 * max(1.0, np.abs(want_R).max()) * np.ones_like(want_R)
    if dt == torch.float32:
        Z = np.abs(resid.T) * np.sqrt(vol * lam)[None, :]
        bound = bound + kc.U32 * (Z @ np.abs(Q).T) * np.sqrt(d)[None, :]
    err = np.abs(got - want_R)
    assert (err <= bound).all(), (what, float((err / bound).max()))
    return float((err / bound).max())


# ------------------------------------------------------------------ a. the prologues through the C ABI
PRO_SHAPES = [(N, T) for T in (1, 2, 3, 31, 32, 33, 63, 64) for N in (1, 63, 64, 65)]
# kron_prologue_kernel: 64 workgroups x 64 rows, a second pass from N = 4097; kron_rows_kernel: 256 x 64, from N = 16385
PRO_SHAPES += [(4097, 2), (4161, 33), (16385, 3), (16449, 64)]
PRO_CASES = [("base", N, T) for N, T in PRO_SHAPES]
PRO_CASES += [(name, 65, T) for name in ("scalar", "clusters", "correlated") for T in (3, 33, 64)]


@DTYPES
@pytest.mark.parametrize("name,N,T", PRO_CASES)
def test_prologues_through_the_c_abi(va, name, N, T, dt):
    """volt_kron_prologue_* and volt_kron_prologue_warm_* (cold, then warm from its own Q) on Y with ldy = T + 5, between guard
    bands, ten times each: bitwise equal runs, intact bands, and _check_prologue on every result.  The warm entry's cold call
    is the one-launch prologue's result bit for bit."""
    p, x, Y = kc.case(name, N, T, N % 2, dt)                    # odd N on the grid from dt, even N from 0
    pn, xn, Yn = kc.as_numpy(p), x.double().numpy(), Y.double().numpy()
    pro, want_R = kref.prologue_ref(pn, xn, Yn), kc.residual_of(pn, xn, Yn)
    prm, xc, Ybuf = _device_case(p, x, Y, dt)
    b = _PrologueBuffers(N, T, dt)
    view = lambda: (b.resid.numpy().reshape(T, N), b.sigma2.numpy(), b.state.numpy(), b.info.numpy())

    runs = []
    for _ in range(10):
        b.reset()
        b.call(False, prm, xc, Ybuf)
        runs.append(b.bits())
    assert all(_same(runs[0], r) for r in runs[1:]), "the one-launch prologue is not bitwise repeatable"
    assert b.intact()
    _check_prologue(dt, pro, want_R, *view(), "one launch")
    cold_bits, cold_state = runs[0], b.state.numpy()

    first, second = [], []
    for _ in range(10):
        b.reset()
        b.call(True, prm, xc, Ybuf)
        first.append(b.bits())
        b.call(True, prm, xc, Ybuf)
        second.append(b.bits())
    assert all(_same(first[0], r) for r in first[1:]) and all(_same(second[0], r) for r in second[1:])
    assert b.intact()
    ratio = _check_prologue(dt, pro, want_R, *view(), "warm")
    assert float(b.state.body[2]) == 1.0 or T == 1, "the second call did not start warm"
    # the first (cold) call against the one-launch prologue: resid, sigma2, info, and the state apart from its stamp words
    assert torch.equal(first[0][0], cold_bits[0]) and torch.equal(first[0][1], cold_bits[1]) and torch.equal(first[0][3], cold_bits[3])
    st = first[0][2][b.state.pad:b.state.pad + b.state.n].view(torch.float64).cpu().numpy()
    assert st[0] == cold_state[0] and st[2] == 0.0 and np.array_equal(st[8:], cold_state[8:])
    print(f"prologue {name} {N} x {T} {_sfx(dt)}: sweeps {int(b.info.body[0])} (warm), worst |R - (Y - mu)| / bound = {ratio:.2f}")


# ------------------------------------------------------------------ b. warm start far from home
@DTYPES
@pytest.mark.parametrize("T", [3, 33, 64])
def test_warm_start_far_from_home(va, T, dt):
    """One workspace through base -> correlated -> scalar -> clusters -> base, twice: every call after the first starts from the
    Q of a different regime's S, and must end where a cold workspace ends."""
    from volt_amd import ops
    N = 65
    dev = torch.device("cuda")
    ws = ops.KronWorkspace(N, T, dev, dt, "linear")
    for i, name in enumerate(("base", "correlated", "scalar", "clusters", "base") * 2):
        p, x, Y = kc.case(name, N, T, 1, dt)
        pn, xn, Yn = kc.as_numpy(p), x.double().numpy(), Y.double().numpy()
        pro, want_R = kref.prologue_ref(pn, xn, Yn), kc.residual_of(pn, xn, Yn)
        prm, xc, Yc = tuple(p[k].cuda() for k in ORDER), x.cuda(), Y.cuda()
        cold = ops.KronWorkspace(N, T, dev, dt, "linear")
        ops.kron_prologue(prm, xc, Yc, ws, warm=True)
        ops.kron_prologue(prm, xc, Yc, cold)
        what = f"call {i} ({name})"
        assert float(ws.state[2]) == (1.0 if i else 0.0), what
        assert int(ws.eig_info) >= 0 and int(cold.eig_info) >= 0, what
        for w in (ws, cold):
            _check_prologue(dt, pro, want_R, w.resid.cpu().double().numpy(), w.sigma2.cpu().double().numpy(), w.state.cpu().numpy(),
                            w.eig_info.cpu().numpy(), what)
        gap = float((ws.lam() - cold.lam()).abs().max())
        assert gap <= 1e-12 * np.linalg.norm(pro["S"]), (what, gap)
        print(f"warm {what} T = {T} {_sfx(dt)}: sweeps warm {int(ws.eig_info)} cold {int(cold.eig_info)}, |lam - cold| / |S| = "
              f"{gap / np.linalg.norm(pro['S']):.1e}")


# ------------------------------------------------------------------ c. all four epilogues on the same inputs
EPI_CASES = [(N, T) for T in (2, 31, 32, 33, 45, 63, 64) for N in (1, 31, 33, 257, 513)]


def _gate_groups(got, want, T, bound, what):
    """|got - want| <= bound(want_group) entry by entry, per quantity (MLL, each of the five gradients)."""
    groups = {"mll": (got[:1], want[:1])}
    g, w = kref.unpack(got, T), kref.unpack(want, T)
    groups.update({k: (g[k].reshape(-1), w[k].reshape(-1)) for k in kref.NAMES})
    for k, (a, b) in groups.items():
        assert (np.abs(a - b) <= bound(b)).all(), (what, k, a, b)


@DTYPES
@pytest.mark.parametrize("N,T", EPI_CASES)
def test_all_four_epilogues_on_the_same_inputs(va, N, T, dt):
    """volt_kron_epilogue_* (one workgroup) and volt_kron_epilogue_ws_* (split) on the resid / out / alpha / state the prologue
    and the chain step left, res and the split's workspace between guard bands.  T in 33 .. 63 fills the threads' later
    accumulator slots partly (T = 33 .. 45: slot 1), T = 63 has the Jacobi dummy index, T = 2 and 32 are the edges below.
    Against kref.epilogue_ref on the kernels' own inputs:
      fp64: 1e-9 of max(1, max |quantity|), the bound of test_split_epilogue_vs_one_workgroup;
      fp32: the kernels convert their fp32 inputs exactly and compute in fp64, so res is the fp64 result rounded ONCE:
            u |want| entry by entry, u = 2^-24, on top of the fp64 bound.
    Against the dense oracle where N T <= 4096: the step's gates (module docstring)."""
    from volt_amd import _lib, ops
    L, st = _lib.lib(), _lib.stream_ptr()
    with_oracle = N * T <= 4096
    if with_oracle:
        r = kc.references("base", N, T, 1, dt)
        p, x, Y = r["p"], r["x"], r["Y"]
    else:
        p, x, Y = kc.case("base", N, T, 1, dt)
    pn, xn = kc.as_numpy(p), x.double().numpy()
    prm, xc, Yc = tuple(p[k].cuda() for k in ORDER), x.cuda(), Y.cuda()
    ws = ops.KronWorkspace(N, T, torch.device("cuda"), dt, "linear")
    ops.kron_prologue(prm, xc, Yc, ws)
    out, alpha, info = ops.bm_step(xc, ws.ones, ws.sigma2, ws.resid, ws.bm, want_grad=True)
    assert not info.any() and out.dtype == dt and alpha.dtype == dt
    nres = 3 + 3 * T
    nws = int(L.volt_kron_epilogue_workspace_bytes(N, T)) // 8
    assert nws >= ((N + 255) // 256) * (2 * T * T + T)
    flat = [t.reshape(-1).contiguous() for t in prm]
    head = (*(t.data_ptr() for t in flat), xc.data_ptr(), ws.resid.data_ptr(), out.data_ptr(), alpha.data_ptr(), ws.state.data_ptr())
    res = {"whole": Guarded(nres, dt), "split": Guarded(nres, dt)}
    wbuf = Guarded(nws, torch.float64)
    _lib.check(getattr(L, "volt_kron_epilogue" + _sfx(dt))(*head, res["whole"].ptr, N, T, st), "volt_kron_epilogue")
    _lib.check(getattr(L, "volt_kron_epilogue_ws" + _sfx(dt))(*head, res["split"].ptr, wbuf.ptr, N, T, st), "volt_kron_epilogue_ws")
    assert all(g.intact() for g in (*res.values(), wbuf))
    got = {k: g.numpy() for k, g in res.items()}
    assert all(np.isfinite(v).all() for v in got.values())

    vol, lam, d, W, Q = _split_state(ws.state.cpu().numpy(), T)
    pro = dict(vol=vol, lam=lam, d=d, W=W, kappa=vol * lam, resid=ws.resid.cpu().double().numpy())
    want = kref.epilogue_ref(pn, xn, pro, out.cpu().double().numpy(), alpha.cpu().double().numpy())
    u = kc.U32 if dt == torch.float32 else 0.0
    for k, v in got.items():
        _gate_groups(v, want, T, lambda b: u * np.abs(b) + 1e-9 * max(1.0, np.abs(b).max()), f"{k} vs restatement")
    print(f"epilogues {N} x {T} {_sfx(dt)}: max |split - whole| = {np.abs(got['split'] - got['whole']).max():.2e}, max |whole - "
          f"restatement| = {np.abs(got['whole'] - want).max():.2e} (max |res| = {np.abs(want).max():.2e})")
    if with_oracle:
        for k, v in got.items():
            errs = kc.rel_errors(v[0], kref.unpack(v, T), *r["oracle"], floor_one=dt == torch.float64)
            bad = {q: e for q, e in errs.items() if e > _step_gate(r, q, dt)}
            assert not bad, (k, "vs dense oracle", bad)


# ------------------------------------------------------------------ d. the step across regimes
def _step_gate(r, q, dt):
    return 1e-9 if dt == torch.float64 else max(kc.F32_BOUND[q], 3.0 * r["yard"][q])


@pytest.fixture(scope="module")
def table():
    """{(dtype, regime, solver, quantity): worst (kernel error, yardstick error, floor, error / gate)} over shapes and starts,
    printed when the module is done."""
    rows = {}
    yield rows
    for sfx in ("_f32", "_f64"):
        if not any(k[0] == sfx for k in rows):
            continue
        print(f"\nKronecker step across regimes, {sfx[1:]}: worst over {kc.SHAPES} x two grid starts, relative errors against the "
              "dense fp64 oracle")
        print("  %-14s %-7s %-16s %10s %10s %10s %8s" % ("regime", "solver", "quantity", "kernel", "yardstick", "floor", "err/gate"))
        for name in kc.REGIMES:
            for solver in ("dense", "linear"):
                for q in kc.QUANTITIES:
                    if (sfx, name, solver, q) in rows:
                        print("  %-14s %-7s %-16s %10.2e %10.2e %10.2e %8.3f" % (name, solver, q, *rows[(sfx, name, solver, q)]))


# (N = 1 on the grid from 0 is left out of the fp32 cases of the step, as FP32_CASES does: SHAPES holds no N = 1)
STEP_CASES = [(name, N, T, start) for name in kc.REGIMES for N, T in kc.SHAPES for start in (0, 1)]


@DTYPES
@pytest.mark.parametrize("name,N,T,start", STEP_CASES)
def test_step_across_regimes(va, table, name, N, T, start, dt):
    """ops.kron_mll_step (dense) and ops.kron_bm_step (linear) against the dense fp64 oracle on the same (rounded) inputs; gates
    in the module docstring, the scale max(1, .) where the oracle's gradient is exactly zero.  One row per solver is printed:
    kernel error, yardstick error and floor per quantity.

    Measured on an MI355X, worst kernel error / gate over shapes and starts (the README's row "the Kronecker step kernel by
    kernel" has the figures behind them):
        fp32  noisy       raw_var 0.048 dense (9.7e-5; yardstick 6.3e-4, floor 3.1e-5), 0.032 linear; covar_factor 0.044 / 0.024;
                          raw_vol 0.016 / 0.018 -- the cancellation in N - tau and a'r - a'a / kappa, 1/20 of the bound
              correlated  covar_factor 0.006 dense (1.3e-5), 0.001 linear; mll 0.005 dense (2.4e-7)
              the rest    <= 0.003 (mll 1.5e-7 at most)
        fp64  <= 0.008 (7.7e-12: covar_factor, noisy, linear); dense <= 4.6e-13 (raw_var, linear_branch)"""
    from volt_amd import ops
    r = kc.references(name, N, T, start, dt)
    p, x, Y = r["p"], r["x"], r["Y"]
    prm, xc, Yc = tuple(p[k].cuda() for k in ORDER), x.cuda(), Y.cuda()
    sfx, f64 = _sfx(dt), dt == torch.float64
    bad = {}
    for solver in ("dense", "linear"):
        if solver == "dense":
            res, info, einfo, _ = ops.kron_mll_step(prm, xc, Yc, torch.minimum(xc[:, None], xc[None, :]))
        else:
            res, info, einfo, _ = ops.kron_bm_step(prm, xc, Yc)
        assert res.dtype == dt and not info.any() and int(einfo) >= 0, (solver, info, einfo)
        res = res.cpu().double().numpy()
        errs = kc.rel_errors(res[0], kref.unpack(res, T), *r["oracle"], floor_one=f64)
        cells = []
        for q in kc.QUANTITIES:
            gate = _step_gate(r, q, dt)
            yard, floor = (0.0, 0.0) if f64 else (r["yard"][q], r["floor"][q])
            key = (sfx, name, solver, q)
            if key not in table or errs[q] / gate > table[key][3]:
                table[key] = (errs[q], yard, floor, errs[q] / gate)
            cells.append(f"{q} {errs[q]:.1e}" + ("" if f64 else f"/{yard:.1e}/{floor:.1e}"))
            if errs[q] > gate:
                bad[(solver, q)] = (errs[q], gate)
        print(f"step {name} {N} x {T} start {start} {sfx} {solver}: " + ("" if f64 else "(kernel/yardstick/floor) ") + "  ".join(cells))
    assert not bad, bad


# ------------------------------------------------------------------ e. the dense path's errors
def _mll_of(p, x, Y, solver):
    from test_gpu_multitask_linear import build
    from volt_amd.gp import ExactMarginalLogLikelihood
    m, lh = build(p, x, Y, solver)
    return ExactMarginalLogLikelihood(lh, m)(m(m.train_inputs[0]), m.train_targets)


@DTYPES
@pytest.mark.parametrize("which", ORDER)
def test_dense_nan_parameter_raises_nan_error(va, which, dt):
    """test_gpu_multitask_linear.test_nan_parameter_raises_nan_error on solver="dense", a NaN in each parameter in turn."""
    from volt_amd.gp import NanError, NotPSDError
    p, x, Y = make_case(120, 3, 1, seed=2, dtype=dt)
    p[which].reshape(-1)[-1] = NAN
    with pytest.raises(NanError) as err:
        _mll_of(p, x, Y, "dense")
    assert not isinstance(err.value, NotPSDError)


@pytest.mark.parametrize("warm", [False, True], ids=["one_launch", "warm"])
@pytest.mark.parametrize("which", ORDER)
@pytest.mark.parametrize("T", [3, 33])
def test_prologues_rank_nan_eigenvalues_last(va, T, which, warm):
    """A NaN parameter through both prologue entries, the state pre-filled with -7: every slot of lambda and Q is written (a
    sort by comparisons alone ranks every NaN 0 and leaves the top slots unwritten), the numbers ascend below the NaNs, sigma2
    carries a NaN (the step's info then reports it), the warm entry leaves no stamp, and ten runs are bitwise equal."""
    N, dt = 65, torch.float64
    p, x, Y = kc.case("base", N, T, 1, dt)
    p[which].reshape(-1)[-1] = NAN
    prm, xc, Ybuf = _device_case(p, x, Y, dt)
    b = _PrologueBuffers(N, T, dt)
    runs = []
    for _ in range(10):
        b.reset(state_fill=-7.0)
        b.call(warm, prm, xc, Ybuf)
        runs.append(b.bits())
    assert all(_same(runs[0], r) for r in runs[1:]) and b.intact()
    state, sigma2 = b.state.numpy(), b.sigma2.numpy()
    assert not (state[8:] == -7.0).any(), "slots of the state left unwritten"
    lam = state[8:8 + T]
    nfin = int(np.isfinite(lam).sum())
    assert np.isfinite(lam[:nfin]).all() and (np.diff(lam[:nfin]) >= 0).all() and np.isnan(lam[nfin:]).all(), lam
    if which == "raw_vol":                                      # S does not depend on vol: a sound decomposition, every kappa NaN
        assert nfin == T and np.isnan(sigma2).all(), (lam, sigma2)
        return
    assert nfin < T and np.isnan(sigma2[nfin:]).all(), (lam, sigma2)
    if warm:
        assert state[1] == 0.0 and np.isnan(sigma2).all()


@DTYPES
@pytest.mark.parametrize("solver", ["dense", "linear"])
@pytest.mark.parametrize("start", [0, 1])
def test_vanishing_noise_has_a_defined_outcome(va, start, solver, dt):
    """raw_noise = raw_task_noises = -800 (softplus underflows to 0: d sits on its 2e-4 floor) with covar_factor = 100
    (lambda_max ~ 1.5e8, sigma^2 ~ 2e-8 in that direction): the MLL within the step's gate of the dense oracle, or
    NotPSDError / NanError from _KronMLL -- never a finite wrong value."""
    from volt_amd.gp import NanError, NotPSDError
    N, T = 65, 3
    p, x, Y = make_case(N, T, start, seed=100 * T + N + start, dtype=dt)
    p["raw_noise"].fill_(-800.0)
    p["raw_task_noises"].fill_(-800.0)
    p["covar_factor"].fill_(100.0)
    ref, _ = oracle_mll(p, x.double(), Y.double())
    assert np.isfinite(ref)
    gate = 1e-9
    if dt == torch.float32:
        pn, xn, Yn = kc.as_numpy(p), x.double().numpy(), Y.double().numpy()
        yard = abs(kc.yardstick(pn, xn, Yn)[0] - ref) / max(1.0, abs(ref))
        gate = max(kc.F32_BOUND["mll"], 3.0 * yard)
    try:
        out = float(_mll_of(p, x, Y, solver))
    except (NotPSDError, NanError) as e:
        print(f"vanishing noise start {start} {solver} {_sfx(dt)}: {type(e).__name__}: {e}")
        return
    err = abs(out - ref) / max(1.0, abs(ref))
    print(f"vanishing noise start {start} {solver} {_sfx(dt)}: mll {out:.9g}, oracle {ref:.9g}, error {err:.2e} (gate {gate:.2e})")
    assert err <= gate, (out, ref)


# ------------------------------------------------------------------ the posterior at more task counts
@pytest.mark.parametrize("route", ["dense", "linear", "sweep"])
@pytest.mark.parametrize("T", [1, 2, 33, 64])
def test_posterior_vs_dense_oracle_at_more_task_counts(va, T, route):
    """test_gpu_multitask.test_posterior_vs_dense_oracle's checks and 2e-4 bounds at T in {1, 2, 33, 64} (it covers 3 and 8),
    N = 40, H = 5, on the dense model, the linear model and the linear model's one-sweep posterior."""
    from volt_amd.gp import MultitaskGaussianLikelihood
    from volt_amd.models import MultitaskBMGP
    N, H = 40, 5
    p, x, Y = make_case(N, T, 1, seed=N + T + H)
    lh = MultitaskGaussianLikelihood(num_tasks=T).cuda()
    kw = {} if route == "dense" else dict(solver="linear", posterior="sweep" if route == "sweep" else "solve")
    m = MultitaskBMGP(x.cuda(), Y.cuda(), lh, **kw).cuda()
    with torch.no_grad():
        for k, prm in model_params(m, lh).items():
            prm.copy_(p[k])
    m.eval()
    xs = x[-1] + (torch.arange(H, dtype=torch.float32) + 1) / 252.
    post = m(xs.cuda())
    mref, cref = oracle_posterior(p, x.double(), Y.double(), xs.double())
    mean = post.mean.detach().cpu().double()
    assert tuple(mean.shape) == (H, T)
    cmax = float(cref.abs().max())
    assert float((mean - mref).abs().max()) <= 2e-4 * max(1.0, float(mref.abs().max()))
    cov = post.covariance_matrix.cpu().double()
    assert float((cov - cref).abs().max()) <= 2e-4 * cmax
    var = post.variance.cpu().double()
    assert float((var.reshape(-1) - torch.diagonal(cref)).abs().max()) <= 2e-4 * cmax
    V, Lb = post.root_blocks()
    V, Lb = V.cpu().double(), Lb.cpu().double()
    R = torch.einsum("tj,jhk->htkj", V, Lb).reshape(H * T, H * T)
    assert float((R @ R.T - cref).abs().max()) <= 2e-4 * cmax
    z = torch.randn(H, T, generator=torch.Generator().manual_seed(H))
    s = post.sample(base_samples=z.cuda()).cpu().double()
    want = mean.reshape(-1) + R @ z.double().reshape(-1)
    assert float((s.reshape(-1) - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    assert tuple(post.sample(torch.Size((4,))).shape) == (4, H, T)
