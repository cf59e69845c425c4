"""MultitaskBMGP(solver="linear") on the MI355X: the warm-started eigensolver, the epilogue with its N-reductions
spread over workgroups, the MLL and its five gradients, the posterior, the trainer, the opt-in on the batched models and the
drivers, the errors and the memory -- against the dense fp64 definition of tests/test_gpu_multitask.py (its oracle and helpers
are imported, not copied) and the fp64 restatement of tests/kron_chain_ref.py."""
import warnings

import numpy as np
import pytest
import torch

import kron_chain_ref as kref
from test_gpu_multitask import CASES, _cpu_adam_oracle, make_case, model_params, oracle_mll, oracle_posterior
from volt_amd.synthetic import sde_batch

pytestmark = pytest.mark.gpu

ORDER = ("raw_vol", "covar_factor", "raw_var", "raw_task_noises", "raw_noise")      # the order ops.kron_* take the parameters in


@pytest.fixture(scope="module")
def va():
    assert torch.cuda.is_available()
    import volt_amd
    return volt_amd


def build(p, x, Y, solver="linear"):
    """test_gpu_multitask.build_model with the solver argument it does not have."""
    from volt_amd.gp import MultitaskGaussianLikelihood
    from volt_amd.models import MultitaskBMGP
    lh = MultitaskGaussianLikelihood(num_tasks=Y.shape[1]).cuda()
    m = MultitaskBMGP(x.cuda(), Y.cuda(), lh, solver=solver).cuda()
    if x.dtype == torch.float64:
        m, lh = m.double(), lh.double()
        m.likelihood = lh
    with torch.no_grad():
        for k, prm in model_params(m, lh).items():
            prm.copy_(p[k])
    return m, lh


def params_of(p):
    return tuple(p[k].cuda() for k in ORDER)


# ------------------------------------------------------------------ 1. the warm-started eigensolver
def _eig_checks(S, lam, Q):
    """The bounds of test_gpu_multitask.test_syev_small_eigenpairs, S rebuilt in fp64 on the host."""
    T = S.shape[0]
    nS = np.linalg.norm(S)
    assert np.linalg.norm(S @ Q - Q * lam) <= 1e-12 * nS
    assert np.linalg.norm(Q.T @ Q - np.eye(T)) <= 1e-12
    ref = np.linalg.eigvalsh(S)
    assert np.abs(lam - ref).max() <= 1e-12 * np.abs(ref).max()
    assert (np.diff(lam) >= 0).all()


def _host_s(p):
    return kref.prologue_ref({k: v.numpy() for k, v in p.items()}, np.zeros(1), np.zeros((1, p["raw_var"].numel())))["S"]


def _walk(p, g, step=1e-3):
    return {k: v + step * torch.randn(v.shape, generator=g, dtype=v.dtype) for k, v in p.items()}


@pytest.mark.parametrize("T", [1, 2, 3, 8, 31, 64])
def test_warm_prologue_cold_start_and_drift(va, T):
    from volt_amd import ops
    N = 64
    p, x, Y = make_case(N, T, 1, seed=40 + T, dtype=torch.float64)
    xc, Yc = x.cuda(), Y.cuda()
    ws = ops.KronWorkspace(N, T, torch.device("cuda"), torch.float64, "linear")
    cold = ops.KronWorkspace(N, T, torch.device("cuda"), torch.float64, "linear")
    ops.kron_prologue(params_of(p), xc, Yc, ws, warm=True)                 # a fresh workspace starts cold ...
    ops.kron_prologue(params_of(p), xc, Yc, cold)
    assert float(ws.state[2]) == 0.0 and int(ws.eig_info) >= 0
    assert torch.equal(ws.lam(), cold.lam()) and torch.equal(ws.Q(), cold.Q())     # ... and is the one-launch prologue's
    assert torch.equal(ws.resid, cold.resid) and torch.equal(ws.sigma2, cold.sigma2) and torch.equal(ws.eig_info, cold.eig_info)
    _eig_checks(_host_s(p), ws.lam().cpu().numpy(), ws.Q().cpu().numpy())
    g = torch.Generator().manual_seed(T)
    for _ in range(300):                                                   # a training run's worth of small moves
        p = _walk(p, g)
        ops.kron_prologue(params_of(p), xc, Yc, ws, warm=True)
    assert float(ws.state[2]) == 1.0 or T == 1, "the last call did not start warm"
    assert int(ws.eig_info) >= 0
    _eig_checks(_host_s(p), ws.lam().cpu().numpy(), ws.Q().cpu().numpy())


@pytest.mark.parametrize("T", [8, 64])
def test_warm_start_takes_fewer_sweeps(va, T):
    """The reason volt_kron_prologue_warm_* exists."""
    from volt_amd import ops
    N = 64
    p, x, Y = make_case(N, T, 1, seed=7 * T, dtype=torch.float64)
    xc, Yc = x.cuda(), Y.cuda()
    ws = ops.KronWorkspace(N, T, torch.device("cuda"), torch.float64, "linear")
    cold = ops.KronWorkspace(N, T, torch.device("cuda"), torch.float64, "linear")
    ops.kron_prologue(params_of(p), xc, Yc, ws, warm=True)
    p1 = _walk(p, torch.Generator().manual_seed(1))
    ops.kron_prologue(params_of(p1), xc, Yc, ws, warm=True)
    ops.kron_prologue(params_of(p1), xc, Yc, cold, warm=True)             # a fresh workspace: cold, on the same parameters
    n_warm, n_cold = int(ws.eig_info), int(cold.eig_info)
    print(f"T = {T}: sweeps warm {n_warm}, cold {n_cold}")
    assert float(ws.state[2]) == 1.0 and float(cold.state[2]) == 0.0
    assert 0 <= n_warm < n_cold, (n_warm, n_cold)
    _eig_checks(_host_s(p1), ws.lam().cpu().numpy(), ws.Q().cpu().numpy())


def test_nan_parameter_clears_the_stamp(va):
    from volt_amd import ops
    N, T = 64, 8
    p, x, Y = make_case(N, T, 1, seed=11, dtype=torch.float64)
    xc, Yc = x.cuda(), Y.cuda()
    ws = ops.KronWorkspace(N, T, torch.device("cuda"), torch.float64, "linear")
    cold = ops.KronWorkspace(N, T, torch.device("cuda"), torch.float64, "linear")
    ops.kron_prologue(params_of(p), xc, Yc, ws, warm=True)
    bad = dict(p, raw_var=p["raw_var"].clone())
    bad["raw_var"][3] = float("nan")
    ops.kron_prologue(params_of(bad), xc, Yc, ws, warm=True)
    assert float(ws.state[1]) == 0.0                                       # no stamp: the next call starts cold
    ops.kron_prologue(params_of(p), xc, Yc, ws, warm=True)
    ops.kron_prologue(params_of(p), xc, Yc, cold)
    assert float(ws.state[2]) == 0.0 and float(ws.state[1]) != 0.0
    assert torch.equal(ws.lam(), cold.lam()) and torch.equal(ws.Q(), cold.Q()) and torch.equal(ws.resid, cold.resid)
    _eig_checks(_host_s(p), ws.lam().cpu().numpy(), ws.Q().cpu().numpy())


def test_warm_prologue_is_bitwise_repeatable(va):
    from volt_amd import ops
    N, T = 64, 31
    p, x, Y = make_case(N, T, 1, seed=5, dtype=torch.float64)
    xc, Yc = x.cuda(), Y.cuda()
    g = torch.Generator().manual_seed(2)
    seq = [p]
    for _ in range(4):
        seq.append(_walk(seq[-1], g))
    runs = []
    for _ in range(10):                                                    # fresh workspace, the same five calls
        ws = ops.KronWorkspace(N, T, torch.device("cuda"), torch.float64, "linear")
        got = []
        for q in seq:
            ops.kron_prologue(params_of(q), xc, Yc, ws, warm=True)
            got += [ws.state.clone(), ws.resid.clone(), ws.sigma2.clone(), ws.eig_info.double()]
        runs.append(torch.cat([t.reshape(-1) for t in got]).cpu())
    assert all(torch.equal(runs[0], r) for r in runs[1:])


# ------------------------------------------------------------------ 2. the split epilogue against the one-workgroup epilogue
SLICE = 256
EPI_N = [1, 31, 32, 33, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 1]


@pytest.mark.parametrize("T", [1, 3, 64])
@pytest.mark.parametrize("N", EPI_N)
def test_split_epilogue_vs_one_workgroup(va, N, T):
    """Both epilogues on the same resid / out / alpha / state in fp64.  Gates: the project's fp64 bound 1e-9 (of max(1, |.|)
    per quantity, as test_kron_mll_and_grads_vs_dense_oracle_fp64) against the dense oracle where N T <= 8192, and against the
    restatement's epilogue formulas on the same inputs everywhere (they differ from the kernels in the order of the sums over
    N only: N eps of each sum's terms, orders below the bound).  The difference between the two kernels is printed."""
    from volt_amd import _lib, ops
    assert ops.KRON_EPILOGUE_SLICE == SLICE
    p, x, Y = make_case(N, T, 1, seed=3 * N + T, dtype=torch.float64)
    xc, Yc, prm = x.cuda(), Y.cuda(), params_of(p)
    ws = ops.KronWorkspace(N, T, torch.device("cuda"), torch.float64, "linear")
    ops.kron_prologue(prm, xc, Yc, ws)
    out, alpha, info = ops.bm_step(xc, ws.ones, ws.sigma2, ws.resid, ws.bm, want_grad=True)
    assert not info.any()
    L, nres, pad = _lib.lib(), 3 + 3 * T, 32                               # pad: 256 bytes of NaN on either side
    nws = int(L.volt_kron_epilogue_workspace_bytes(N, T)) // 8
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    res1, res2, wbuf = nan(nres + pad), nan(nres + pad), nan(nws + 2 * pad)
    assert (wbuf.data_ptr() + 8 * pad) % 256 == 0
    rv, cf, var, rtn, rn = (t.reshape(-1).contiguous() for t in prm)
    head = (rv.data_ptr(), cf.data_ptr(), var.data_ptr(), rtn.data_ptr(), rn.data_ptr(), xc.data_ptr(), ws.resid.data_ptr(),
            out.data_ptr(), alpha.data_ptr(), ws.state.data_ptr())
    st = _lib.stream_ptr()
    _lib.check(L.volt_kron_epilogue_f64(*head, res1.data_ptr(), N, T, st), "volt_kron_epilogue")
    runs = []
    for _ in range(10):
        res2[:nres] = float("nan")
        _lib.check(L.volt_kron_epilogue_ws_f64(*head, res2.data_ptr(), wbuf.data_ptr() + 8 * pad, N, T, st), "volt_kron_epilogue_ws")
        runs.append(res2.clone())
    assert all(torch.equal(torch.nan_to_num(runs[0], nan=-7.0), torch.nan_to_num(r, nan=-7.0)) for r in runs[1:])
    for r in (res1, res2):                                                 # the sentinels behind res and around the workspace
        assert torch.isnan(r[nres:]).all() and torch.isfinite(r[:nres]).all()
    assert torch.isnan(wbuf[:pad]).all() and torch.isnan(wbuf[pad + nws:]).all()
    stride, ns = 2 * T * T + T, (N + SLICE - 1) // SLICE
    assert torch.isfinite(wbuf[pad:pad + ns * stride]).all()
    a, b = res1[:nres].cpu().numpy(), res2[:nres].cpu().numpy()
    print(f"N = {N}, T = {T}: max |split - one workgroup| = {np.abs(a - b).max():.3e} (max |res| = {np.abs(a).max():.3e})")

    def gate(got, mll, grads, what):
        assert abs(got[0] - mll) <= 1e-9 * max(1.0, abs(mll)), (what, got[0], mll)
        for k, gk in kref.unpack(got, T).items():
            want = np.asarray(grads[k], np.float64).reshape(gk.shape)
            assert np.abs(gk - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (what, k, gk, want)

    pn = {k: v.numpy() for k, v in p.items()}
    pro = kref.prologue_ref(pn, x.numpy(), Y.numpy())
    pro.update(vol=float(ws.state[0]), lam=ws.lam().cpu().numpy(), d=ws.d().cpu().numpy(), W=ws.W().cpu().numpy(),
               resid=ws.resid.cpu().numpy())
    pro["kappa"] = pro["vol"] * pro["lam"]                                  # the kernels' own inputs: eigenvector signs are theirs
    want = kref.epilogue_ref(pn, x.numpy(), pro, out.cpu().numpy(), alpha.cpu().numpy())
    for got, name in ((a, "one workgroup"), (b, "split")):
        gate(got, float(want[0]), kref.unpack(want, T), name + " vs restatement")
    if N * T <= 8192:
        ref, gref = oracle_mll(p, x, Y)
        for got, name in ((a, "one workgroup"), (b, "split")):
            gate(got, ref, {k: v.numpy() for k, v in gref.items()}, name + " vs dense oracle")


# ------------------------------------------------------------------ 3. MLL + gradients through ExactMarginalLogLikelihood
def _mll_errors(p, x, Y, solver):
    """(mll, ref, {name: (max |g - gref|, max |gref|)}) through ExactMarginalLogLikelihood."""
    from volt_amd.gp import ExactMarginalLogLikelihood
    m, lh = build(p, x, Y, solver)
    mll = ExactMarginalLogLikelihood(lh, m)
    out = mll(m(m.train_inputs[0]), m.train_targets)
    out.backward()
    ref, gref = _oracle(p, x, Y)
    errs = {}
    for k, prm in model_params(m, lh).items():
        g = prm.grad.detach().cpu().double().reshape(gref[k].shape)
        errs[k] = (float((g - gref[k]).abs().max()), float(gref[k].abs().max()))
    return out, ref, errs


_ORACLES = {}


def _oracle(p, x, Y):
    """oracle_mll once per case (the side-by-side test and the gate share 399 x 8)."""
    key = (tuple(Y.shape), float(x[0]), float(Y.double().sum()), float(p["raw_vol"].double().sum()))
    if key not in _ORACLES:
        _ORACLES[key] = oracle_mll(p, x.double(), Y.double())
    return _ORACLES[key]


SMALL = [(N, T) for N in (1, 2, 3, 63, 65, 129) for T in (1, 3)]
# every shape on the grid from 0 and on the grid from dt -- but N = 1 from dt only: on the one-point grid x = [0] K_x is the
# zero matrix whatever vol is, the oracle's d / d raw_vol is EXACTLY 0, and "2e-3 of the gradient's max" is no bound at all
# (measured there: 5.8e-8 and 2.4e-7 of rounding; the host restatement covers N = 1 on both grids with an absolute scale)
FP32_CASES = [(N, T, start) for N, T in CASES + SMALL for start in (0, 1) if (N, start) != (1, 0)]


@pytest.mark.parametrize("N,T,start", FP32_CASES)
def test_linear_mll_and_grads_vs_dense_oracle_fp32(va, N, T, start):
    p, x, Y = make_case(N, T, start, seed=100 * T + N + start)
    out, ref, errs = _mll_errors(p, x, Y, "linear")
    assert out.dtype == torch.float32
    assert abs(float(out) - ref) <= 5e-5 * max(1.0, abs(ref)), (float(out), ref)
    for k, (err, scale) in errs.items():
        assert err <= 2e-3 * scale, (k, err, scale)


@pytest.mark.parametrize("start", [0, 1])
def test_linear_mll_and_grads_vs_dense_oracle_fp64(va, start):
    p, x, Y = make_case(399, 8, start, seed=7 + start, dtype=torch.float64)
    out, ref, errs = _mll_errors(p, x, Y, "linear")
    assert out.dtype == torch.float64
    assert abs(float(out) - ref) <= 1e-9 * max(1.0, abs(ref)), (float(out), ref)
    for k, (err, scale) in errs.items():
        assert err <= 1e-9 * max(1.0, scale), (k, err, scale)


def test_linear_and_dense_errors_side_by_side(va):
    """399 x 8, fp32, the same parameters through both solvers: their errors against the oracle, printed (README row 4.14).
    Not gated against each other -- both share the fp32 rounding of resid, so "linear <= dense" per quantity could fail by
    chance; each is gated against the oracle by its own test."""
    p, x, Y = make_case(399, 8, 1, seed=100 * 8 + 399 + 1)
    rows = {s: _mll_errors(p, x, Y, s) for s in ("dense", "linear")}
    ref = rows["dense"][1]
    print(f"399 x 8 fp32, relative errors against the dense fp64 oracle (mll = {ref:.6f})")
    print("  %-16s %10s %10s" % ("quantity", "dense", "linear"))
    print("  %-16s %10.2e %10.2e" % ("mll", *(abs(float(rows[s][0]) - ref) / max(1.0, abs(ref)) for s in ("dense", "linear"))))
    for k in ORDER:
        print("  %-16s %10.2e %10.2e" % (k, *(rows[s][2][k][0] / rows[s][2][k][1] for s in ("dense", "linear"))))


# ------------------------------------------------------------------ 4. the posterior
@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("H", [1, 8, 100])
@pytest.mark.parametrize("N,T", [(120, 3), (399, 8)])
def test_linear_posterior_vs_dense_oracle(va, N, T, H, start):
    """test_gpu_multitask.test_posterior_vs_dense_oracle's checks and bounds on the linear model."""
    p, x, Y = make_case(N, T, start, seed=N + T + H)
    m, lh = build(p, x, Y)
    m.eval()
    xs = x[-1] + (torch.arange(H, dtype=torch.float32) + 1) / 252.
    post = m(xs.cuda())
    mref, cref = oracle_posterior(p, x.double(), Y.double(), xs.double())
    mean = post.mean.detach().cpu().double()
    assert tuple(mean.shape) == (H, T)
    assert float((mean - mref).abs().max()) <= 2e-4 * max(1.0, float(mref.abs().max()))
    cov = post.covariance_matrix.cpu().double()
    assert float((cov - cref).abs().max()) <= 2e-4 * float(cref.abs().max())
    var = post.variance.cpu().double()
    assert float((var.reshape(-1) - torch.diagonal(cref)).abs().max()) <= 2e-4 * float(cref.abs().max())
    V, L = post.root_blocks()
    V, L = V.cpu().double(), L.cpu().double()
    R = torch.einsum("tj,jhk->htkj", V, L).reshape(H * T, H * T)
    assert float((R @ R.T - cref).abs().max()) <= 2e-4 * float(cref.abs().max())
    z = torch.randn(H, T, generator=torch.Generator().manual_seed(H))
    s = post.sample(base_samples=z.cuda()).cpu().double()
    want = mean.reshape(-1) + R @ z.double().reshape(-1)
    assert float((s.reshape(-1) - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    assert tuple(post.sample(torch.Size((4,))).shape) == (4, H, T)


# ------------------------------------------------------------------ 5. the trainer
@pytest.fixture(scope="module")
def adam_case():
    """130 x 3, 40 iterations: the paths, the initial draws and the fp64 CPU Adam trajectory, once for the three loops."""
    from volt_amd.gp import MultitaskGaussianLikelihood
    from volt_amd.models import MultitaskBMGP
    from volt_amd.train_utils import LR_VOL
    T, n, iters = 3, 130, 40
    x, F, vol = sde_batch(T, n, seed=21)
    tx, vp = torch.tensor(x, device="cuda"), torch.tensor(vol, device="cuda")
    torch.manual_seed(5)
    lh0 = MultitaskGaussianLikelihood(T).cuda()
    lh0.noise = 1e-3
    m0 = MultitaskBMGP(tx, vp.log().t(), lh0, solver="linear")
    p0 = {k: v.detach().cpu() for k, v in model_params(m0, lh0).items()}
    want = _cpu_adam_oracle(p0, tx.cpu().double(), vp.log().t().cpu().double(), iters, LR_VOL)
    return tx, vp, iters, want


@pytest.mark.parametrize("graph", [False, True, None])
def test_train_vol_model_multitask_linear_matches_cpu_adam(va, adam_case, graph):
    """The bounds of test_train_vol_model_multitask_matches_cpu_adam, eager / captured / graph=None (which captures)."""
    from volt_amd.train_utils import TrainVolModelMultitask
    tx, vp, iters, want = adam_case
    torch.manual_seed(5)                                     # the same initial draws
    m, lh = TrainVolModelMultitask(tx, vp, train_iters=iters, graph=graph, solver="linear")
    assert m.solver == "linear" and not hasattr(m, "_base")
    for k, prm in model_params(m, lh).items():
        got = prm.detach().cpu().double().reshape(want[k].shape)
        assert float((got - want[k]).abs().max()) <= 2e-3, (k, got, want[k])


def test_train_vol_model_multitask_linear_graph_equals_eager(va):
    """test_train_vol_model_multitask_graph_equals_eager's criterion (bitwise equal losses) on the linear iteration: warm
    prologue -> chain step -> split epilogue -> fused Adam, captured once and replayed -- the eigenvectors carried in the
    workspace go through the same sequence of calls in both runs."""
    from volt_amd import gp
    from volt_amd.models import MultitaskBMGP
    from volt_amd.optim import FusedAdam
    from volt_amd.train_utils import LR_VOL
    T, n, iters, warm = 4, 300, 20, 3
    x, F, vol = sde_batch(T, n, seed=8)
    tx, vp = torch.tensor(x, device="cuda"), torch.tensor(vol, device="cuda")
    runs = {}
    for graph in (False, True):
        torch.manual_seed(9)
        lh = gp.MultitaskGaussianLikelihood(T).cuda()
        lh.noise = 1e-3
        m = MultitaskBMGP(tx, vp.log().t(), lh, solver="linear")
        opt = FusedAdam(list(m.parameters()), lr=LR_VOL)
        mll = gp.ExactMarginalLogLikelihood(lh, m)
        target = m.train_targets

        def it():
            loss = -mll(m(m.train_inputs[0]), target)
            loss.backward()
            return loss

        losses = []
        with gp.deferred_checks(immediate=True) as chk:
            nwarm = warm if graph else iters
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(nwarm):
                    opt.zero_grad(set_to_none=True)
                    losses.append(it().detach().clone())
                    opt.step()
            torch.cuda.current_stream().wait_stream(side)
            if graph:
                chk.immediate = False
                opt.zero_grad(set_to_none=True)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    static = it()
                    opt.step()
                for _ in range(warm, iters):
                    g.replay()
                    losses.append(static.detach().clone())
                assert chk.any_bad() == 0
        runs[graph] = torch.stack(losses).cpu()
    assert torch.equal(runs[False], runs[True]), (runs[False], runs[True])


# ------------------------------------------------------------------ 6. the batched models and the driver
def _batched(kind, tx, F, vp, vol_solver):
    from volt_amd.gp import GaussianLikelihood
    from volt_amd.models import VoltMagpie, VoltronGP
    from volt_amd.models.Volt import Volt
    T = vp.shape[0]
    ty = torch.log(F[:, 1:])
    torch.manual_seed(0)                                     # the same draws of covar_factor and raw_var for both solvers
    if kind == "VoltMagpie":
        return VoltMagpie(tx, ty, GaussianLikelihood(batch_shape=torch.Size([T])).cuda(), vp, k=20, multitask_vol=True,
                          vol_solver=vol_solver)
    if kind == "VoltronGP":
        return VoltronGP(tx, ty, GaussianLikelihood(batch_shape=torch.Size([T])).cuda(), vp, multitask_vol=True,
                         vol_solver=vol_solver)
    full_x = torch.arange(F.shape[1], device="cuda") / 252.                 # Volt keeps [1:] of its inputs and prices
    return Volt(full_x, torch.log(F), mean="ewma", vol_path=vp, k=20, multitask_vol=True, vol_solver=vol_solver)


@pytest.mark.parametrize("kind", ["VoltMagpie", "VoltronGP", "Volt"])
def test_batched_models_multitask_vol_linear(va, kind):
    from volt_amd.models import MultitaskBMGP
    T, n, H = 4, 150, 6
    x, F, vol = sde_batch(T, n, seed=5)
    tx, Fd, vp = torch.tensor(x, device="cuda"), torch.tensor(F, device="cuda"), torch.tensor(vol, device="cuda")
    lin, dense = _batched(kind, tx, Fd, vp, "linear"), _batched(kind, tx, Fd, vp, "dense")
    assert isinstance(lin.vol_model, MultitaskBMGP) and lin.vol_model.solver == "linear" and lin.vol_solver == "linear"
    assert not hasattr(lin.vol_model, "_base") and dense.vol_model.solver == "dense"
    # one vol MLL + backward, against the oracle on the grid the model was built on
    vm = lin.vol_model
    grid = vm.train_inputs[0][:, 0]
    mll = lin.VolMLL()
    mll.backward()
    p = {k: v.detach().cpu().double() for k, v in model_params(vm, lin.vol_lh).items()}
    ref, gref = oracle_mll(p, grid.cpu().double(), vp.log().t().cpu().double())
    assert abs(float(mll) - ref) <= 5e-5 * max(1.0, abs(ref))
    for k, prm in model_params(vm, lin.vol_lh).items():
        g = prm.grad.detach().cpu().double().reshape(gref[k].shape)
        assert float((g - gref[k]).abs().max()) <= 2e-3 * float(gref[k].abs().max()), k
    # the vol samples GeneratePrediction is handed: [T,H], the dense-built model's on identical draws
    test_x = (torch.arange(H, device="cuda") + 1) / 252. + grid[-1]
    z = torch.randn(H, T, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    got = {}
    for name, m in (("linear", lin), ("dense", dense)):
        m.vol_model.eval()
        got[name] = m._vol_layout(m.vol_model(test_x).sample(base_samples=z).exp())
    assert tuple(got["linear"].shape) == (T, H)
    assert float((got["linear"] - got["dense"]).abs().max()) <= 2e-4 * float(got["dense"].abs().max())
    if kind == "VoltronGP":                                  # (batched VoltMagpie.GeneratePrediction takes no H test points)
        pred, pv = lin.SamplePrediction(test_x, return_vol=True)
        assert tuple(pv.shape) == (T, H) and tuple(pred.shape) == (T, H) and bool(torch.isfinite(pred).all())


def test_stocks_driver_with_the_linear_multitask_vol_forecaster(va):
    from volt_amd.forecast import GenerateStockPredictionsBatch
    B, ntrain, H, S = 3, 130, 4, 5
    _, F, _ = sde_batch(B, ntrain + 5, seed=77)
    closes = torch.as_tensor(np.asarray(F)).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    torch.manual_seed(1)
    dbg = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = GenerateStockPredictionsBatch(["AAA", "BBB", "CCC"], closes, forecast_horizon=H, train_iters=3, nsample=S,
                                            ntrain=ntrain, mean="ewma", k=10, ntimes=1, vol_iters=4, generator=g, debug=dbg,
                                            vol_solver="linear", multitask_vol=True)
    assert tuple(out.shape) == (B, S, H) and torch.isfinite(out).all()
    assert tuple(dbg["pred_vol"].shape) == (B, S, H) and bool((dbg["pred_vol"] > 0).all())


# ------------------------------------------------------------------ 7. errors
def test_nan_parameter_raises_nan_error(va):
    from volt_amd.gp import ExactMarginalLogLikelihood, NanError, NotPSDError
    p, x, Y = make_case(120, 3, 1, seed=2)
    p["raw_var"][1] = float("nan")
    m, lh = build(p, x, Y)
    with pytest.raises(NanError) as err:
        ExactMarginalLogLikelihood(lh, m)(m(m.train_inputs[0]), m.train_targets)
    assert not isinstance(err.value, NotPSDError)


def test_cpu_tensor_raises(va):
    from volt_amd import ops
    from volt_amd._lib import VoltHipError
    p, x, Y = make_case(40, 3, 1, seed=1)
    with pytest.raises(VoltHipError):
        ops.kron_bm_step(params_of(p), x, Y.cuda())
    with pytest.raises(VoltHipError):
        ops.kron_bm_step(params_of(p), x.cuda(), Y)


# ------------------------------------------------------------------ 8. no N^2 anywhere
def test_no_quadratic_memory_at_n_65536(va):
    """N = 65536, T = 8: construction, one step + backward and the posterior at H = 20 grow the peak of allocated device
    memory by less than 64 MB (the bound of tests/test_gpu_bm_linear.py) -- one fp32 N x N matrix would be 17 GB."""
    from volt_amd.gp import ExactMarginalLogLikelihood
    N, T, H = 65536, 8, 20
    p, x, Y = make_case(N, T, 1, seed=9)
    xc, Yc = x.cuda(), Y.cuda()
    # torch's BLAS handles take their one-time workspaces from the caching allocator at the first product of each kind: not
    # this model's memory, so they are taken before the baseline (the posterior multiplies in fp64, plain and batched)
    w = torch.ones(2, 4, 4, dtype=torch.float64, device="cuda")
    (w[0] @ w[1], w @ w, w.float() @ w.float())
    del w
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    grown = lambda: torch.cuda.max_memory_allocated() - base
    m, lh = build(p, xc, Yc)
    print(f"peak growth after construction: {grown() / 2 ** 20:.1f} MB")
    mll = ExactMarginalLogLikelihood(lh, m)
    out = mll(m(m.train_inputs[0]), m.train_targets)
    out.backward()
    torch.cuda.synchronize()
    print(f"peak growth after one step + backward: {grown() / 2 ** 20:.1f} MB")
    m.eval()
    xs = xc[-1] + (torch.arange(H, device="cuda") + 1) / 252.
    post = m(xs)
    torch.cuda.synchronize()
    print(f"peak growth after the posterior at H = {H}: {grown() / 2 ** 20:.1f} MB")
    assert grown() < 64 * 2 ** 20, grown()
    assert bool(torch.isfinite(out)) and bool(torch.isfinite(post.mean).all()) and tuple(post.mean.shape) == (H, T)
    assert all(bool(torch.isfinite(prm.grad).all()) for prm in model_params(m, lh).values())
