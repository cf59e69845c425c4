"""MultitaskBMGP(solver="linear")'s host side (no GPU): the fp64 restatement of the linear-time Kronecker evaluation
(tests/kron_chain_ref.py) against dense NT x NT fp64 autograd, the constructor's validation, no N x N at construction, the lazy
prior, the batched models' opt-in, the argument codes and workspace formula of the new entries, and csrc/kron_chain.hip
cross-compiling for gfx950 without scratch or spills."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import kron_chain_ref as kref
from test_gpu_multitask import make_case, oracle_mll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10                       # the bound of tests/test_bm_chain_host.py, relative to each quantity's scale


# ------------------------------------------------------------------ the restatement against the dense definition
@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("N", [1, 2, 3, 64, 65, 399])
def test_restatement_vs_dense_autograd(N, T, start):
    """MLL and all five gradients.  Scale of the MLL: max(1, |mll|) (it is a sum of O(1) terms per datum divided by N T); of a
    gradient: max(1, max |gradient|) over its entries (each entry is a difference of sums of that magnitude) -- the scales
    of the fp64 gate of tests/test_gpu_multitask.py."""
    p, x, Y = make_case(N, T, start, seed=1000 * T + 10 * N + start, dtype=torch.float64)
    mll, g = kref.kron_chain_ref({k: v.numpy() for k, v in p.items()}, x.numpy(), Y.numpy())
    ref, gref = oracle_mll(p, x, Y)
    errs = {"mll": abs(mll - ref) / max(1.0, abs(ref))}
    for k in kref.NAMES:
        want = gref[k].numpy().reshape(g[k].shape)
        errs[k] = float(np.abs(g[k] - want).max()) / max(1.0, float(np.abs(want).max()))
    print(f"restatement N={N} T={T} start={start}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= TOL, errs


# ------------------------------------------------------------------ the constructor
def _lh(T):
    from volt_amd.gp import MultitaskGaussianLikelihood
    return MultitaskGaussianLikelihood(num_tasks=T)


def test_constructor_validation():
    from volt_amd.models import MultitaskBMGP
    x = torch.arange(12, dtype=torch.float32) / 252.
    Y = torch.zeros(12, 3)
    with pytest.raises(ValueError, match="solver"):
        MultitaskBMGP(x, Y, _lh(3), solver="banded")
    with pytest.raises(ValueError, match="increasing"):
        MultitaskBMGP(x.flip(0), Y, _lh(3), solver="linear")
    with pytest.raises(ValueError, match="x\\[0\\] >= 0"):
        MultitaskBMGP(x - 1.0, Y, _lh(3), solver="linear")
    with pytest.raises(ValueError, match="1-D"):
        MultitaskBMGP(x.reshape(6, 2), Y, _lh(3), solver="linear")
    assert MultitaskBMGP(x, Y, _lh(3)).solver == "dense"                 # the default, and the dense model keeps its M
    assert tuple(MultitaskBMGP(x, Y, _lh(3))._base.shape) == (12, 12)
    MultitaskBMGP(x.flip(0), Y, _lh(3))                                  # ... and does not validate the grid


def test_no_n_by_n_at_construction():
    from volt_amd.models import MultitaskBMGP
    N, T = 257, 3
    m = MultitaskBMGP(torch.arange(N, dtype=torch.float32) / 252., torch.zeros(N, T), _lh(T), solver="linear")
    assert not hasattr(m, "_base")
    held = [v for v in vars(m).values() if torch.is_tensor(v)] + list(m.parameters()) + list(m.buffers())
    held += [t for t in m.train_inputs] + [m.train_targets]
    assert held and all(t.numel() < N * N for t in held), [tuple(t.shape) for t in held]
    prior = m(m.train_inputs[0]).lazy_covariance_matrix
    assert prior.linear and prior._M is None and tuple(prior.shape) == (N * T, N * T)
    with pytest.raises(ValueError, match="training grid"):
        m(torch.arange(N, dtype=torch.float32) / 365.)


def test_lazy_prior_evaluates_to_the_kronecker_product():
    from volt_amd.models import MultitaskBMGP
    torch.manual_seed(3)
    N, T = 9, 4
    x = torch.arange(1, N + 1, dtype=torch.float32) / 252.
    lin = MultitaskBMGP(x, torch.zeros(N, T), _lh(T), solver="linear")
    prior = lin(lin.train_inputs[0]).lazy_covariance_matrix
    vol = lin.covar_module.data_covar_module.vol.reshape(())
    Kt = lin.covar_module.task_covar_module.covar_matrix.evaluate()
    want = torch.kron(vol * torch.minimum(x[:, None], x[None, :]), Kt)
    assert torch.equal(prior.evaluate(), want) and torch.equal(prior.to_dense(), want)
    # the dense model's prior is unchanged: it carries its M
    torch.manual_seed(3)
    dense = MultitaskBMGP(x, torch.zeros(N, T), _lh(T))
    dprior = dense(dense.train_inputs[0]).lazy_covariance_matrix
    assert not dprior.linear and dprior.M is dense._base and torch.equal(dprior.evaluate(), want)


def test_init_vol_state_accepts_multitask_linear():
    from volt_amd.gp import GaussianLikelihood
    from volt_amd.models import MultitaskBMGP, VoltronGP
    T, N = 3, 20
    x = torch.arange(N, dtype=torch.float32) / 252.

    class _Probe(VoltronGP):                          # _init_vol_state alone: the constructors fill train_cov on the device
        def __init__(self, vol_solver):
            from volt_amd.gp import ExactGP
            ExactGP.__init__(self, x, torch.zeros(T, N), GaussianLikelihood(batch_shape=torch.Size([T])))
            self._vol_prior = lambda *a: None
            self._init_vol_state(x, torch.zeros(T, N), torch.full((T, N), 0.2), True, vol_solver, "linear")

    m = _Probe("linear")
    assert isinstance(m.vol_model, MultitaskBMGP) and m.vol_model.solver == "linear" and m.vol_solver == "linear"
    assert not hasattr(m.vol_model, "_base")
    assert _Probe("dense").vol_model.solver == "dense"
    with pytest.raises(ValueError, match="vol_solver"):
        _Probe("banded")


# ------------------------------------------------------------------ the C entries without a device
def test_argument_codes_of_the_new_entries():
    from volt_amd import _lib
    L = _lib.lib()
    a = [256] * 12
    for fn in (L.volt_kron_prologue_warm_f32, L.volt_kron_prologue_warm_f64):
        for k in range(7):                                                    # -1 .. -7: the pointers up to Y
            args = list(a[:7])
            args[k] = None
            assert fn(*args, 100, *a[:4], 10, 3, None) == -(k + 1)
        assert fn(*a[:7], 2, *a[:4], 10, 3, None) == -8                       # ldy < T
        for k in range(4):                                                    # -9 .. -12: resid, sigma2, state, info
            args = list(a[:4])
            args[k] = None
            assert fn(*a[:7], 100, *args, 10, 3, None) == -(9 + k)
        assert fn(*a[:7], 100, *a[:4], 0, 3, None) == -13
        assert fn(*a[:7], 100, *a[:4], 10, 0, None) == -14 and fn(*a[:7], 100, *a[:4], 10, 65, None) == -14
    for fn in (L.volt_kron_epilogue_ws_f32, L.volt_kron_epilogue_ws_f64):
        for k in range(11):                                                   # -1 .. -11: the pointers up to res
            args = list(a[:11])
            args[k] = None
            assert fn(*args, 256, 10, 3, None) == -(k + 1)
        assert fn(*a[:11], None, 10, 3, None) == -12 and fn(*a[:11], 257, 10, 3, None) == -12   # NULL / not 256-byte aligned
        assert fn(*a[:11], 256, 0, 3, None) == -13
        assert fn(*a[:11], 256, 10, 0, None) == -14 and fn(*a[:11], 256, 10, 65, None) == -14


def test_epilogue_workspace_formula():
    from volt_amd import _lib
    q = _lib.lib().volt_kron_epilogue_workspace_bytes
    assert q(0, 3) == 0 and q(-1, 3) == 0 and q(10, 0) == 0 and q(10, 65) == 0
    al = lambda b: (b + 255) // 256 * 256
    for N, T in ((1, 1), (256, 3), (257, 3), (4096, 64), (65536, 8)):
        assert q(N, T) == al(((N + 255) // 256) * (2 * T * T + T) * 8), (N, T)
    last = 0
    for N in (1, 255, 256, 257, 1000, 4096, 65536, 1 << 20):                  # monotone in N ...
        assert q(N, 8) >= last > -1
        last = q(N, 8)
    assert all(q(4096, T + 1) > q(4096, T) for T in range(1, 64))             # ... and in T
    assert q(65536, 64) < 64 * 2 ** 20                                         # nothing like an N x N matrix


def test_kron_workspace_solver_argument():
    from volt_amd import ops
    with pytest.raises(ValueError, match="solver"):
        ops.KronWorkspace(10, 3, torch.device("cpu"), solver="banded")


def test_kron_chain_hip_cross_compiles_without_scratch_or_spills(tmp_path):
    """The new kernels live in csrc/kron_chain.hip (csrc/kron.hip keeps its five); LDS stays under 160 KB per workgroup."""
    from volt_amd.build import FLAGS, SOURCES, _hipcc
    assert "kron_chain.hip" in SOURCES
    src = os.path.join(ROOT, "volt_amd", "csrc", "kron_chain.hip")
    r = subprocess.run([_hipcc(), *FLAGS, "-c", src, "-o", str(tmp_path / "kron_chain.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    field = lambda name: [int(v) for v in re.findall(name + r": (\d+)", r.stderr)]
    scratch, sspill, vspill, lds = (field(n) for n in (r"ScratchSize \[bytes/lane\]", "SGPRs Spill", "VGPRs Spill",
                                                       r"LDS Size \[bytes/block\]"))
    assert len(kernels) == 8 and all(len(v) == 8 for v in (scratch, sspill, vspill, lds)), r.stderr[-2000:]
    for want in ("kron_eigen_warm_kernel", "kron_rows_kernel", "kron_gram_kernel", "kron_epilogue_ws_kernel"):
        assert sum(want in k for k in kernels) == 2, (want, kernels)          # _f32 and _f64
    assert scratch == [0] * 8 and sspill == [0] * 8 and vspill == [0] * 8, dict(zip(kernels, zip(scratch, sspill, vspill)))
    assert max(lds) < 160 * 1024, dict(zip(kernels, lds))
