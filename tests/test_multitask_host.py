"""MultitaskBMGP's host side (no GPU): parameter names, shapes and registration order, the constructor's init, the
likelihood's noise setter, the gpytorch / voltron names, no CPU fallback, and csrc/kron.hip cross-compiling for gfx950
without scratch."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(T=3, N=12, seed=0):
    from volt_amd.gp import MultitaskGaussianLikelihood
    from volt_amd.models import MultitaskBMGP
    lh = MultitaskGaussianLikelihood(num_tasks=T)
    torch.manual_seed(seed)
    return MultitaskBMGP(torch.arange(N, dtype=torch.float32) / 252., torch.zeros(N, T), lh), lh


def test_parameter_names_shapes_and_order():
    m, _ = _model(T=3)
    got = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    assert got == [("likelihood.raw_task_noises", (3,)), ("likelihood.raw_noise", (1,)),
                   ("covar_module.task_covar_module.covar_factor", (3, 1)),
                   ("covar_module.task_covar_module.raw_var", (3,)),
                   ("covar_module.data_covar_module.raw_vol", (1,))]
    assert not hasattr(type(m), "named_priors") or not list(m.named_priors())


def test_constructor_init_divides_covar_factor_only():
    torch.manual_seed(4)
    f = torch.randn(5, 1)
    v = torch.randn(5)
    m, _ = _model(T=5, seed=4)
    task = m.covar_module.task_covar_module
    assert torch.equal(task.covar_factor.detach(), f / 10.)
    assert torch.equal(task.raw_var.detach(), v)                 # var.data /= 10. divides a temporary
    assert torch.allclose(task.var, F.softplus(v))
    Kt = task.covar_matrix.evaluate()
    assert torch.allclose(Kt, (f / 10.) @ (f / 10.).T + torch.diag(F.softplus(v)))
    # the mean as the reference writes it: -1/2 vol^2 x K_t[t,t]
    x = torch.arange(12, dtype=torch.float32) / 252.
    vol = m.covar_module.data_covar_module.vol
    assert torch.allclose(m.mean_module(x), -0.5 * vol ** 2 * x[:, None] * torch.diagonal(Kt)[None, :])


def test_noise_setter():
    from volt_amd.gp import MultitaskGaussianLikelihood
    lh = MultitaskGaussianLikelihood(num_tasks=4)
    assert torch.allclose(lh.noise, torch.tensor([F.softplus(torch.tensor(0.)) + 1e-4]))
    lh.noise = 1e-3
    assert float(lh.noise) == pytest.approx(1e-3, rel=1e-5)
    assert float(lh.raw_noise) == pytest.approx(float(torch.log(torch.expm1(torch.tensor(1e-3 - 1e-4)))), rel=1e-5)
    assert torch.allclose(lh.task_noises, F.softplus(torch.zeros(4)) + 1e-4)
    with pytest.raises(NotImplementedError):
        MultitaskGaussianLikelihood(num_tasks=4, rank=1)


def test_namespaces_resolve():
    code = ("import volt_amd; volt_amd.install_as_voltron(); import voltron, gpytorch; "
            "from voltron.models import MultitaskBMGP; "
            "assert voltron.MultitaskBMGP is MultitaskBMGP is volt_amd.MultitaskBMGP; "
            "from volt_amd import gp; from volt_amd.kernels import IndexKernel, MultitaskKernel; "
            "assert gpytorch.likelihoods.MultitaskGaussianLikelihood is gp.MultitaskGaussianLikelihood; "
            "assert gpytorch.distributions.MultitaskMultivariateNormal is gp.MultitaskMultivariateNormal; "
            "assert gpytorch.kernels.MultitaskKernel is MultitaskKernel and gpytorch.kernels.IndexKernel is IndexKernel")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_multitask_kernel_dense_is_interleaved():
    from volt_amd.kernels import BMKernel, MultitaskKernel
    torch.manual_seed(1)
    k = MultitaskKernel(BMKernel(), num_tasks=3)
    x = torch.arange(4, dtype=torch.float32) / 252.
    K = k.forward(x.unsqueeze(-1))
    Kt = k.task_covar_module.covar_matrix.evaluate()
    Kx = 0.2 * torch.minimum(x[:, None], x[None, :])
    for n, mm, s, t in ((1, 2, 0, 2), (3, 3, 1, 1), (2, 0, 2, 1)):
        assert torch.allclose(K[n * 3 + s, mm * 3 + t], Kx[n, mm] * Kt[s, t])


def test_cpu_tensors_raise():
    from volt_amd import ops
    from volt_amd._lib import VoltHipError
    from volt_amd.gp import ExactMarginalLogLikelihood
    m, lh = _model(T=3)
    mll = ExactMarginalLogLikelihood(lh, m)
    with pytest.raises(VoltHipError):
        mll(m(m.train_inputs[0]), m.train_targets)
    with pytest.raises(VoltHipError):
        ops.syev_small(torch.eye(3, dtype=torch.float64))
    m.eval()
    with pytest.raises(VoltHipError):
        m(torch.tensor([0.1]))


def test_argument_validation_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    assert L.volt_syev_small_f64(None, 9, 1, 1, 1, 1, 3, None) == -1
    assert L.volt_syev_small_f64(1, 65 * 65, 1, 1, 1, 1, 65, None) == -7           # T > 64
    assert L.volt_kron_state_bytes(65) == 0 and L.volt_kron_state_bytes(0) == 0
    assert L.volt_kron_state_bytes(8) == (8 + 2 * 8 + 2 * 64) * 8
    args = [1] * 12
    assert L.volt_kron_prologue_f32(*args[:7], 100, *args[:4], 10, 65, None) == -14
    assert L.volt_kron_prologue_f32(*args[:7], 2, *args[:4], 10, 3, None) == -8     # ldy < T
    assert L.volt_kron_epilogue_f64(*args[:11], 10, 0, None) == -13


def test_kron_hip_cross_compiles_without_scratch(tmp_path):
    from volt_amd.build import FLAGS, _hipcc
    src = os.path.join(ROOT, "volt_amd", "csrc", "kron.hip")
    r = subprocess.run([_hipcc(), *FLAGS, "-c", src, "-o", str(tmp_path / "kron.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(kernels) == 5 and len(scratch) == 5, r.stderr[-2000:]
    assert scratch == [0] * 5, dict(zip(kernels, scratch))
