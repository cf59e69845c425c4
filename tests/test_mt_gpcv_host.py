"""MultitaskVariationalGP's host side (no GPU): the names resolve, parameter names / shapes / order / start values, the
two fp64 restatements of the ELBO (dense definition vs Kronecker-structured form, tests/mt_gpcv_ref.py) agree, no CPU
fallback, what is out of scope raises, and csrc/gpcv_mt.hip cross-compiles for gfx950 without scratch."""
import os
import re
import subprocess
import sys

import pytest
import torch

import mt_gpcv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(T=3, N=12, seed=0, x0=1):
    from volt_amd.kernels import BMKernel
    from volt_amd.models import MultitaskVariationalGP
    torch.manual_seed(seed)
    x = (torch.arange(N, dtype=torch.float32) + x0) / 252.
    return MultitaskVariationalGP(x, T, covar_module=BMKernel()), x


def test_names_resolve():
    from volt_amd.models import MultitaskVariationalGP  # noqa: F401
    code = ("import volt_amd; volt_amd.install_as_voltron(); import gpytorch; "
            "from voltron.models import MultitaskVariationalGP; import volt_amd.models as m; "
            "assert MultitaskVariationalGP is m.MultitaskVariationalGP; from volt_amd import gp; "
            "assert gpytorch.means.MultitaskMean is gp.MultitaskMean; "
            "from voltron.train_utils import LearnGPCVMultitask, FitGPCVMultitask")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_parameter_names_shapes_order_and_start_values():
    m, x = _model(T=3, N=12, seed=5)
    got = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    assert got == [("variational_mean", (12, 3)), ("variational_covar_root", (12, 12)),
                   ("variational_task_covar_root", (3, 3)), ("index_kernel.covar_factor", (3, 1)),
                   ("index_kernel.raw_var", (3,)), ("data_kernel.raw_vol", (1,)),
                   ("mean_module.base_means.0.constant", (1,)), ("mean_module.base_means.1.constant", (1,)),
                   ("mean_module.base_means.2.constant", (1,))]
    torch.manual_seed(5)                                   # draw order of the reference's __init__: mean, covar_factor, raw_var
    mean0, cf0, rv0 = 0.01 * torch.randn(12, 3), torch.randn(3, 1), torch.randn(3)
    assert torch.equal(m.variational_mean.detach(), mean0)
    assert torch.equal(m.index_kernel.covar_factor.detach(), cf0)
    assert torch.equal(m.index_kernel.raw_var.detach(), rv0)
    assert torch.equal(m.variational_covar_root.detach(), torch.eye(12))
    assert torch.equal(m.variational_task_covar_root.detach(), torch.eye(3))
    assert all(float(b.constant.detach()) == 0.0 for b in m.mean_module.base_means)
    assert m.variational_strategy is m and m.num_tasks == 3 and m.inducing_points is x
    assert tuple(m.mean_module(x).shape) == (12, 3)


@pytest.mark.parametrize("N,T", [(48, 3), (64, 5)])
def test_dense_definition_equals_structured_form(N, T):
    """The NT x NT definition and the Kronecker-structured form agree to 1e-10 relative, in value and in all seven
    autograd gradients (both in fp64)."""
    p, x, y = R.case(N, T, seed=1)
    td, gd = R.value_and_grads(R.dense, p, x, y)
    ts, gs = R.value_and_grads(R.struct, p, x, y)
    for k in ("F", "ell", "kl"):
        err = abs(float(td[k] - ts[k])) / max(1.0, abs(float(td[k])))
        print(N, T, k, float(td[k]), err)
        assert err < 1e-10
    assert set(gd) == set(R.KEYS)
    for k in R.KEYS:
        err = float((gd[k] - gs[k]).abs().max() / gd[k].abs().max().clamp_min(1e-300))
        print(N, T, "grad", k, err)
        assert err < 1e-10, k
        if k in ("Lx", "Lt"):                               # junk above the diagonals is ignored
            assert float(gs[k].triu(1).abs().max()) == 0.0


def test_structured_form_at_one_task_is_the_single_task_elbo():
    """T = 1 with K_t = S_t = 1 (covar_factor = 0, raw_var = log(e - 1), L_t = 1) is the single-task ELBO of
    oracle/gpcv_oracle.py."""
    import math
    from oracle import gpcv_oracle as GO
    p, x, y = R.case(40, 1, seed=3)
    p["F"] = torch.zeros(1, 1, dtype=torch.float64)
    p["raw_var"] = torch.tensor([math.log(math.e - 1)], dtype=torch.float64)
    p["Lt"] = torch.ones(1, 1, dtype=torch.float64)
    t = R.struct(p, x, y)
    gx, gw = GO.gauss_hermite(75)
    s = GO.elbo_terms(p["m"][:, 0], p["Lx"], p["c"], R.data_cov(x, p["raw_vol"]), y[:, 0], gx, gw)
    assert abs(float(t["F"] - s["elbo"])) < 1e-12 * max(1.0, abs(float(s["elbo"])))
    assert abs(float(t["kl"] - s["kl"])) < 1e-10 * abs(float(s["kl"]))


def test_cpu_tensors_raise_and_out_of_scope_raises():
    from volt_amd import ops
    from volt_amd._lib import VoltHipError
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import MultitaskVariationalGP
    from volt_amd.variational import VariationalELBO
    m, x = _model(T=3, N=12)
    lh = VolatilityGaussianLikelihood(param="exp")
    elbo = VariationalELBO(lh, m, 36)
    with pytest.raises(VoltHipError):
        elbo(m(x), torch.zeros(12, 3))
    with pytest.raises(VoltHipError):
        m.kl_divergence()
    with pytest.raises(VoltHipError):
        ops.gpcv_mt_step(torch.eye(4), torch.zeros(4, 2), torch.zeros(2), torch.eye(4), torch.eye(2), torch.zeros(2),
                         torch.zeros(2), torch.zeros(4, 2), torch.zeros(3), torch.zeros(3))
    with pytest.raises(NotImplementedError):
        MultitaskVariationalGP(x, 3, covar_module=BMKernel(), rank=2)
    with pytest.raises(NotImplementedError):
        m(x + 1.0)
    with pytest.raises(NotImplementedError):
        m(x[:5])
    with pytest.raises(NotImplementedError):
        m.initialize_variational_parameters(VolatilityGaussianLikelihood(param="cv"), x, y=torch.ones(12, 3))
    with pytest.raises(NotImplementedError):
        VariationalELBO(VolatilityGaussianLikelihood(param="cv"), m, 36)
    with pytest.raises(TypeError):                          # other latent types are still refused
        elbo(object(), torch.zeros(12, 3))
    with pytest.raises(ValueError):
        MultitaskVariationalGP(x, 65, covar_module=BMKernel())


def test_argument_validation_and_exports_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    assert "volt_gpcv_mt_workspace_bytes" in _lib.EXPORTS and "volt_gpcv_mt_step_f32" in _lib.EXPORTS
    assert L.volt_gpcv_mt_workspace_bytes(300, 65, 0) == 0 and L.volt_gpcv_mt_workspace_bytes(300, 0, 0) == 0
    assert L.volt_gpcv_mt_workspace_bytes(0, 4, 0) == 0
    b0, b1 = L.volt_gpcv_mt_workspace_bytes(300, 4, 0), L.volt_gpcv_mt_workspace_bytes(300, 4, 1)
    assert b1 > b0 > L.volt_mll_workspace_bytes(1, 300, 1)
    # ONE factorisation, one variational root: the scratch does not scale with T the way the batched step's does
    assert L.volt_gpcv_mt_workspace_bytes(300, 64, 0) < 2 * b0 < L.volt_gpcv_workspace_bytes(8, 300, 0)
    tail = [75, 1e-6, 1e-3, 1.0, 1.0]
    assert L.volt_gpcv_mt_step_f32(None, 8, 1e-3, *([None] * 9), *tail, *([None] * 10), 8, 2, 0, None) == -1
    assert L.volt_gpcv_mt_step_f32(1, 4, 1e-3, *([1] * 9), *tail, *([1] * 10), 8, 2, 0, None) == -2      # ldk < N
    assert L.volt_gpcv_mt_step_f32(1, 8, 1e-3, *([1] * 9), *tail, *([1] * 7), None, 1, 256, 8, 65, 0, None) == -29
    assert L.volt_gpcv_mt_step_f32(1, 8, 1e-3, *([1] * 9), *tail, *([1] * 7), None, 1, 100, 8, 2, 0, None) == -27


def test_gpcv_mt_hip_cross_compiles_without_scratch(tmp_path):
    from volt_amd.build import FLAGS, SOURCES, _hipcc
    assert "gpcv_mt.hip" in SOURCES
    src = os.path.join(ROOT, "volt_amd", "csrc", "gpcv_mt.hip")
    r = subprocess.run([_hipcc(), *FLAGS, "-c", src, "-o", str(tmp_path / "gpcv_mt.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(kernels) == 8 and len(scratch) == 8, r.stderr[-2000:]
    assert scratch == [0] * 8, dict(zip(kernels, scratch))
    lib = os.path.join(ROOT, "volt_amd", "csrc", "libvolt_hip.so")
    from volt_amd import _lib
    _lib.lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    assert " T volt_gpcv_mt_step_f32" in syms and " T volt_gpcv_mt_workspace_bytes" in syms
