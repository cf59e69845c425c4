#!/usr/bin/env python3
"""Golden vectors for the start-up of the multi-task GPCV model, made by EXECUTING the reference's own method on a fake
``self``, for BOTH likelihood branches:

    voltron/models/multi_task_variational_gp.py:38-88     MultitaskVariationalGP.initialize_variational_parameters
    voltron/likelihoods/volatility_likelihood.py:9-51     VolatilityGaussianLikelihood(K=1, batch_shape=[T]): its own draws of
                                                          raw_a, raw_b, raw_c, its constraints, its forward (sigma on "cv")
    voltron/kernels/BMKernel.py:38-52                     BMKernel.forward (kuu)

Runs only in the build container (needs /root/reference); writes ``mt_gpcv_cv.npz`` next to itself.  The stand-ins for
gpytorch / botorch are those of make_golden_gpcv.py, imported and not edited; added here is what the model file's import
lines need besides (GP, IndexKernel, MultitaskMean, ZeroMean, KroneckerProductLazyTensor, MultitaskMultivariateNormal,
settings: names only, except IndexKernel, which carries covar_factor and a ``var`` property so that lines 86-88 execute)
and one method the method calls:

    LazyTensor.root_inv_decomposition().root  -> C^-T for A = C C', C = the lower psd_safe_cholesky factor

ASSUMPTION, as make_golden_gpcv.py states for its own root_decomposition: gpytorch picks the Cholesky route for a dense
matrix of this size (N <= 800); its Lanczos route would give another root of the same inverse.  Only root root' enters the
model (the tests compare that product), so the assumption decides rounding, not meaning.

Cases (N, T) = (60, 3), (90, 2), each in fp64 and in fp32 from the same series and the same raws.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mt_gpcv_cv.py
"""
import importlib.util
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
warnings.filterwarnings("ignore")


def _local(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(OUT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    G = _local("make_golden_gpcv")
    sde_series = _local("make_golden").sde_series
    G._install_standins()

    def root_inv_decomposition(self, **kw):
        C = G.psd_safe_cholesky(self.tensor)
        eye = torch.eye(C.shape[-1], dtype=C.dtype)
        return types.SimpleNamespace(root=G._Dense(torch.linalg.solve_triangular(C, eye, upper=False).mT))
    G._Dense.root_inv_decomposition = root_inv_decomposition

    class IndexKernel(G._Module):
        def __init__(self, num_tasks, rank=1, dtype=torch.float32):
            super().__init__()
            self.covar_factor = torch.nn.Parameter(torch.randn(num_tasks, rank, dtype=dtype))
            self.raw_var = torch.nn.Parameter(torch.randn(num_tasks, dtype=dtype))

        @property
        def var(self):
            return torch.nn.functional.softplus(self.raw_var)

    empty = lambda n: type(n, (G._Module,), {})
    sys.modules["gpytorch.models"].GP = empty("GP")
    sys.modules["gpytorch.kernels"].IndexKernel = IndexKernel
    sys.modules["gpytorch.lazy"].KroneckerProductLazyTensor = empty("KroneckerProductLazyTensor")
    sys.modules["gpytorch.means"].MultitaskMean = empty("MultitaskMean")
    sys.modules["gpytorch.distributions"].MultitaskMultivariateNormal = empty("MultitaskMultivariateNormal")
    sys.modules["gpytorch"].settings = types.SimpleNamespace()
    BM = G._load("ref_bmkernel", "kernels/BMKernel.py")
    VL = G._load("ref_vol_likelihood", "likelihoods/volatility_likelihood.py")
    MT = G._load("ref_mtvgp", "models/multi_task_variational_gp.py")

    out = {}
    for tag, (n, T, seed) in {"n60_t3": (60, 3, 2019), "n90_t2": (90, 2, 31)}.items():
        prices = torch.stack([torch.tensor(sde_series(n, seed + i)[0]) for i in range(T)]).double()        # [T,N+1]
        x64 = (torch.arange(n + 1) / 252.).double()[:n]
        torch.manual_seed(seed)
        lik_cv = VL.VolatilityGaussianLikelihood(K=1, batch_shape=torch.Size([T]), param="cv")             # its own draws
        raws = {k: getattr(lik_cv, k).detach().clone() for k in ("raw_a", "raw_b", "raw_c")}
        out.update({f"{tag}_x": x64.numpy(), f"{tag}_prices": prices.numpy()})
        out.update({f"{tag}_{k}": v.numpy() for k, v in raws.items()})
        for prec, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            x, py = x64.to(dtype), prices.to(dtype)
            dt = x[1] - x[0]
            yy = ((py[:, 1:] - py[:, :-1]) / py[:, :-1] / dt ** 0.5).t().contiguous()                     # train_utils.py:16-18, [N,T]
            if prec == "f64":
                out[f"{tag}_y"] = yy.numpy()
            for param in ("exp", "cv"):
                lik = VL.VolatilityGaussianLikelihood(K=1, batch_shape=torch.Size([T]), param=param)
                if param == "cv":
                    for k, v in raws.items():
                        setattr(lik, k, torch.nn.Parameter(v.to(dtype)))
                fake = types.SimpleNamespace()
                fake.data_kernel = BM.BMKernel().to(dtype)                                                 # vol = 0.2 default
                fake.inducing_points = x.view(-1, 1)
                fake.variational_mean = torch.nn.Parameter(torch.zeros(n, T, dtype=dtype))
                fake.variational_covar_root = torch.nn.Parameter(torch.eye(n, dtype=dtype))
                fake.index_kernel = IndexKernel(T, dtype=dtype)
                cf0 = fake.index_kernel.covar_factor.detach().clone()
                fake.mean_module = types.SimpleNamespace(
                    base_means=[types.SimpleNamespace(constant=torch.nn.Parameter(torch.zeros(1, dtype=dtype))) for _ in range(T)])
                MT.MultitaskVariationalGP.initialize_variational_parameters(fake, lik, x, y=yy)
                assert torch.equal(fake.index_kernel.covar_factor.detach(), cf0 / 10.)
                key = f"{tag}_{param}_{prec}_"
                out[key + "mean"] = fake.variational_mean.data.numpy()
                out[key + "root"] = fake.variational_covar_root.data.numpy()
                out[key + "const"] = torch.cat([b.constant.data for b in fake.mean_module.base_means]).numpy()
                assert out[key + "mean"].shape == (n, T) and np.isfinite(out[key + "root"]).all()
    path = os.path.join(OUT, "mt_gpcv_cv.npz")
    np.savez_compressed(path, **out)
    print("mt_gpcv_cv.npz", os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
