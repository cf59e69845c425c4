#!/usr/bin/env python3
"""Golden vectors for the copula-process ("cv") half of the GPCV stage, made by EXECUTING the reference's own code:

    voltron/models/single_task_variational_gp.py:204-254   initialize_variational_parameters, the ``param == "cv"`` branch
    voltron/likelihoods/volatility_likelihood.py:43-51     VolatilityGaussianLikelihood.forward  ("cv", K = 1 and K = 5)

behind the gpytorch / botorch stand-ins of ``make_golden_gpcv.py`` (this repository's code, imported from there).
Runs only where the reference is checked out; writes ``gpcv_cv.npz`` next to itself.

Every series is run twice from the same draws of raw_a, raw_b, raw_c: in fp32 (what the product computes in) and in
fp64 (what the fp32 tolerance is judged against); tags ``<name>_f32`` / ``<name>_f64``.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gpcv_cv.py
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(OUT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    mg = _sibling("make_golden_gpcv")                                   # the stand-ins and the loader
    sde_series = _sibling("make_golden").sde_series
    mg._install_standins()
    BM = mg._load("ref_bmkernel", "kernels/BMKernel.py")
    VL = mg._load("ref_vol_likelihood", "likelihoods/volatility_likelihood.py")
    ST = mg._load("ref_stvgp", "models/single_task_variational_gp.py")
    out = {}

    g = torch.Generator().manual_seed(13)
    fs = torch.cat((torch.randn(40, generator=g) * 3.0, torch.tensor([-30.0, -8.0, -2.0, 0.0, 5.0, 40.0])))
    for K in (1, 5):
        torch.manual_seed(100 + K)
        lik = VL.VolatilityGaussianLikelihood(K=K, param="cv")
        out[f"lik{K}_raw"] = torch.stack([lik.raw_a, lik.raw_b, lik.raw_c]).detach().numpy()
        out[f"lik{K}_f"], out[f"lik{K}_scale"] = fs.numpy(), lik.forward(fs).scale.detach().numpy()
        out[f"lik{K}_scale64"] = lik.double().forward(fs.double()).scale.detach().numpy()

    for name, (n, seed, dt_) in {"n60": (60, 2019, 1 / 252.), "n90": (90, 31, 1 / 252.), "n80_wind": (80, 5, 1 / 365.)}.items():
        F, _ = sde_series(n, seed)
        torch.manual_seed(seed)
        raws = VL.VolatilityGaussianLikelihood(K=1, param="cv")
        raw = torch.stack([raws.raw_a, raws.raw_b, raws.raw_c]).detach()                # the class's own draws, fp32
        for dname, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            tag = f"{name}_{dname}"
            lik = VL.VolatilityGaussianLikelihood(K=1, param="cv").to(dtype)
            with torch.no_grad():
                lik.raw_a.copy_(raw[0]), lik.raw_b.copy_(raw[1]), lik.raw_c.copy_(raw[2])
            train_x = (torch.arange(n + 1) * dt_).to(dtype)[:n]
            train_y = torch.tensor(F).to(dtype)
            dt = train_x[1] - train_x[0]
            yy = (train_y[1:] - train_y[:-1]) / train_y[:-1] / dt ** 0.5                # train_utils.py:16-18, restated
            kern = BM.BMKernel().to(dtype)
            fake = types.SimpleNamespace()
            fake.covar_module = kern
            dist = types.SimpleNamespace(variational_mean=torch.nn.Parameter(torch.zeros(n, dtype=dtype)),
                                         chol_variational_covar=torch.nn.Parameter(torch.eye(n, dtype=dtype)))
            fake.variational_strategy = types.SimpleNamespace(inducing_points=train_x.view(-1, 1), _variational_distribution=dist,
                                                              variational_params_initialized=torch.zeros(1))
            fake.mean_module = types.SimpleNamespace(constant=torch.nn.Parameter(torch.zeros(1, dtype=dtype)))
            ST.SingleTaskVariationalGP.initialize_variational_parameters(fake, lik, train_x, y=yy)
            assert float(fake.variational_strategy.variational_params_initialized) == 1.0
            out.update({f"{tag}_x": train_x.numpy(), f"{tag}_prices": train_y.numpy(), f"{tag}_y": yy.numpy(),
                        f"{tag}_raw": raw.numpy(), f"{tag}_mean": dist.variational_mean.data.numpy(),
                        f"{tag}_chol": dist.chol_variational_covar.data.numpy(),
                        f"{tag}_const": fake.mean_module.constant.data.numpy()})
    np.savez_compressed(os.path.join(OUT, "gpcv_cv.npz"), **out)
    print("gpcv_cv.npz", os.path.getsize(os.path.join(OUT, "gpcv_cv.npz")), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
