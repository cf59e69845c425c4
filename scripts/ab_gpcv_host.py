#!/usr/bin/env python
"""A/B of the GPCV host layer (ops.gpcv_*_step and the Gpcv*Workspace classes, variational._GPCV*Elbo and VariationalELBO,
train_utils.FitGPCV / FitGPCVMultitask) between two checkouts: the same bits out, the same exceptions.

    python scripts/ab_gpcv_host.py --tree <checkout> --out digests.json     # SHA-256 of every case
    python scripts/ab_gpcv_host.py --compare a.json b.json                  # exit 1 unless every digest is equal

One process imports ONE volt_amd, so run it once per checkout (``--tree``: the checkout whose volt_amd is imported, default this
one; it must be built).  Only public names are used, so it runs on either side of a change to the layer.  The cases:
  elbo/      the ELBO and the .grad of every model and likelihood parameter, by name: dense with BMKernel (closed-form scale
             gradient) and FBMKernel (grad_K), prior_solver "linear" and "markov", MultitaskVariationalGP with bm and fbm;
             "exp", "cv" with Kc in {1, 5} -- single-task: a shared [Kc] likelihood and a batched [B,Kc] one; N in {1, 5, 33, 130};
             B in {1 (unbatched), 3}, T in {1, 3}; loss = -elbo (summed), and for a batch (w * elbo).sum(), w = [0.5, -2, 3]
  fit/       FitGPCV (every solver, "exp" and "cv" K = 1 with train_likelihood, unbatched and [3,N+1] prices) and
             FitGPCVMultitask at N = 33 for 8 iterations, eager and graph=True: the losses and the final state_dict
  rsample/   every latent class on fixed base_samples, unbatched and batched
  fail/      by exception type and text: a negative vol, a NaN in variational_mean, Kc = 9 at the four ops steps, a likelihood
             whose batch shape is not the model's
NaNs are canonicalised before hashing; nothing else is.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES, W = (1, 5, 33, 130), (0.5, -2.0, 3.0)
RAISED = {}                                   # exception type -> cases that ended in it (reported beside the digests)


def digest(t):
    a = t.detach().cpu().contiguous().numpy() if hasattr(t, "detach") else np.asarray(t)
    if a.dtype.kind == "f":
        a = np.where(np.isnan(a), np.array(np.nan, dtype=a.dtype), a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + np.ascontiguousarray(a).tobytes()).hexdigest()


def digest_cases(torch, dev):
    from volt_amd import gp, ops
    from volt_amd.kernels import BMKernel, FBMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood as Lik
    from volt_amd.models import MultitaskVariationalGP, SingleTaskVariationalGP
    from volt_amd.train_utils import FitGPCV, FitGPCVMultitask
    from volt_amd.variational import VariationalELBO, _gauss_hermite, num_gauss_hermite_locs
    out = {}

    def case(name, fn):
        """fn() -> {key: tensor or value} to hash."""
        try:
            res = {k: digest(v) if hasattr(v, "shape") else repr(v) for k, v in fn().items()}
        except Exception as e:                                                # noqa: BLE001 -- the exception IS the result
            res = {"raised": f"{type(e).__name__}: {e}"}
            RAISED[type(e).__name__] = RAISED.get(type(e).__name__, 0) + 1
            print("raised", name, res["raised"][:160], file=sys.stderr, flush=True)
        torch.cuda.synchronize()
        out[name] = hashlib.sha256(json.dumps(res, sort_keys=True).encode()).hexdigest()

    class NegBM(BMKernel):                                                    # a prior no step can factor
        vol = property(lambda self: -torch.sigmoid(self.raw_vol), BMKernel.vol.fset)

    def rand(g, *shape, scale=1.0):
        return (scale * torch.randn(*shape, generator=g)).to(dev)

    def grid(n):
        return (torch.arange(1, n + 1, dtype=torch.float32) / 32.0).to(dev)

    def likelihood(lik, batch):
        """lik: "exp" | ("cv", Kc, batch shape or None)."""
        torch.manual_seed(7)
        if lik == "exp":
            return Lik(param="exp")
        return Lik(K=lik[1], param="cv", **({"batch_shape": torch.Size(lik[2])} if lik[2] else {})).to(dev)

    def single(family, n, B, lik, kernel=None):
        g = torch.Generator().manual_seed(100 + n)
        x, kw, bs = grid(n), ({"batch_shape": torch.Size([B])} if B else {}), ((B,) if B else ())
        solver = family if family in ("linear", "markov") else "dense"
        kernel = kernel or (FBMKernel if family == "dense-fbm" else BMKernel)
        lh = likelihood(lik, B)
        model = SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=lh, use_piv_chol_init=False,
                                        mean_module=gp.ConstantMean(**kw), covar_module=kernel(**kw),
                                        learn_inducing_locations=False, use_whitened_var_strat=False, prior_solver=solver).to(dev)
        d = model.variational_strategy._variational_distribution
        with torch.no_grad():
            d.variational_mean.data = -1.0 + rand(g, *bs, n, scale=0.3)
            if solver == "markov":
                d.log_diag_precision_root.data, d.coupling.data = rand(g, *bs, n, scale=0.3), rand(g, *bs, n, scale=0.3)
            else:
                d.chol_variational_covar.data = 0.5 * torch.eye(n, device=dev) + rand(g, *bs, n, n, scale=0.1).tril()
            model.mean_module.constant.copy_(-0.9 + rand(g, *model.mean_module.constant.shape, scale=0.2))
            model.covar_module.raw_vol.copy_(rand(g, *model.covar_module.raw_vol.shape, scale=0.5))
        return model, lh, x, rand(g, *bs, n, scale=0.2), n

    def multi(kernel, n, T, lik):
        g = torch.Generator().manual_seed(200 + n)
        torch.manual_seed(8)
        x, lh = grid(n), likelihood(lik, T)
        model = MultitaskVariationalGP(x, num_tasks=T, covar_module=kernel()).to(dev)
        with torch.no_grad():
            model.variational_mean.copy_(-1.0 + rand(g, n, T, scale=0.3))
            model.variational_covar_root.add_(rand(g, n, n, scale=0.1).tril())
            model.variational_task_covar_root.add_(rand(g, T, T, scale=0.1).tril())
        return model, lh, x, rand(g, n, T, scale=0.2), n * T

    def params(model, lh):
        ps = dict(model.named_parameters())
        ps.update({"likelihood." + k: p for k, p in lh.named_parameters() if all(p is not q for q in ps.values())})
        return ps

    def elbo_and_grads(built, weighted):
        model, lh, x, yy, num_data = built()
        ps = params(model, lh)
        for p in ps.values():
            p.requires_grad_(True)
        with num_gauss_hermite_locs(75):
            val = VariationalELBO(lh, model, num_data)(model(x), yy)
        loss = (torch.tensor(W, device=dev) * val).sum() if weighted else -(val.sum() if val.ndim else val)
        loss.backward()
        return {"elbo": val, **{"grad:" + k: (p.grad if p.grad is not None else "None") for k, p in ps.items()}}

    def lik_name(lik):
        return lik if lik == "exp" else f"cv{lik[1]}-" + ("x".join(map(str, lik[2])) if lik[2] else "shared")

    # ---- elbo/
    for n in SIZES:
        print("elbo N", n, file=sys.stderr, flush=True)
        for family in ("dense-bm", "dense-fbm", "linear", "markov"):
            for B in (0, 3):
                liks = ["exp"] + [("cv", Kc, bs) for Kc in (1, 5) for bs in ((None, (B,)) if B else (None,))]
                for lik in liks:
                    for weighted in ((False, True) if B else (False,)):
                        case(f"elbo/{family}/N{n}/B{B or 1}/{lik_name(lik)}/{'weighted' if weighted else 'neg'}",
                             lambda: elbo_and_grads(lambda: single(family, n, B, lik), weighted))
        for kname, kernel in (("bm", BMKernel), ("fbm", FBMKernel)):
            for T in (1, 3):
                for lik in ("exp", ("cv", 1, (T,)), ("cv", 5, (T,))):
                    case(f"elbo/multitask-{kname}/N{n}/T{T}/{lik_name(lik)}/neg",
                         lambda: elbo_and_grads(lambda: multi(kernel, n, T, lik), False))

    # ---- fit/
    n = 33
    gp_ = torch.Generator().manual_seed(5)
    prices = (100.0 * torch.exp(torch.cumsum(0.01 * torch.randn(3, n + 1, generator=gp_), -1))).to(dev)
    tx = (torch.arange(n, dtype=torch.float32) / 252.0).to(dev)

    def fitted(fit, train_y, **kw):
        torch.manual_seed(9)
        model, lh, losses = fit(tx, train_y, train_iters=8, **kw)
        res = {"losses": torch.stack([l.reshape(-1) for l in losses]) if losses else "none", "n_losses": len(losses)}
        res.update({"model." + k: v for k, v in model.state_dict().items()})
        res.update({"lik." + k: v for k, v in lh.state_dict().items()})
        return res
    print("fit", file=sys.stderr, flush=True)
    for graph in (False, True):
        for param, kw in (("exp", {}), ("cv", dict(param="cv", K=1, train_likelihood=True))):
            for solver in ("dense", "linear", "markov"):
                for tag, y in (("unbatched", prices[0]), ("batched", prices)):
                    case(f"fit/FitGPCV/{solver}/{param}/{tag}/{'graph' if graph else 'eager'}",
                         lambda: fitted(FitGPCV, y, graph=graph, solver=solver, **kw))
            case(f"fit/FitGPCVMultitask/{param}/{'graph' if graph else 'eager'}",
                 lambda: fitted(FitGPCVMultitask, prices, graph=graph, **kw))

    # ---- rsample/
    for B in (0, 3):
        for family in ("dense-bm", "markov"):
            def draw():
                model, _, x, _, _ = single(family, 33, B, "exp")
                eps = rand(torch.Generator().manual_seed(3), 4, *((B,) if B else ()), 33)
                return {"f": model(x).rsample(base_samples=eps)}
            case(f"rsample/{family}/B{B or 1}", draw)

    def draw_mt():
        model, _, x, _, _ = multi(BMKernel, 33, 3, "exp")
        return {"f": model(x).rsample(base_samples=rand(torch.Generator().manual_seed(3), 4, 33, 3))}
    case("rsample/multitask", draw_mt)

    # ---- fail/
    def broken(build, how):
        def fn():
            model, lh, x, yy, num_data = build()
            if how == "nan":
                vm = model.variational_mean if hasattr(model, "variational_mean") else \
                    model.variational_strategy._variational_distribution.variational_mean
                with torch.no_grad():
                    vm.view(-1)[vm.numel() // 2] = float("nan")
            return elbo_and_grads(lambda: (model, lh, x, yy, num_data), False)
        return fn
    for family in ("dense-bm", "linear", "markov"):
        for B in (0, 3):
            case(f"fail/negative-vol/{family}/B{B or 1}", broken(lambda: single(family, 33, B, "exp", kernel=NegBM), None))
            case(f"fail/nan-mean/{family}/B{B or 1}", broken(lambda: single(family, 33, B, ("cv", 2, None)), "nan"))
        case(f"fail/lik-batch/{family}", broken(lambda: single(family, 33, 3, ("cv", 2, (2,))), None))
    case("fail/nan-mean/dense-fbm/B3", broken(lambda: single("dense-fbm", 33, 3, "exp"), "nan"))
    for lik in ("exp", ("cv", 2, (3,))):
        case(f"fail/negative-vol/multitask/{lik_name(lik)}", broken(lambda: multi(NegBM, 33, 3, lik), None))
        case(f"fail/nan-mean/multitask/{lik_name(lik)}", broken(lambda: multi(BMKernel, 33, 3, lik), "nan"))
    case("fail/lik-batch/multitask", broken(lambda: multi(BMKernel, 33, 3, ("cv", 2, (2,))), None))

    n, B, T = 5, 2, 2
    g = torch.Generator().manual_seed(4)
    gh_x, gh_w = _gauss_hermite(20, dev)
    x, vol, eye = grid(n), torch.full((B,), 0.3, device=dev), torch.eye(n, device=dev)
    K = (torch.minimum(x[:, None], x[None, :]) * 0.3).expand(B, n, n).contiguous()
    r, m, y, Lq = rand(g, B, n), rand(g, B, n), rand(g, B, n), eye.expand(B, n, n).contiguous()
    abc9, abc9t = torch.ones(B, 3, 9, device=dev), torch.ones(T, 3, 9, device=dev)
    case("fail/Kc9/gpcv_cv_step", lambda: {"info": ops.gpcv_cv_step(K, r, m, Lq, y, abc9, gh_x, gh_w).info})
    case("fail/Kc9/gpcv_bm_step", lambda: {"info": ops.gpcv_bm_step(x, vol, r, m, Lq, y, gh_x, gh_w, abc=abc9).info})
    case("fail/Kc9/gpcv_markov_step",
         lambda: {"info": ops.gpcv_markov_step(x, vol, r, m, 0 * m, 0 * m, y, gh_x, gh_w, abc=abc9).info})
    case("fail/Kc9/gpcv_mt_step",
         lambda: {"info": ops.gpcv_mt_step(K[0], rand(g, n, T), torch.zeros(T, device=dev), eye, torch.eye(T, device=dev),
                                           torch.ones(T, device=dev), torch.zeros(T, device=dev), rand(g, n, T), gh_x, gh_w,
                                           abc=abc9t).info})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--out", help="write the digests to this JSON file")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        A, B = (json.load(open(f)) for f in a.compare)
        bad = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
        print(f"{len(A)} and {len(B)} digests, {len(bad)} differ")
        for k in sorted(set(A) | set(B)):
            print("  ", "DIFFERS" if k in bad else "same   ", k, A.get(k, "-")[:16], B.get(k, "-")[:16])
        sys.exit(1 if bad or not A else 0)
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    d = digest_cases(torch, torch.device("cuda"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(d, fh, indent=0, sort_keys=True)
    print(json.dumps({"tree": os.path.abspath(a.tree), "digests": len(d), "cases_that_end_in_an_exception": RAISED,
                      "all": hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest()}))


if __name__ == "__main__":
    main()
