"""The natural-gradient update of the Markov GPCV (csrc/gpcv_markov_ng.hip) against the ELBO step it stands beside
and against Adam on q, in ONE process: the arms of a comparison alternate, each round is one window of hipGraph replays between
two device events after a warm-up, and the median over the rounds is reported with their minimum and maximum ("spread").
  update      ms per ops.gpcv_markov_natgrad against ms per ops.gpcv_markov_step, inputs resident, "exp" (and "cv" K = 5)
  iteration   ms per captured FitGPCV iteration under optimizer="adam" and "natgrad" (zero_grad, [update,] model(x) ->
              VariationalELBO -> backward, optim.FusedAdam at LR_GPCV), parameters set directly
  reach       on synthetic.sde_batch series of 399 points: Adam's loss after 1000 iterations, the first iteration at which each
              optimizer's eager loop is at or below it, and the wall time of a captured FitGPCV of that many iterations
"clocks_per_point": the update's time x 2.4 GHz / N at 8 x 65536 (one workgroup per series: the series run side by side), next
to the step's -- what the serial pivot chain costs.  Prints ONE JSON line; --out FILE also writes it there.
Usage: bench_gpcv_natgrad.py [--iters K] [--warmup W] [--rounds R] [--shapes 1x399,8x4096] [--out profiles/gpcv_natgrad/bench.json]"""
import argparse
import json
import math
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_gpcv_linear as BL                                     # noqa: E402
from bench_bm_linear import prepare                                # noqa: E402
from bench_gpcv_markov import markov_inputs, markov_step_arm      # noqa: E402
from volt_amd import gp, ops, train_utils                          # noqa: E402
from volt_amd.variational import VariationalELBO, _gauss_hermite, num_gauss_hermite_locs     # noqa: E402

SHAPES = [(1, 399), (64, 399), (8, 4096), (8, 65536)]
KC = BL.KC
CLOCK_GHZ = 2.4


def update_arm(B, N, lik, warmup):
    x, m, y, rho, gam, abc = markov_inputs(B, N)
    abc = abc if lik == "cv" else None
    vol = torch.full((B,), 0.2, device="cuda")
    mu = torch.full((B, N), math.log(0.2), device="cuda")
    gh_x, gh_w = _gauss_hermite(75, x.device)
    lam1, lam2 = (torch.zeros(B, N, dtype=torch.float64, device="cuda") for _ in range(2))
    ws = ops.GpcvMarkovNgWorkspace(B, N, "cuda", KC if abc is not None else 0)
    # (the same q goes in every time: the new one lands in the workspace; at step 1 the sites do not depend on their past)
    run = prepare(lambda: ops.gpcv_markov_natgrad(x, vol, mu, m, rho, gam, y, gh_x, gh_w, lam1, lam2, ws, abc=abc,
                                                  w_ell=1.0 / N, w_kl=1.0 / N), warmup, bool(warmup))
    return run, ws


def iteration_arm(B, N, optimizer, warmup):
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import SingleTaskVariationalGP
    x, m, y, rho, gam, _ = markov_inputs(B, N)
    kw = {"batch_shape": torch.Size([B])} if B > 1 else {}
    lh = VolatilityGaussianLikelihood(param="exp")
    model = SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=lh, use_piv_chol_init=False,
                                    mean_module=gp.ConstantMean(**kw), covar_module=BMKernel(**kw),
                                    learn_inducing_locations=False, use_whitened_var_strat=False, prior_solver="markov").cuda()
    d = model.variational_strategy._variational_distribution
    pick = lambda t: t.clone() if B > 1 else t[0].clone()
    d.variational_mean.data, d.log_diag_precision_root.data, d.coupling.data = pick(m), pick(rho), pick(gam)
    with torch.no_grad():
        model.mean_module.constant.fill_(math.log(0.2))
    yy = pick(y)
    elbo = VariationalELBO(lh, model, N)
    variational = [d.variational_mean, d.log_diag_precision_root, d.coupling]
    params = list(model.parameters())
    if optimizer == "natgrad":
        params = [p for p in params if all(p is not q for q in variational)]
        for q in variational:
            q.requires_grad_(False)
    opt = train_utils._adam([{"params": params}], train_utils.LR_GPCV, True)

    def it():
        opt.zero_grad(set_to_none=True)
        with num_gauss_hermite_locs(75):
            if optimizer == "natgrad":
                elbo.natural_gradient_step(yy)
            loss = -elbo(model(x), yy).sum()
        loss.backward()
        opt.step()
        return loss
    with gp.deferred_checks(immediate=True) as chk:
        it()
        chk.immediate = False
        run = prepare(it, warmup, True)
    return run, chk


def reach(n, seeds):
    """Per series: Adam's 1000-iteration loss and where each optimizer first gets there."""
    from volt_amd.synthetic import sde_batch
    out = []
    _, F, _ = sde_batch(len(seeds), n, seed=seeds[0])
    x = (torch.arange(n, dtype=torch.float32) / 252).cuda()
    for i in range(len(seeds)):
        prices = torch.as_tensor(F[i], dtype=torch.float32).cuda()
        rec = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, _, la = train_utils.FitGPCV(x, prices, train_iters=1000, solver="markov", graph=False)
            la = torch.stack(la).reshape(-1).cpu()
            target = float(la[-1])
            _, _, ln = train_utils.FitGPCV(x, prices, train_iters=1000, solver="markov", optimizer="natgrad", graph=False)
            ln = torch.stack(ln).reshape(-1).cpu()
            rec["adam_loss_at_1000"] = target
            rec["natgrad_loss_at"] = {str(k): float(ln[k - 1]) for k in (1, 10, 50, 200, 1000)}
            rec["adam_loss_at"] = {str(k): float(la[k - 1]) for k in (1, 10, 50, 200, 1000)}
            for name, ls in (("adam", la), ("natgrad", ln)):
                hit = (ls <= target).nonzero()
                count = int(hit[0]) + 1 if len(hit) else None
                rec[name + "_iterations"] = count
                if count is not None:
                    fit = lambda: train_utils.FitGPCV(x, prices, train_iters=count, solver="markov", graph=True,
                                                      **({"optimizer": "natgrad"} if name == "natgrad" else {}))
                    fit()                                          # (the process's first call pays for the library's start-up)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fit()
                    torch.cuda.synchronize()
                    rec[name + "_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gpcv_natgrad.py measures on the MI355X; no GPU, no number")
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s] or SHAPES
    out = {"metric": "ms per call, median of alternating rounds", "measured": True, "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "rounds": a.rounds, "Kc": KC, "update": {}, "iteration": {}, "calls_per_window": {}, "clocks_per_point": {}}
    for B, N in shapes:
        iters = BL.window_calls(a.iters, N)
        for lik in ("exp", "cv"):
            key = f"{B}x{N}/{lik}"
            out["calls_per_window"][key] = iters
            arms = {}
            arms["natgrad"], w1 = update_arm(B, N, lik, a.warmup)
            arms["step"], w2 = markov_step_arm(B, N, lik, a.warmup)
            out["update"][key] = BL.alternate(arms, iters, a.rounds)
            out["clocks_per_point"][key] = {k: round(out["update"][key][k] * 1e-3 * CLOCK_GHZ * 1e9 / N, 1) for k in arms}
            if bool(w1.info.any()) or bool(w2.info.any()):
                out.setdefault("failed", []).append(key)
            del arms, w1, w2
            torch.cuda.empty_cache()
            print(json.dumps({key: out["update"][key]}), file=sys.stderr, flush=True)
        if N <= 4096:
            key = f"{B}x{N}/exp"
            arms, chks = {}, {}
            for optimizer in ("adam", "natgrad"):
                arms[optimizer], chks[optimizer] = iteration_arm(B, N, optimizer, a.warmup)
            out["iteration"][key] = BL.alternate(arms, iters, a.rounds)
            for k, c in chks.items():
                if c.any_bad():
                    out.setdefault("failed", []).append(f"{key}/iteration/{k}")
            del arms, chks
            torch.cuda.empty_cache()
            print(json.dumps({key: out["iteration"][key]}), file=sys.stderr, flush=True)
    out["reach"] = {"N": 399, "series": reach(399, (11, 12, 13))}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
