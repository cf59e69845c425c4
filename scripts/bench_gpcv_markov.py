"""The O(N) GPCV step for the Markov variational family (csrc/gpcv_markov.hip) against the dense and the O(N^2)
("linear") steps, in ONE process: per shape and likelihood the arms alternate (dense, linear, markov, dense, ...); each round is
one window of hipGraph replays between two device events after a warm-up; the median over the rounds is reported with their
minimum and maximum ("spread": a difference smaller than it is not a difference).  The method, the inputs of the dense and
linear arms and the window sizes are scripts/bench_gpcv_linear.py's.
  step       the raw ELBO + gradient step with its inputs resident (ops.gpcv_step / gpcv_cv_step, ops.gpcv_bm_step,
             ops.gpcv_markov_step)
  iteration  one captured trainer iteration (model(x) -> VariationalELBO -> backward) of SingleTaskVariationalGP with
             prior_solver = "dense" / "linear" / "markov", parameters set directly
The three solvers are three models (another variational family; "markov" another prior jitter): what is compared is the cost of
a step at a shape, not its value.  32 x 16384 runs linear and markov only, 8 x 65536 markov only (the others' N x N arrays do
not fit); an arm that runs out of memory is listed under "not_run".  "clocks_per_point": the markov step's time x 2.4 GHz / N for a single series -- the figure the chain kernels are
judged by.  Likelihoods: "exp", and "cv" with K = 5.  Prints ONE JSON line.
Usage: bench_gpcv_markov.py [--iters K] [--warmup W] [--rounds R] [--shapes 1x399,8x4096]
       bench_gpcv_markov.py --trace B N [STEPS]     # eager markov steps, nothing timed: for rocprofv3 --kernel-trace --stats"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_gpcv_linear as BL                                     # noqa: E402
from bench_bm_linear import prepare                                # noqa: E402
from volt_amd import gp, ops                                       # noqa: E402
from volt_amd.variational import VariationalELBO, _gauss_hermite, num_gauss_hermite_locs     # noqa: E402

SHAPES = [(1, 399), (64, 399), (1, 4096), (8, 4096), (32, 4096), (32, 16384), (8, 65536)]
NO_DENSE = {(32, 16384), (8, 65536)}
MARKOV_ONLY = {(8, 65536)}
KC = BL.KC
CLOCK_GHZ = 2.4


def markov_inputs(B, N, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.arange(N, device="cuda", dtype=torch.float32) / 252
    m = math.log(0.2) + 0.3 * torch.randn(B, N, device="cuda", generator=g)
    y = torch.randn(B, N, device="cuda", generator=g) * m.exp()
    rho = 3.0 + 0.1 * torch.randn(B, N, device="cuda", generator=g)
    gam = -0.5 + 0.1 * torch.randn(B, N, device="cuda", generator=g)
    abc = torch.stack([torch.rand(B, KC, device="cuda", generator=g) + 0.3, 0.1 + 0.1 * torch.rand(B, KC, device="cuda", generator=g),
                       torch.rand(B, KC, device="cuda", generator=g)], 1)
    return x, m, y, rho, gam, abc


def markov_step_arm(B, N, lik, warmup):
    x, m, y, rho, gam, abc = markov_inputs(B, N)
    abc = abc if lik == "cv" else None
    vol = torch.full((B,), 0.2, device="cuda")
    resid = m - math.log(0.2)
    gh_x, gh_w = _gauss_hermite(75, x.device)
    ws = ops.GpcvMarkovWorkspace(B, N, "cuda", KC if abc is not None else 0)
    run = prepare(lambda: ops.gpcv_markov_step(x, vol, resid, m, rho, gam, y, gh_x, gh_w, ws, abc=abc, w_ell=1.0 / N, w_kl=1.0 / N),
                  warmup, bool(warmup))
    return run, ws


def markov_iteration_arm(B, N, lik, warmup):
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import SingleTaskVariationalGP
    x, m, y, rho, gam, _ = markov_inputs(B, N)
    kw = {"batch_shape": torch.Size([B])} if B > 1 else {}
    torch.manual_seed(0)
    lh = VolatilityGaussianLikelihood(param="exp") if lik == "exp" else VolatilityGaussianLikelihood(K=KC, param="cv", **kw).cuda()
    model = SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=lh, use_piv_chol_init=False,
                                    mean_module=gp.ConstantMean(**kw), covar_module=BMKernel(**kw),
                                    learn_inducing_locations=False, use_whitened_var_strat=False, prior_solver="markov").cuda()
    d = model.variational_strategy._variational_distribution
    pick = lambda t: t if B > 1 else t[0]
    d.variational_mean.data, d.log_diag_precision_root.data, d.coupling.data = pick(m), pick(rho), pick(gam)
    with torch.no_grad():
        model.mean_module.constant.fill_(math.log(0.2))
    yy = pick(y)
    elbo = VariationalELBO(lh, model, N)
    params = list(model.parameters())

    def it():
        for p in params:
            p.grad = None
        with num_gauss_hermite_locs(75):
            loss = -elbo(model(x), yy).sum()
        loss.backward()
        return loss
    with gp.deferred_checks(immediate=True) as chk:
        it()
        chk.immediate = False
        run = prepare(it, warmup, True)
    return run, chk


def trace(B, N, steps):
    for lik in ("exp", "cv"):
        run, ws = markov_step_arm(B, N, lik, 0)
        for _ in range(2 + steps):
            run.fn()
        torch.cuda.synchronize()
    print(f"traced {2 + steps} markov steps, exp and cv, at B={B} N={N}")


def main():
    if "--trace" in sys.argv:
        rest = [int(v) for v in sys.argv[sys.argv.index("--trace") + 1:]]
        return trace(rest[0], rest[1], rest[2] if len(rest) > 2 else 5)
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gpcv_markov.py measures on the MI355X; no GPU, no number")
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s] or SHAPES
    out = {"metric": "ms per call, median of alternating rounds", "measured": True, "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "rounds": a.rounds, "Kc": KC, "step": {}, "iteration": {}, "calls_per_window": {}, "clocks_per_point": {}}
    for B, N in shapes:
        for lik in ("exp", "cv"):
            key = f"{B}x{N}/{lik}"
            iters = BL.window_calls(a.iters, N)
            out["calls_per_window"][key] = iters
            arms, keep = {}, []
            if (B, N) not in MARKOV_ONLY:
                arms, keep = BL.step_arms(B, N, lik, (B, N) not in NO_DENSE, a.warmup)
            arms["markov"], ws = markov_step_arm(B, N, lik, a.warmup)
            out["step"][key] = BL.alternate(arms, iters, a.rounds)
            if B == 1 or (B, N) in MARKOV_ONLY:
                out["clocks_per_point"][key] = round(out["step"][key]["markov"] * 1e-3 * CLOCK_GHZ * 1e9 / N, 1)
            del arms, keep, ws
            torch.cuda.empty_cache()
            arms, chks = {}, {}
            for solver in ("dense", "linear"):
                if (B, N) in MARKOV_ONLY or (solver == "dense" and (B, N) in NO_DENSE):
                    continue
                try:
                    arms[solver], chks[solver] = BL.iteration_arm(B, N, lik, solver, a.warmup)
                except torch.OutOfMemoryError as e:        # (the linear iteration at 32 x 16384 holds five [B,N,N] arrays)
                    out.setdefault("not_run", {})[f"{key}/iteration/{solver}"] = "out of memory: " + str(e)[:120]
                    torch.cuda.empty_cache()
            arms["markov"], chks["markov"] = markov_iteration_arm(B, N, lik, a.warmup)
            out["iteration"][key] = BL.alternate(arms, iters, a.rounds)
            for solver, c in chks.items():
                if c.any_bad():                            # reported, not hidden: the timing of a failed step means nothing
                    out.setdefault("failed_steps", {})[f"{key}/{solver}"] = [t.tolist()[:8] for t in c._acc.values()]
            del arms, chks
            torch.cuda.empty_cache()
            print(json.dumps({key: {k: out[k].get(key) for k in ("step", "iteration")}}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
