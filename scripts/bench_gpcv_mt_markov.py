"""The multi-task GPCV step for the Markov variational family (csrc/gpcv_mt_markov.hip) against the dense
multi-task step and the batched single-task Markov step, in ONE process: per shape and likelihood the arms alternate (markov,
dense, single, markov, ...); each round is one window of hipGraph replays between two device events after a warm-up; the median
over the rounds is reported with their minimum and maximum ("spread": a difference smaller than it is not a difference).  The
method and the window sizes are scripts/bench_gpcv_markov.py's.
  step       the raw ELBO + gradient step with its inputs resident:
               markov  ops.gpcv_mt_markov_step at (N, T)
               dense   ops.gpcv_mt_step at the same (N, T) (the dense joint model: K + j I factored, a dense N x N root)
               single  ops.gpcv_markov_step at B = T (T independent single-task Markov models: no task covariance)
  iteration  one captured trainer iteration (model(x) -> VariationalELBO -> backward) of MultitaskVariationalGP with
             prior_solver = "markov" / "dense", parameters set directly
The three arms are three models: what is compared is the cost of a step at a shape, not its value.  65536 x 8 runs the two
Markov arms only (the dense arm's N x N arrays do not fit).  Likelihoods: "exp", and "cv" with K = 5.  Prints ONE JSON line.
Usage: bench_gpcv_mt_markov.py [--iters K] [--warmup W] [--rounds R] [--shapes 399x8,4096x64]
       bench_gpcv_mt_markov.py --trace N T [STEPS]   # eager markov steps, nothing timed: for rocprofv3 --kernel-trace --stats"""
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

SHAPES = [(399, 8), (399, 64), (4096, 8), (4096, 64), (65536, 8)]
MARKOV_ONLY = {(65536, 8)}
KC = BL.KC


def inputs(N, T, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    u = lambda *s: torch.rand(*s, device="cuda", generator=g)
    x = torch.arange(N, device="cuda", dtype=torch.float32) / 252
    M = math.log(0.2) + 0.3 * r(N, T)
    return dict(x=x, M=M, y=r(N, T) * M.exp(), rho=3.0 + 0.1 * r(N), gam=-0.5 + 0.1 * r(N),
                Lt=(torch.eye(T, device="cuda") + 0.1 * r(T, T)).tril(), c=torch.full((T,), math.log(0.2), device="cuda"),
                cf=0.1 * r(T), rv=torch.zeros(T, device="cuda"),
                abc=torch.stack([u(T, KC) + 0.3, 0.1 + 0.1 * u(T, KC), u(T, KC)], 1))


def step_arms(N, T, lik, dense, warmup):
    p = inputs(N, T)
    abc = p["abc"] if lik == "cv" else None
    gx, gw = _gauss_hermite(75, p["x"].device)
    vol = torch.full((1,), 0.2, device="cuda")
    kw = dict(w_ell=1.0 / N, w_kl=1.0 / (N * T))
    keep = [p]
    wm = ops.GpcvMtMarkovWorkspace(N, T, "cuda", KC if abc is not None else 0)
    arms = {"markov": prepare(lambda: ops.gpcv_mt_markov_step(p["x"], vol, p["M"], p["c"], p["rho"], p["gam"], p["Lt"], p["cf"], p["rv"],
                                                              p["y"], gx, gw, wm, abc=abc, **kw), warmup, bool(warmup))}
    if dense:
        K = 0.2 * torch.minimum(p["x"][:, None], p["x"][None, :])
        Lx = (0.05 * torch.eye(N, device="cuda") + 0.001 * torch.randn(N, N, device="cuda")).tril()
        wd = ops.GpcvMtWorkspace(N, T, False, torch.device("cuda"), KC if abc is not None else 0)
        keep += [K, Lx, wd]
        arms["dense"] = prepare(lambda: ops.gpcv_mt_step(K, p["M"], p["c"], Lx, p["Lt"], p["cf"], p["rv"], p["y"], gx, gw, wd, abc=abc,
                                                         **kw), warmup, bool(warmup))
    # T independent single-task Markov models over the same grid
    m1, y1 = p["M"].t().contiguous(), p["y"].t().contiguous()
    rho1, gam1 = p["rho"].expand(T, N).contiguous(), p["gam"].expand(T, N).contiguous()
    vols = torch.full((T,), 0.2, device="cuda")
    ws1 = ops.GpcvMarkovWorkspace(T, N, "cuda", KC if abc is not None else 0)
    resid = m1 - math.log(0.2)
    arms["single"] = prepare(lambda: ops.gpcv_markov_step(p["x"], vols, resid, m1, rho1, gam1, y1, gx, gw, ws1, abc=abc,
                                                          w_ell=1.0 / N, w_kl=1.0 / N), warmup, bool(warmup))
    keep += [wm, ws1, m1, y1, rho1, gam1, resid]
    return arms, keep


def iteration_arm(N, T, lik, solver, warmup):
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import MultitaskVariationalGP
    p = inputs(N, T)
    torch.manual_seed(0)
    lh = VolatilityGaussianLikelihood(param="exp") if lik == "exp" else \
        VolatilityGaussianLikelihood(K=KC, param="cv", batch_shape=torch.Size([T])).cuda()
    model = MultitaskVariationalGP(p["x"], num_tasks=T, covar_module=BMKernel(), prior_solver=solver).cuda()
    with torch.no_grad():
        model.variational_mean.copy_(p["M"])
        model.variational_task_covar_root.copy_(p["Lt"])
        if solver == "markov":
            model.log_diag_precision_root.copy_(p["rho"])
            model.coupling.copy_(p["gam"])
        else:
            model.variational_covar_root.copy_(0.05 * torch.eye(N, device="cuda"))
        for m in model.mean_module.base_means:
            m.constant.fill_(math.log(0.2))
    elbo = VariationalELBO(lh, model, N * T)
    params = list(model.parameters())

    def it():
        for q in params:
            q.grad = None
        with num_gauss_hermite_locs(75):
            loss = -elbo(model(p["x"]), p["y"])
        loss.backward()
        return loss
    with gp.deferred_checks(immediate=True) as chk:
        it()
        chk.immediate = False
        run = prepare(it, warmup, True)
    return run, chk


def trace(N, T, steps):
    for lik in ("exp", "cv"):
        arms, keep = step_arms(N, T, lik, False, 0)
        for _ in range(2 + steps):
            arms["markov"].fn()
        torch.cuda.synchronize()
    print(f"traced {2 + steps} multi-task markov steps, exp and cv, at N={N} T={T}")


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
        raise SystemExit("bench_gpcv_mt_markov.py measures on the MI355X; no GPU, no number")
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s] or SHAPES
    out = {"metric": "ms per call, median of alternating rounds", "measured": True, "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "rounds": a.rounds, "Kc": KC, "step": {}, "iteration": {}, "calls_per_window": {}}
    for N, T in shapes:
        for lik in ("exp", "cv"):
            key = f"{N}x{T}/{lik}"
            iters = BL.window_calls(a.iters, N)
            out["calls_per_window"][key] = iters
            arms, keep = step_arms(N, T, lik, (N, T) not in MARKOV_ONLY, a.warmup)
            out["step"][key] = BL.alternate(arms, iters, a.rounds)
            del arms, keep
            torch.cuda.empty_cache()
            arms, chks = {}, {}
            for solver in ("markov", "dense"):
                if solver == "dense" and (N, T) in MARKOV_ONLY:
                    continue
                arms[solver], chks[solver] = iteration_arm(N, T, lik, solver, a.warmup)
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
