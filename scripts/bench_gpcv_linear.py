"""The GPCV ELBO step for the Brownian-motion prior on the O(N^2) path (csrc/gpcv_bm.hip) against the dense step, in ONE process:
per shape and likelihood the two arms alternate (dense, linear, dense, linear, ...); each round is one window of calls between
two device events after a warm-up, every call a hipGraph replay, and the median over the rounds is reported WITH their minimum
and maximum ("spread": a difference smaller than it is not a difference).  A window holds `iters` calls at N >= 4096 and is
scaled up for shorter series (x 10 at N = 399) so that it lasts tens of milliseconds, not a few.
  step       the raw ELBO + gradient step with its inputs resident: ops.gpcv_step / ops.gpcv_cv_step (K = vol min(x, x') filled
             beforehand) against ops.gpcv_bm_step
  iteration  one trainer iteration (model(x) -> VariationalELBO -> backward) of SingleTaskVariationalGP, prior_solver="dense" /
             "linear", parameters set directly (the start-up values are dense either way and not what is measured)
  sweep      the column-sweep kernel's share: its minimum traffic (tril(Lq) read twice, the packed fp64 z written and read,
             grad_Lq written whole) over the linear step's time -- a LOWER bound on its bytes/s (the step also runs the row
             kernel and the O(N) chain); the kernel's own time comes from a `rocprofv3 --kernel-trace --stats` run
32 x 16384 runs the linear arm's raw step only: the dense step's K, Lq, gradient and workspace would need > 300 GB.
Likelihoods: "exp", and "cv" with K = 5.  Prints ONE JSON line.
Usage: bench_gpcv_linear.py [--iters K] [--warmup W] [--rounds R] [--shapes 1x399,8x4096] [--no-large]
       bench_gpcv_linear.py --trace B N [STEPS]     # warm-up + STEPS eager raw steps of each arm and likelihood, nothing timed:
                                                    # for rocprofv3 --kernel-trace --stats -- python ... (the kernels' own times)"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_bm_linear import prepare, window                        # noqa: E402
from volt_amd import gp, ops                                       # noqa: E402
from volt_amd.variational import VariationalELBO, _gauss_hermite, num_gauss_hermite_locs     # noqa: E402

SHAPES = [(1, 399), (64, 399), (1, 4096), (8, 4096), (32, 4096)]
LINEAR_ONLY = [(32, 16384)]
KC = 5


def alternate(arms, iters, rounds):
    """arms: {name: callable}; round-robin over the arms, `rounds` windows each; median, and [min, max], ms per call."""
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, run in arms.items():
            times[k].append(window(run, iters))
    out = {k: round(statistics.median(v), 5) for k, v in times.items()}
    out["spread"] = {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()}
    return out


def window_calls(iters, N):
    """Calls per window: `iters` from N = 4096 on (a quarter beyond), more for short series, whose calls take ~0.1 ms."""
    if N > 4096:
        return max(iters // 4, 3)
    return iters * max(1, min(10, 4096 // N))


def inputs(B, N, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.arange(N, device="cuda", dtype=torch.float32) / 252
    m = math.log(0.2) + 0.3 * torch.randn(B, N, device="cuda", generator=g)
    y = torch.randn(B, N, device="cuda", generator=g) * m.exp()
    Lq = torch.empty(B, N, N, device="cuda")
    for b in range(B):                                              # (series by series: no second [B,N,N] temporary)
        Lq[b] = (0.3 / math.sqrt(N)) * torch.randn(N, N, device="cuda", generator=g)
        Lq[b].tril_()
        Lq[b].diagonal().copy_(0.05 + 0.3 * torch.rand(N, device="cuda", generator=g))
    abc = torch.stack([torch.rand(B, KC, device="cuda", generator=g) + 0.3, 0.1 + 0.1 * torch.rand(B, KC, device="cuda", generator=g),
                       torch.rand(B, KC, device="cuda", generator=g)], 1)
    return x, m, y, Lq, abc


def step_arms(B, N, lik, dense, warmup):
    x, m, y, Lq, abc = inputs(B, N)
    abc = abc if lik == "cv" else None
    vol = torch.full((B,), 0.2, device="cuda")
    resid = m - math.log(0.2)
    gh_x, gh_w = _gauss_hermite(75, x.device)
    kw = dict(w_ell=1.0 / N, w_kl=1.0 / N)
    arms, keep = {}, []
    wl = ops.GpcvBmWorkspace(B, N, "cuda", KC if abc is not None else 0)
    arms["linear"] = prepare(lambda: ops.gpcv_bm_step(x, vol, resid, m, Lq, y, gh_x, gh_w, wl, abc=abc, **kw), warmup, bool(warmup))
    keep.append(wl)
    if dense:
        K = (0.2 * torch.minimum(x[:, None], x[None, :])).expand(B, N, N).contiguous()
        wd = ops.GpcvWorkspace(B, N, False, "cuda", Kc=KC if abc is not None else 0)
        if abc is None:
            arms["dense"] = prepare(lambda: ops.gpcv_step(K, resid, m, Lq, y, gh_x, gh_w, wd, **kw), warmup, bool(warmup))
        else:
            arms["dense"] = prepare(lambda: ops.gpcv_cv_step(K, resid, m, Lq, y, abc, gh_x, gh_w, wd, **kw), warmup, bool(warmup))
        keep.append(wd)
    return arms, keep


def iteration_arm(B, N, lik, solver, warmup):
    from volt_amd.kernels import BMKernel
    from volt_amd.likelihoods import VolatilityGaussianLikelihood
    from volt_amd.models import SingleTaskVariationalGP
    x, m, y, Lq, _ = inputs(B, N)
    kw = {"batch_shape": torch.Size([B])} if B > 1 else {}
    torch.manual_seed(0)
    lh = VolatilityGaussianLikelihood(param="exp") if lik == "exp" else VolatilityGaussianLikelihood(K=KC, param="cv", **kw).cuda()
    model = SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=lh, use_piv_chol_init=False,
                                    mean_module=gp.ConstantMean(**kw), covar_module=BMKernel(**kw),
                                    learn_inducing_locations=False, use_whitened_var_strat=False, prior_solver=solver).cuda()
    d = model.variational_strategy._variational_distribution
    d.variational_mean.data = m if B > 1 else m[0]
    d.chol_variational_covar.data = Lq if B > 1 else Lq[0]
    with torch.no_grad():
        model.mean_module.constant.fill_(math.log(0.2))
    yy = y if B > 1 else y[0]
    elbo = VariationalELBO(lh, model, N)
    params = list(model.parameters())

    def it():
        for p in params:
            p.grad = None
        with num_gauss_hermite_locs(75):
            loss = -elbo(model(x), yy).sum()
        loss.backward()
        return loss
    with gp.deferred_checks(immediate=True) as chk:   # (a replay needs no context: the captured step notes into chk's words)
        it()
        chk.immediate = False
        run = prepare(it, warmup, True)
    return run, chk


def trace(B, N, steps):
    for lik in ("exp", "cv"):
        arms, keep = step_arms(B, N, lik, True, 0)
        for _ in range(2 + steps):
            for run in arms.values():
                run.fn()
        torch.cuda.synchronize()
    print(f"traced {2 + steps} dense and linear steps, exp and cv, at B={B} N={N}")


def sweep_bytes(B, N):
    tri = B * N * (N + 1) // 2
    return 2 * 4 * tri + 2 * 8 * tri + 4 * B * N * N


def main():
    if "--trace" in sys.argv:
        rest = [int(v) for v in sys.argv[sys.argv.index("--trace") + 1:]]
        return trace(rest[0], rest[1], rest[2] if len(rest) > 2 else 5)
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="")
    ap.add_argument("--no-large", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gpcv_linear.py measures on the MI355X; no GPU, no number")
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s] or SHAPES + ([] if a.no_large else LINEAR_ONLY)
    out = {"metric": "ms per call, median of alternating rounds", "measured": True, "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "rounds": a.rounds, "Kc": KC, "step": {}, "iteration": {}, "calls_per_window": {}}
    for B, N in shapes:
        dense = (B, N) not in LINEAR_ONLY
        for lik in ("exp", "cv"):
            key = f"{B}x{N}/{lik}"
            iters = window_calls(a.iters, N)
            out["calls_per_window"][key] = iters
            arms, keep = step_arms(B, N, lik, dense, a.warmup)
            st = alternate(arms, iters, a.rounds)
            st["sweep_min_GBps"] = round(sweep_bytes(B, N) / (st["linear"] * 1e-3) / 1e9, 1)
            out["step"][key] = st
            del arms, keep
            torch.cuda.empty_cache()
            if dense:
                arms, chks = {}, []
                for solver in ("dense", "linear"):
                    arms[solver], chk = iteration_arm(B, N, lik, solver, a.warmup)
                    chks.append(chk)
                out["iteration"][key] = alternate(arms, iters, a.rounds)
                for solver, c in zip(arms, chks):
                    if c.any_bad():                        # reported, not hidden: the timing of a failed step means nothing
                        out.setdefault("failed_steps", {})[f"{key}/{solver}"] = [t.tolist()[:8] for t in c._acc.values()]
                for k in ("step", "iteration"):
                    out[k][key]["speedup"] = round(out[k][key]["dense"] / out[k][key]["linear"], 2)
                del arms
                torch.cuda.empty_cache()
            print(json.dumps({key: {k: out[k].get(key) for k in ("step", "iteration")}}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
