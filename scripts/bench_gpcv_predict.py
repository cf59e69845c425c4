"""Vol-path draws from a Markov GPCV away from its grid (csrc/markov_predict.hip), in ONE process: per shape
(series x grid, H test points -- half between observations, half beyond the last -- and S paths) the arms alternate; each round is
one window of calls between two device events after a warm-up; the median over the rounds is reported with their minimum and
maximum ("spread": a difference smaller than it is not a difference).  The method is scripts/bench_gpcv_markov.py's.
  predict     (a) model(test_x).rsample([S]) as a user calls it: validation, sort, plan, base samples, draw (eager: it reads
              the step count from the device once)
  dense       (b) the route a user has without it: the dense N x N covariance of q(u) (``_covar``), a dense conditional and a
              Cholesky draw, in fp64 torch; only where the [B,N,N] arrays fit (N <= 4096)
  plan, draw  the two kernels alone, inputs resident, replayed from a hipGraph
  second_stage (c) CONTEXT, a different model: what the vol forecast costs today -- TrainVolModelBatch(solver="linear",
              vol_posterior="chain") fitted for 1000 iterations to a vol path, then sample([S]) at the same points; ONE wall-clock
              run per shape (fit and sample apart), N <= 4096 only
The parameters are set directly (no fit: the cost of a prediction does not depend on their values).  Prints ONE JSON line.
Usage: bench_gpcv_predict.py [--iters K] [--warmup W] [--rounds R] [--shapes 1x399,8x4096] [--no-second-stage]
       bench_gpcv_predict.py --trace B N [CALLS]     # eager predictions, nothing timed: for rocprofv3 --kernel-trace --stats"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import statistics                                                  # noqa: E402

from bench_bm_linear import prepare, window                        # noqa: E402
from bench_gpcv_markov import markov_inputs                        # noqa: E402
from volt_amd import gp, ops                                       # noqa: E402

SHAPES = [(1, 399), (64, 399), (8, 4096), (8, 65536)]
POINTS = [(20, 1000), (20, 10000), (100, 1000), (100, 10000)]                 # (H, S)
DENSE_NMAX = 4096
DENSE_FAILED = []


def alternate(arms, calls, rounds):
    """arms: {name: callable}; round-robin over the arms, `rounds` windows of calls[name] calls each; median and [min, max]."""
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, run in arms.items():
            times[k].append(window(run, calls[k]))
    out = {k: round(statistics.median(v), 5) for k, v in times.items()}
    out["spread"] = {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()}
    return out


def model_of(B, N):
    from volt_amd.kernels import BMKernel
    from volt_amd.models import SingleTaskVariationalGP
    x, m, _, rho, gam, _ = markov_inputs(B, N)
    x = x + 1.0 / 252
    kw = {"batch_shape": torch.Size([B])} if B > 1 else {}
    model = SingleTaskVariationalGP(init_points=x.view(-1, 1), use_piv_chol_init=False, mean_module=gp.ConstantMean(**kw),
                                    covar_module=BMKernel(**kw), learn_inducing_locations=False, use_whitened_var_strat=False,
                                    prior_solver="markov").cuda()
    d = model.variational_strategy._variational_distribution
    pick = lambda t: t if B > 1 else t[0]
    d.variational_mean.data, d.log_diag_precision_root.data, d.coupling.data = pick(m), pick(rho), pick(gam)
    with torch.no_grad():
        model.mean_module.constant.fill_(math.log(0.2))
    return model.eval(), x


def test_points(x, H):
    """H points: half at the midpoints of the last intervals, half beyond the last observation, on the grid's step."""
    h = H // 2
    return torch.cat([(x[-h - 1:-1] + x[-h:]) / 2, x[-1] + torch.arange(1, H - h + 1, device=x.device) / 252])


def dense_route(model, x, xs, S):
    """q(f(xs)) from the N x N matrices, then a Cholesky draw: what a user of the markov family can do today."""
    from volt_amd.variational import PRIOR_JITTER, MarkovVariationalLatent
    lat = MarkovVariationalLatent(model)
    Sq = lat._covar.double().reshape(-1, x.shape[0], x.shape[0])
    m = lat.loc.detach().double().reshape(Sq.shape[0], -1)
    mu = model.mean_module.constant.detach().double().reshape(-1, 1)
    vol = model.covar_module.vol.detach().double().reshape(-1, 1, 1)
    xd, xsd = x.double(), xs.double()
    k = lambda a, b: vol * torch.minimum(a.unsqueeze(-1), b.unsqueeze(-2)) + PRIOR_JITTER
    Kuu, Ksu, Kss = k(xd, xd), k(xsd, xd), k(xsd, xsd)
    A = torch.linalg.solve(Kuu, Ksu.mT).mT
    mean = mu + (A @ (m - mu).unsqueeze(-1)).squeeze(-1)
    C = A @ Sq @ A.mT + Kss - A @ Kuu @ A.mT
    # (``_covar`` comes back in fp32: C is positive definite only to that rounding, hence a jitter at its level)
    jit = 1e-6 * C.diagonal(dim1=-2, dim2=-1).amax(-1).reshape(-1, 1, 1)
    L, info = torch.linalg.cholesky_ex(C + jit * torch.eye(xs.shape[0], device=x.device, dtype=torch.float64))
    DENSE_FAILED.append(info)                                          # (counted after the timing: reported, not hidden)
    z = torch.randn(S, *mean.shape, device=x.device, dtype=torch.float64)
    return mean + (L @ z.unsqueeze(-1)).squeeze(-1)


def second_stage(B, N, x, xs, S):
    """(fit s, sample ms): the vol forecaster fitted to a vol path and sampled at xs, wall clock, one run."""
    from volt_amd.train_utils import TrainVolModelBatch
    g = torch.Generator(device="cuda").manual_seed(5)
    vol_path = (math.log(0.2) + 0.05 * torch.randn(B, N, device="cuda", generator=g).cumsum(-1) / math.sqrt(N)).exp()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vmod, _ = TrainVolModelBatch(x, vol_path, train_iters=1000, solver="linear", vol_posterior="chain")
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    vmod.eval()
    paths = vmod(xs[xs > x[-1]]).sample(torch.Size((S,))).exp()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return round(t1 - t0, 3), round((t2 - t1) * 1e3, 3), tuple(paths.shape)


def trace(B, N, calls):
    model, x = model_of(B, N)
    xs = test_points(x, 100)
    for _ in range(2 + calls):
        model(xs).rsample(torch.Size([1000]))
    torch.cuda.synchronize()
    print(f"traced {2 + calls} predictions (H = 100, S = 1000) at B={B} N={N}")


def main():
    if "--trace" in sys.argv:
        rest = [int(v) for v in sys.argv[sys.argv.index("--trace") + 1:]]
        return trace(rest[0], rest[1], rest[2] if len(rest) > 2 else 5)
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="")
    ap.add_argument("--no-second-stage", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gpcv_predict.py measures on the MI355X; no GPU, no number")
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s] or SHAPES
    out = {"metric": "ms per call, median of alternating rounds", "measured": True, "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "rounds": a.rounds, "ms": {}, "steps_per_path": {}, "second_stage": {}, "not_run": {}}
    for B, N in shapes:
        model, x = model_of(B, N)
        for H, S in POINTS:
            key = f"{B}x{N}/H{H}/S{S}"
            xs = test_points(x, H)
            arms = {"predict": prepare(lambda: model(xs).rsample(torch.Size([S])), a.warmup, False)}
            if N <= DENSE_NMAX:
                try:
                    arms["dense"] = prepare(lambda: dense_route(model, x, xs, S), max(1, a.warmup // 3), False)
                except torch.OutOfMemoryError as e:
                    out["not_run"][key + "/dense"] = "out of memory: " + str(e)[:120]
                    torch.cuda.empty_cache()
            else:
                out["not_run"][key + "/dense"] = f"[B,N,N] fp64 arrays of {B * N * N * 8 / 2 ** 30:.0f} GiB each"
            lat = model(xs)
            plan = lat.plan
            d = model.variational_strategy._variational_distribution
            flat = [t.detach().reshape(B, N) for t in (d.variational_mean, d.log_diag_precision_root, d.coupling)]
            vol = model.covar_module.vol.detach().reshape(-1)
            mu = model.mean_module.constant.detach().reshape(-1)
            arms["plan"] = prepare(lambda: ops.markov_predict_plan(x, xs, vol, mu, *flat), a.warmup, True)
            eps = torch.randn(B, S, plan.E, device="cuda")
            arms["draw"] = prepare(lambda: ops.markov_predict_draw(plan, eps), a.warmup, True)
            iters = max(3, a.iters // 4) if (N > 4096 or S > 1000) else a.iters
            calls = {k: iters for k in arms}
            calls["dense"] = 1 if N > 1000 else max(2, iters // 4)    # (seconds per call at N = 4096: an N x N inverse per series)
            DENSE_FAILED.clear()
            out["ms"][key] = alternate(arms, calls, a.rounds)
            if DENSE_FAILED:
                failed = int(torch.stack([(i != 0).sum() for i in DENSE_FAILED]).sum())
                if failed:
                    out.setdefault("dense_cholesky_failed", {})[key] = f"{failed} of {len(DENSE_FAILED) * B} factorisations"
            out.setdefault("calls_per_window", {})[key] = calls
            out["steps_per_path"][key] = plan.E
            print(json.dumps({key: out["ms"][key]}), file=sys.stderr, flush=True)
            del arms, eps, lat, plan
            torch.cuda.empty_cache()
        if not a.no_second_stage and N <= DENSE_NMAX:
            fit_s, sample_ms, shape = second_stage(B, N, x, test_points(x, 100), 1000)
            out["second_stage"][f"{B}x{N}/H50 beyond/S1000"] = {"fit_s_1000_iterations": fit_s, "sample_ms": sample_ms,
                                                              "paths": list(shape), "runs": 1}
        del model
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
