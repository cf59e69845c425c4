"""The vol forecaster's posterior, posterior="solve" (ops.bm_step + ops.bm_solve on K_t* [T,N,H]) against posterior="sweep" (ONE
ops.bm_post launch, csrc/bm.hip), in ONE process (the protocol of DESIGN 4.11): per shape the two arms alternate
(solve, sweep, solve, sweep, ...) and the median of the rounds is reported, each round `iters` eager calls of
model.eval()(test_x) between two device events after a warm-up -- the host read of info is part of a call in both arms.
  bmgp        BMGP(solver="linear") at T x N = 1 x 399, 64 x 399, 1 x 4096, 8 x 4096, 8 x 65536
  multitask   MultitaskBMGP(solver="linear") at N x T = 399 x 8, 4096 x 8, 4096 x 64, 65536 x 8
each at H = 20 and H = 100 test points (the first beyond the grid, as a forecast's are).
  kernel      ops.bm_post alone, inputs resident, captured into a hipGraph: ms per launch and clocks per grid point at the
              nominal 2.4 GHz (one wave walks the N steps of a series for up to 64 test points)
Every shape is reported, also where "sweep" loses.  Prints ONE JSON line and writes it to --out when given; no figure here is a
gate.  Kernel times and register / LDS figures: `rocprofv3 --kernel-trace --stats -- python scripts/bench_bm_posterior.py`
in a run of its own, and scripts/resource_usage.py.
Usage: bench_bm_posterior.py [--iters K] [--warmup W] [--rounds R] [--out FILE] [--skip-long]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_bm_linear import NOMINAL_GHZ, alternate, data, prepare, window  # noqa: E402
from volt_amd import gp, ops                                               # noqa: E402
from volt_amd.models import BMGP, MultitaskBMGP                            # noqa: E402

BMGP_SHAPES = [(1, 399), (64, 399), (1, 4096), (8, 4096), (8, 65536)]       # T x N
MT_SHAPES = [(399, 8), (4096, 8), (4096, 64), (65536, 8)]                   # N x T
HS = (20, 100)
KERNEL_SHAPES = [(1, 399), (1, 4096), (8, 4096), (64, 4096), (8, 65536)]    # B x N


def test_points(tx, H):
    return torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]


def bmgp_arms(T, N, H, warmup):
    tx, vp = data(T, N)
    y = vp.log() if T > 1 else vp[0].log()
    xs = test_points(tx, H)
    arms = {}
    for posterior in ("solve", "sweep"):
        lh = gp.GaussianLikelihood(batch_shape=torch.Size([T]) if T > 1 else torch.Size()).cuda()
        m = BMGP(tx, y, lh, solver="linear", posterior=posterior).cuda().eval()
        arms[posterior] = prepare(lambda m=m: m(xs), warmup, False)
    return arms


def multitask_arms(N, T, H, warmup):
    tx, vp = data(T, N)
    xs = test_points(tx, H)
    arms = {}
    for posterior in ("solve", "sweep"):
        lh = gp.MultitaskGaussianLikelihood(num_tasks=T).cuda()
        lh.noise = 1e-3
        m = MultitaskBMGP(tx, vp.log().t().contiguous(), lh, solver="linear", posterior=posterior).cuda().eval()
        arms[posterior] = prepare(lambda m=m: m(xs), warmup, False)
    return arms


def kernel_arm(B, N, H, warmup):
    tx, vp = data(B, N)
    x64, xs = tx.double(), test_points(tx, H).double()
    v = torch.full((B,), 0.2, device="cuda", dtype=torch.float64)
    s = torch.full((B,), 0.6932, device="cuda", dtype=torch.float64)
    r = (vp.log() + 0.5 * 0.04 * tx).double()
    return prepare(lambda: ops.bm_post(x64, xs, v, s, r), warmup, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-long", action="store_true", help="leave out the N = 65536 shapes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bm_posterior.py needs the MI355X: there is no CPU path to time")
    res = {"bench": "bm_posterior", "device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds,
           "unit": "ms per posterior call, median of rounds, host read included", "bmgp": {}, "multitask": {}, "kernel": {}}
    keep = lambda n: not (a.skip_long and n >= 65536)
    for T, N in BMGP_SHAPES:
        for H in HS:
            if keep(N):
                iters = a.iters if N < 65536 else max(2, a.iters // 5)
                t = alternate(bmgp_arms(T, N, H, a.warmup), iters, a.rounds)
                res["bmgp"][f"{T}x{N}_H{H}"] = dict(t, speedup=round(t["solve"] / t["sweep"], 3))
    for N, T in MT_SHAPES:
        for H in HS:
            if keep(N):
                iters = a.iters if N < 65536 else 2
                t = alternate(multitask_arms(N, T, H, a.warmup if N < 65536 else 1), iters, a.rounds if N < 65536 else 3)
                res["multitask"][f"{N}x{T}_H{H}"] = dict(t, speedup=round(t["solve"] / t["sweep"], 3))
    for B, N in KERNEL_SHAPES:
        for H in HS:
            if keep(N):
                run = kernel_arm(B, N, H, a.warmup)
                ms = sorted(window(run, a.iters) for _ in range(a.rounds))[a.rounds // 2]
                res["kernel"][f"{B}x{N}_H{H}"] = {"ms": round(ms, 5), "clocks_per_grid_point": round(ms * 1e-3 * NOMINAL_GHZ * 1e9 / N, 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
