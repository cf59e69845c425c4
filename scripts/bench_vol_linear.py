"""The data model's fit (VoltMagpie / VoltronGP / Volt) on the linear-time step over each series' integrated vol path
(volt_vk_step_*, csrc/bm.hip; data_solver="linear") against the dense path, in ONE process: per shape the arms alternate
(dense, linear, bm, dense, linear, bm, ...) and the median of the rounds is reported, each round `iters` graph replays between
two device events after a warm-up.
  step       the raw MLL + gradient step with its inputs resident: ops.mll_step (fp32, K = V[min(i,j)] filled beforehand)
             against ops.vk_step (fp32 I/O), and ops.bm_step on the same B x N (one shared grid) as a third arm: what the
             second staged array costs.  linear also as clocks per grid point at the nominal 2.4 GHz
  iteration  one trainer iteration of TrainVoltMagpieBatch (zero_grad -> model(x) -> mll -> backward -> Adam) on the model it
             builds, solver="dense" / "linear", captured into a hipGraph
8 x 65536 runs the linear arms only (one dense fp32 matrix of that size is 17 GB).
Prints ONE JSON line.  Kernel times: `rocprofv3 --kernel-trace --stats -- python scripts/bench_vol_linear.py` in a run of its own.
Usage: bench_vol_linear.py [--iters K] [--warmup W] [--rounds R]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_bm_linear import NOMINAL_GHZ, alternate, prepare           # noqa: E402
from volt_amd import gp, ops, train_utils                             # noqa: E402
from volt_amd.models import VoltMagpie                                # noqa: E402
from volt_amd.synthetic import sde_batch                              # noqa: E402

SHAPES = [(1, 399), (64, 399), (1, 4096), (8, 4096), (64, 2048), (64, 4096)]
LINEAR_ONLY = [(8, 65536)]
K_TAPS = 25


def data(B, N):
    x, F, vol = sde_batch(B, N, seed=3)
    dev = lambda a: torch.tensor(a, device="cuda", dtype=torch.float32)
    return dev(x), dev(F), dev(vol)


def step_arms(B, N, dense, warmup):
    tx, F, vp = data(B, N)
    V = ops.cumtrapz(vp, tx, square=True)
    s = torch.full((B,), 0.6932, device="cuda")
    r = F[:, 1:].log() - F[:, 1:].log().mean(-1, keepdim=True)
    arms = {}
    ws = ops.BmWorkspace(B, N, "cuda", torch.float32)
    arms["linear"] = prepare(lambda: ops.vk_step(V, s, r, ws), warmup, True)
    wb = ops.BmWorkspace(B, N, "cuda", torch.float32)
    one = torch.ones(B, device="cuda")
    x1 = tx + tx[1]                                                    # (a strictly increasing grid from x_0 > 0)
    arms["bm"] = prepare(lambda: ops.bm_step(x1, one, s, r, wb), warmup, True)
    if dense:
        K = ops.fill(V)
        wd = ops.MllWorkspace(B, N, True, "cuda", torch.float32)
        arms["dense"] = prepare(lambda: ops.mll_step(K, r, s, wd, want_grad=True), warmup, True)
    return arms


def iteration_arm(B, N, solver, warmup):
    """The iteration TrainVoltMagpieBatch captures: its model, its parameters, its optimiser."""
    tx, F, vp = data(B, N)
    log_y = F[:, 1:].log()
    lh = gp.GaussianLikelihood(batch_shape=torch.Size([B])).cuda()
    m = VoltMagpie(tx, log_y, lh, vp, k=K_TAPS, data_solver=solver).cuda()
    params = train_utils._train_noise_and_mean(m, lh)
    m.train()
    lh.train()
    opt = train_utils._adam([{"params": params}], train_utils.LR_DATA, True)
    mll = gp.ExactMarginalLogLikelihood(lh, m)

    def it():
        opt.zero_grad(set_to_none=True)
        loss = -mll(m(tx), log_y).sum()
        loss.backward()
        opt.step()
        return loss
    with gp.deferred_checks(immediate=True) as chk:   # (a replay needs no context: the captured step notes into chk's words)
        it()
        chk.immediate = False
        run = prepare(it, warmup, True)
    return run, chk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vol_linear.py measures on the MI355X; no GPU, no number")
    out = {"metric": "ms per call, median of alternating rounds", "measured": True, "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "rounds": a.rounds, "step": {}, "iteration": {}}
    for B, N in SHAPES + LINEAR_ONLY:
        key, dense = f"{B}x{N}", (B, N) in SHAPES
        st = alternate(step_arms(B, N, dense, a.warmup), a.iters, a.rounds)
        st["linear_clocks_per_point"] = round(st["linear"] * 1e-3 * NOMINAL_GHZ * 1e9 / N, 1)
        st["linear_over_bm"] = round(st["linear"] / st["bm"], 2)
        out["step"][key] = st
        torch.cuda.empty_cache()
        arms, chks = {}, []
        for solver in (("dense", "linear") if dense else ("linear",)):
            arms[solver], chk = iteration_arm(B, N, solver, a.warmup)
            chks.append(chk)
        out["iteration"][key] = alternate(arms, a.iters, a.rounds)
        for solver, c in zip(arms, chks):
            if c.any_bad():                            # reported, not hidden: the timing of a failed step means nothing
                out.setdefault("failed_steps", {})[f"{key}/{solver}"] = [t.tolist()[:8] for t in c._acc.values()]
        if dense:
            for k in ("step", "iteration"):
                out[k][key]["speedup"] = round(out[k][key]["dense"] / out[k][key]["linear"], 2)
        del arms
        torch.cuda.empty_cache()
        print(json.dumps({key: {k: out[k].get(key) for k in ("step", "iteration")}}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
