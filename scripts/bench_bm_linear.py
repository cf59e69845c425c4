"""The vol forecaster's BM-GP on the linear-time solver (csrc/bm.hip) against the dense path, in ONE process: per shape the two
arms alternate (dense, linear, dense, linear, ...) and the median of the rounds is reported, each round `iters` calls between
two device events after a warm-up.
  step       the raw MLL + gradient step with its inputs resident: ops.mll_step (fp32, K = vol min(x, x') filled beforehand)
             against ops.bm_step (fp32 I/O); linear also as clocks per grid point at the nominal 2.4 GHz
  iteration  one trainer iteration (model(x) -> mll -> backward) of BMGP, solver="dense" / "linear", captured into a hipGraph
  posterior  model.eval()(test_x) at H = 20, eager (it reads info back), both solvers
8 x 65536 runs the linear arm only (one dense fp32 matrix of that size is 17 GB).
Prints ONE JSON line.  Kernel times: `rocprofv3 --kernel-trace --stats -- python scripts/bench_bm_linear.py` in a run of its own.
Usage: bench_bm_linear.py [--iters K] [--warmup W] [--rounds R]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from volt_amd import gp, ops                                       # noqa: E402
from volt_amd.models import BMGP                                   # noqa: E402
from volt_amd.synthetic import sde_batch                           # noqa: E402

SHAPES = [(1, 399), (64, 399), (1, 4096), (8, 4096), (64, 4096)]
LINEAR_ONLY = [(8, 65536)]
H = 20
NOMINAL_GHZ = 2.4


class Prepared:
    """A warmed-up callable and, when captured, its graph.  It OWNS what the graph touches: a captured graph holds raw
    addresses, so the closure (the model, the workspaces, the inputs) has to live as long as the graph is replayed."""

    def __init__(self, fn, graph):
        self.fn, self.graph = fn, graph

    def __call__(self):
        return self.graph.replay() if self.graph is not None else self.fn()


def prepare(fn, warmup, graph):
    """Warm `fn` up (on a side stream when it is to be captured), capture it if asked; returns the callable to time."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    if not graph:
        return Prepared(fn, None)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return Prepared(fn, g)


def window(run, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(arms, iters, rounds):
    """arms: {name: callable}; round-robin over the arms, `rounds` windows each; median ms per call."""
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, run in arms.items():
            times[k].append(window(run, iters))
    return {k: round(statistics.median(v), 5) for k, v in times.items()}


def data(B, N):
    x, _, vol = sde_batch(B, N, seed=3)
    tx = torch.tensor(x, device="cuda", dtype=torch.float32)
    return tx, torch.tensor(vol, device="cuda", dtype=torch.float32)


def step_arms(B, N, dense, warmup):
    tx, vp = data(B, N)
    v = torch.full((B,), 0.2, device="cuda")
    s = torch.full((B,), 0.6932, device="cuda")
    r = vp.log() + 0.5 * 0.04 * tx
    arms = {}
    ws = ops.BmWorkspace(B, N, "cuda", torch.float32)
    arms["linear"] = prepare(lambda: ops.bm_step(tx, v, s, r, ws), warmup, True)
    if dense:
        K = (0.2 * torch.minimum(tx[:, None], tx[None, :])).expand(B, N, N).contiguous()
        wd = ops.MllWorkspace(B, N, True, "cuda", torch.float32)
        arms["dense"] = prepare(lambda: ops.mll_step(K, r, s, wd, want_grad=True), warmup, True)
    return arms


def model_of(B, N, solver):
    tx, vp = data(B, N)
    y = vp.log() if B > 1 else vp[0].log()
    lh = gp.GaussianLikelihood(batch_shape=torch.Size([B]) if B > 1 else torch.Size()).cuda()
    return BMGP(tx, y, lh, solver=solver).cuda(), lh, tx, y


def iteration_arm(B, N, solver, warmup):
    m, lh, tx, y = model_of(B, N, solver)
    mll = gp.ExactMarginalLogLikelihood(lh, m)
    params = list(m.parameters())

    def it():
        for p in params:
            p.grad = None
        loss = -mll(m(tx), y).sum()
        loss.backward()
        return loss
    with gp.deferred_checks(immediate=True) as chk:   # (a replay needs no context: the captured step notes into chk's words)
        it()
        chk.immediate = False
        run = prepare(it, warmup, True)
    return run, chk


def posterior_arm(B, N, solver, warmup):
    m, lh, tx, y = model_of(B, N, solver)
    m.eval()
    test_x = tx[-1] + (1 + torch.arange(H, device="cuda")) / 252.0
    return prepare(lambda: m(test_x).mean, warmup, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bm_linear.py measures on the MI355X; no GPU, no number")
    out = {"metric": "ms per call, median of alternating rounds", "measured": True, "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "rounds": a.rounds, "H": H, "step": {}, "iteration": {}, "posterior": {}}
    for B, N in SHAPES + LINEAR_ONLY:
        key, dense = f"{B}x{N}", (B, N) in SHAPES
        st = alternate(step_arms(B, N, dense, a.warmup), a.iters, a.rounds)
        st["linear_clocks_per_point"] = round(st["linear"] * 1e-3 * NOMINAL_GHZ * 1e9 / N, 1)
        out["step"][key] = st
        arms, chks = {}, []
        for solver in (("dense", "linear") if dense else ("linear",)):
            arms[solver], chk = iteration_arm(B, N, solver, a.warmup)
            chks.append(chk)
        out["iteration"][key] = alternate(arms, a.iters, a.rounds)
        for solver, c in zip(arms, chks):
            if c.any_bad():                            # reported, not hidden: the timing of a failed step means nothing
                out.setdefault("failed_steps", {})[f"{key}/{solver}"] = [a.tolist()[:8] for a in c._acc.values()]
        if dense:
            for k in ("step", "iteration"):
                out[k][key]["speedup"] = round(out[k][key]["dense"] / out[k][key]["linear"], 2)
        if (B, N) != (64, 4096):                       # (the dense posterior of 64 x 4096 is another 4 GB of inverse: left out)
            arms = {s_: posterior_arm(B, N, s_, a.warmup) for s_ in (("dense", "linear") if dense else ("linear",))}
            out["posterior"][key] = alternate(arms, max(a.iters // 4, 3), a.rounds)
        del arms
        torch.cuda.empty_cache()
        print(json.dumps({key: {k: out[k].get(key) for k in ("step", "iteration", "posterior")}}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
