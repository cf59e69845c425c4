"""ms per MLL + gradient iteration of MultitaskBMGP (the Kronecker step: prologue -> batched step over the shared M ->
epilogue -> backward), eager and hipGraph-captured, timed with device events after a warm-up; beside it the batched BMGP
iteration at B = T (TrainVolModelBatch's: the same step without the Kronecker wrapping), the eigensolver alone, and at
(399, 8) the dense route (one 3192^2 fp32 factorisation of the NT x NT covariance on the library's potrf).
Prints ONE JSON line.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_multitask.py`.
Usage: bench_multitask.py [--iters K] [--warmup W]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from volt_amd import gp, ops                                       # noqa: E402
from volt_amd.models import BMGP, MultitaskBMGP                    # noqa: E402
from volt_amd.synthetic import sde_batch                           # noqa: E402

SHAPES = [(399, 8), (399, 64), (4096, 8), (4096, 64)]


def timed(fn, iters, warmup, graph):
    """Median-free simple timing: `iters` calls between two device events (graph: one captured call, replayed)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    run = fn
    if graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        run = g.replay
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kron_iteration(N, T):
    x, F, vol = sde_batch(T, N, seed=3)
    tx, vp = torch.tensor(x, device="cuda"), torch.tensor(vol, device="cuda")
    torch.manual_seed(0)
    lh = gp.MultitaskGaussianLikelihood(T).cuda()
    lh.noise = 1e-3
    m = MultitaskBMGP(tx, vp.log().t(), lh)
    mll = gp.ExactMarginalLogLikelihood(lh, m)
    params = list(m.parameters())
    chk = gp.deferred_checks(immediate=True)

    def it():
        for p in params:
            p.grad = None
        loss = -mll(m(m.train_inputs[0]), m.train_targets)
        loss.backward()
        return loss
    return it, chk


def batch_iteration(N, T):
    x, F, vol = sde_batch(T, N, seed=3)
    tx, vp = torch.tensor(x, device="cuda"), torch.tensor(vol, device="cuda")
    lh = gp.GaussianLikelihood(batch_shape=torch.Size([T])).cuda()
    m = BMGP(tx, vp.log(), lh).cuda()
    mll = gp.ExactMarginalLogLikelihood(lh, m)
    params = list(m.parameters())
    chk = gp.deferred_checks(immediate=True)
    target = vp.log()

    def it():
        for p in params:
            p.grad = None
        loss = -mll(m(tx), target).sum()
        loss.backward()
        return loss
    return it, chk


def run_deferred(make, N, T, iters, warmup, graph):
    it, chk = make(N, T)
    with chk:
        it()                                       # sizes the deferred accumulators (immediate check)
        chk.immediate = False
        ms = timed(it, iters, warmup, graph)
        bad = chk.any_bad()
    assert bad == 0, f"failed factorisation at {(N, T)}"
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    out = {"metric": "ms per MLL+grad iteration", "measured": True, "device": torch.cuda.get_device_name(0), "kron": {},
           "batch_bmgp": {}, "syev": {}}
    for N, T in SHAPES:
        key = f"{N}x{T}"
        out["kron"][key] = {g: round(run_deferred(kron_iteration, N, T, a.iters, a.warmup, g == "graph"), 4)
                            for g in ("eager", "graph")}
        out["batch_bmgp"][key] = {g: round(run_deferred(batch_iteration, N, T, a.iters, a.warmup, g == "graph"), 4)
                                  for g in ("eager", "graph")}
        print(json.dumps({key: [out["kron"][key], out["batch_bmgp"][key]]}), file=sys.stderr, flush=True)
    for T in (8, 64):
        g = torch.Generator(device="cuda").manual_seed(T)
        X = torch.randn(T, T, device="cuda", dtype=torch.float64, generator=g)
        S = X @ X.T + torch.eye(T, device="cuda", dtype=torch.float64)
        lam, Q, info = ops.syev_small(S)
        out["syev"][f"T{T}"] = {"ms": round(timed(lambda: ops.syev_small(S), a.iters, a.warmup, True), 4),
                                "sweeps": int(info)}
    # the dense route at (399, 8): one 3192^2 factorisation of K_x (x) K_t + I (x) D (fp32, the library potrf)
    N, T = 399, 8
    x = torch.arange(N, device="cuda", dtype=torch.float32) / 252.
    Kt = torch.eye(T, device="cuda") * 0.5 + 0.1
    Sd = torch.kron(0.2 * torch.minimum(x[:, None], x[None, :]), Kt)[None].contiguous()
    s2 = torch.full((1,), 1e-3, device="cuda")
    out["dense_potrf_399x8"] = round(timed(lambda: ops.potrf(Sd, s2), a.iters, a.warmup, False), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
