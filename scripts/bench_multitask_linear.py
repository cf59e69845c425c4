"""MultitaskBMGP on the linear-time Kronecker step (csrc/kron_chain.hip around csrc/bm.hip; solver="linear") against its dense
path, in ONE process: per shape the arms alternate (dense, linear, batched, dense, ...) and the median of the rounds is
reported, each round `iters` hipGraph replays between two device events after a warm-up.
  iteration  one MLL + gradient iteration (model(x) -> mll -> backward), captured, parameters FIXED (how DESIGN 4.8 timed the
             dense path): MultitaskBMGP solver="dense" / "linear", and the batched BMGP(solver="linear") at B = T beside them
             (T independent vol models: what the multitask model costs over).  The warm-started eigensolver sees the same S in
             every replay here, its best case --
  training   -- so the same iteration with the trainer's fused Adam step at LR_VOL captured behind it (the parameters move as
             in TrainVolModelMultitask), dense and linear: the row that says what the warm start is worth in a fit
  posterior  model.eval()(test_x) at H = 20, eager (it reads info back), both solvers (the dense one not at 4096 x 64: its
             inverse alone is 4 GB)
  sweeps     the eigensolver's sweep counts of the linear training arm's last replay (warm) and of a cold call on the same
             parameters
N x T in {399, 4096} x {8, 64}; 65536 x 8 runs the linear arms only (one dense fp32 matrix of that size is 17 GB).
Prints ONE JSON line.
`--trace N T [STEPS]`: no timing -- STEPS eager iterations of the linear arm, then on the same inputs STEPS calls each of the
one-launch prologue and the one-workgroup epilogue of csrc/kron.hip, for a run of their own under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_multitask_linear.py --trace 4096 64`.
Usage: bench_multitask_linear.py [--iters K] [--warmup W] [--rounds R]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_bm_linear import alternate, prepare                     # noqa: E402  (the two scripts time the same way)
from volt_amd import _lib, gp, ops                                 # noqa: E402
from volt_amd.models import BMGP, MultitaskBMGP                    # noqa: E402
from volt_amd.optim import FusedAdam                               # noqa: E402
from volt_amd.train_utils import LR_VOL                            # noqa: E402
from volt_amd.synthetic import sde_batch                           # noqa: E402

SHAPES = [(399, 8), (399, 64), (4096, 8), (4096, 64)]
LINEAR_ONLY = [(65536, 8)]
H = 20


def data(N, T):
    x, _, vol = sde_batch(T, N, seed=3)
    return torch.tensor(x, device="cuda", dtype=torch.float32), torch.tensor(vol, device="cuda", dtype=torch.float32)


def multitask(N, T, solver):
    tx, vp = data(N, T)
    torch.manual_seed(1)
    lh = gp.MultitaskGaussianLikelihood(T).cuda()
    lh.noise = 1e-3
    return MultitaskBMGP(tx, vp.log().t().contiguous(), lh, solver=solver).cuda(), lh, tx


def captured(m, lh, x, y, warmup, adam=False):
    mll = gp.ExactMarginalLogLikelihood(lh, m)
    params = list(m.parameters())
    opt = FusedAdam(params, lr=LR_VOL) if adam else None

    def it():
        for p in params:
            p.grad = None
        loss = -mll(m(x), y).sum()
        loss.backward()
        if opt is not None:
            opt.step()
        return loss
    with gp.deferred_checks(immediate=True) as chk:   # (a replay needs no context: the captured step notes into chk's words)
        it()
        chk.immediate = False
        run = prepare(it, warmup, True)
    return run, chk, mll


def iteration_arm(N, T, arm, warmup, adam=False):
    if arm == "batched":
        tx, vp = data(N, T)
        lh = gp.GaussianLikelihood(batch_shape=torch.Size([T])).cuda()
        m = BMGP(tx, vp.log(), lh, solver="linear").cuda()
        return captured(m, lh, tx, vp.log(), warmup)
    m, lh, tx = multitask(N, T, arm)
    return captured(m, lh, m.train_inputs[0], m.train_targets, warmup, adam)


def posterior_arm(N, T, solver, warmup):
    m, lh, tx = multitask(N, T, solver)
    m.eval()
    test_x = tx[-1] + (1 + torch.arange(H, device="cuda")) / 252.0
    return prepare(lambda: m(test_x).mean, warmup, False)


def sweeps(mll, m, lh):
    """(warm, cold) sweep counts at the parameters the linear arm's workspace last saw."""
    ws = mll._kws
    task, dat = m.covar_module.task_covar_module, m.covar_module.data_covar_module
    params = (dat.raw_vol, task.covar_factor, task.raw_var, lh.raw_task_noises, lh.raw_noise)
    cold = ops.KronWorkspace(ws.N, ws.T, ws.state.device, ws.dtype, "linear")
    ops.kron_prologue(params, m.train_inputs[0][:, 0], m.train_targets, cold, warm=True)
    return int(ws.eig_info), int(cold.eig_info)


def trace(N, T, steps):
    m, lh, tx = multitask(N, T, "linear")
    mll = gp.ExactMarginalLogLikelihood(lh, m)
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    for _ in range(steps):                                  # the parameters move as in training: the warm start sees real steps
        opt.zero_grad()
        (-mll(m(m.train_inputs[0]), m.train_targets)).backward()
        opt.step()
    ws = mll._kws
    task, dat = m.covar_module.task_covar_module, m.covar_module.data_covar_module
    params = (dat.raw_vol, task.covar_factor, task.raw_var, lh.raw_task_noises, lh.raw_noise)
    x, Y = m.train_inputs[0][:, 0], m.train_targets
    rv, cf, var, rtn, rn = ops._kron_params(params, torch.float32)
    res = torch.empty_like(ws.res)
    for _ in range(steps):                                  # the kernels of csrc/kron.hip on the same inputs
        ops.kron_prologue(params, x, Y, ws)
        _lib.check(_lib.lib().volt_kron_epilogue_f32(rv.data_ptr(), cf.data_ptr(), var.data_ptr(), rtn.data_ptr(), rn.data_ptr(),
                                                     x.data_ptr(), ws.resid.data_ptr(), ws.bm.out.data_ptr(), ws.bm.alpha.data_ptr(),
                                                     ws.state.data_ptr(), res.data_ptr(), N, T, _lib.stream_ptr()), "volt_kron_epilogue")
    torch.cuda.synchronize()
    print(json.dumps({"trace": [N, T], "steps": steps, "last_sweeps": int(ws.eig_info)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", nargs="+", type=int, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multitask_linear.py measures on the MI355X; no GPU, no number")
    if a.trace:
        return trace(a.trace[0], a.trace[1], a.trace[2] if len(a.trace) > 2 else 20)
    out = {"metric": "ms per call, median of alternating rounds", "measured": True, "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "rounds": a.rounds, "H": H, "iteration": {}, "training": {}, "posterior": {}, "sweeps": {}}
    for N, T in SHAPES + LINEAR_ONLY:
        key, dense = f"{N}x{T}", (N, T) in SHAPES
        arms, kept = {}, {}
        for arm in (("dense", "linear", "batched") if dense else ("linear", "batched")):
            arms[arm], chk, mll = iteration_arm(N, T, arm, a.warmup)
            kept[arm] = (chk, mll)
        out["iteration"][key] = alternate(arms, a.iters, a.rounds)
        for arm, (chk, _) in kept.items():
            if chk.any_bad():                              # reported, not hidden: the timing of a failed step means nothing
                out.setdefault("failed_steps", {})[f"{key}/{arm}"] = [v.tolist()[:8] for v in chk._acc.values()]
        if dense:
            out["iteration"][key]["speedup"] = round(out["iteration"][key]["dense"] / out["iteration"][key]["linear"], 2)
        arms, kept = {}, {}
        for arm in (("dense", "linear") if dense else ("linear",)):
            arms[arm], chk, mll = iteration_arm(N, T, arm, a.warmup, adam=True)
            kept[arm] = (chk, mll)
        out["training"][key] = alternate(arms, a.iters, a.rounds)
        for arm, (chk, _) in kept.items():
            if chk.any_bad():
                out.setdefault("failed_steps", {})[f"{key}/{arm}/training"] = [v.tolist()[:8] for v in chk._acc.values()]
        if dense:
            out["training"][key]["speedup"] = round(out["training"][key]["dense"] / out["training"][key]["linear"], 2)
        lin_mll = kept["linear"][1]
        out["sweeps"][key] = dict(zip(("warm", "cold"), sweeps(lin_mll, lin_mll.model, lin_mll.likelihood)))
        solvers = ("dense", "linear") if dense and (N, T) != (4096, 64) else ("linear",)
        parms = {s_: posterior_arm(N, T, s_, a.warmup) for s_ in solvers}
        out["posterior"][key] = alternate(parms, max(a.iters // 4, 3), a.rounds)
        del arms, kept, parms, lin_mll
        torch.cuda.empty_cache()
        print(json.dumps({key: {k: out[k].get(key) for k in ("iteration", "training", "posterior", "sweeps")}}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
