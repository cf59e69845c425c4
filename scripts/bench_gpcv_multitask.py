"""Multi-task GPCV (MultitaskVariationalGP, csrc/gpcv_mt.hip): ms per ELBO + gradient step and per captured trainer
iteration, next to the batched single-task step (ops.gpcv_step at B = T) measured in the SAME process, alternating.

    python scripts/bench_gpcv_multitask.py [--shapes 399x8,399x64,4096x8,4096x64] [--rounds 5] [--no-trainer] [--json PATH]
    python scripts/bench_gpcv_multitask.py --trace N T [STEPS]      # warm-up + STEPS raw steps, nothing timed: for
                                                                    # rocprofv3 --kernel-trace --stats -- python ...

Device events after warm-up; a "round" times `reps` back-to-back steps of one variant, the variants alternate, and the
spread over the rounds (min .. max of the per-round means) is printed next to the median.  A batched shape whose buffers do
not fit the device is skipped and said so."""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from volt_amd import ops                                                                    # noqa: E402
from volt_amd.synthetic import sde_batch                                                    # noqa: E402

dev = "cuda:0"


def _gh():
    x, w = np.polynomial.hermite.hermgauss(75)
    return (torch.tensor(x, dtype=torch.float32, device=dev),
            torch.tensor(w / math.sqrt(math.pi), dtype=torch.float32, device=dev))


def _inputs(n, T):
    x, F, _ = sde_batch(T, n, seed=5)
    xt = torch.tensor(x, dtype=torch.float64)
    Ft = torch.tensor(F, dtype=torch.float64)
    yy = ((Ft[:, 1:] - Ft[:, :-1]) / Ft[:, :-1] / (xt[1] - xt[0]) ** 0.5)                  # [T,n]
    g = torch.Generator().manual_seed(0)
    K = (0.2 * torch.minimum(xt[:, None], xt[None, :])).float().to(dev)
    Lq = (0.05 * torch.eye(n) + 0.001 * torch.randn(n, n, generator=g)).tril().to(dev)
    m = yy.abs().clamp_min(1e-2).log().float().to(dev)                                     # [T,n]
    return x, F, K, Lq, m, yy.float().to(dev)


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _mt_step_fn(n, T, K, Lq, m, y, gx, gw):
    g = torch.Generator().manual_seed(1)
    Lt = (torch.eye(T) + 0.1 * torch.randn(T, T, generator=g)).tril().to(dev)
    c = torch.full((T,), -1.5, device=dev)
    cf = (0.1 * torch.randn(T, generator=g)).to(dev)
    rv = torch.zeros(T, device=dev)
    M, Y = m.t().contiguous(), y.t().contiguous()
    ws = ops.GpcvMtWorkspace(n, T, False, torch.device(dev))
    return lambda: ops.gpcv_mt_step(K, M, c, Lq, Lt, cf, rv, Y, gx, gw, ws, w_ell=1 / n, w_kl=1 / (n * T)), ws


def _batched_step_fn(n, T, K, Lq, m, y, gx, gw):
    need = ops._lib.lib().volt_gpcv_workspace_bytes(T, n, 0) + 3 * T * n * n * 4             # workspace + Lq + grad_Lq (+ slack)
    free, _ = torch.cuda.mem_get_info()
    if need > 0.9 * free:
        return None, f"skipped: the batched step needs {need / 2**30:.1f} GiB, {free / 2**30:.1f} GiB free"
    K3 = K.expand(T, n, n)                                                                 # shared prior: batch stride 0
    L3 = Lq.expand(T, n, n).contiguous()
    mu = torch.full((T, n), -1.5, device=dev)
    ws = ops.GpcvWorkspace(T, n, False, torch.device(dev))
    return (lambda: ops.gpcv_step(K3, m - mu, m, L3, y, gx, gw, ws, w_ell=1 / n, w_kl=1 / n)), None


def _trainer_ms(x, F, n, T, reps):
    """ms per captured iteration of FitGPCVMultitask's loop: two runs of the loop driver that differ by `reps` replays."""
    from volt_amd.train_utils import LR_GPCV, FitGPCVMultitask, _adam, _run_iterations
    from volt_amd.variational import VariationalELBO, num_gauss_hermite_locs
    import warnings
    xd, Fd = torch.tensor(x, device=dev), torch.tensor(F, device=dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model, lh, _ = FitGPCVMultitask(xd, Fd, train_iters=0)
    model.train()
    dt = xd[1] - xd[0]
    yy = ((Fd[:, 1:] - Fd[:, :-1]) / Fd[:, :-1] / dt ** 0.5).t().contiguous()
    elbo = VariationalELBO(lh, model, yy.numel())

    def iteration():
        with num_gauss_hermite_locs(75):
            loss = -elbo(model(xd), yy)
            loss.backward()
        return loss

    out = []
    for iters in (8, 8, 8 + reps):                       # (the first run pays the one-off set-up: not used)
        opt = _adam([{"params": model.parameters()}], LR_GPCV, True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        _run_iterations(iteration, opt, iters, False, graph=True)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return (out[2] - out[1]) / reps


def trace(n, T, steps):
    _, _, K, Lq, m, y = _inputs(n, T)
    gx, gw = _gh()
    fn, _ = _mt_step_fn(n, T, K, Lq, m, y, gx, gw)
    for _ in range(2 + steps):
        fn()
    torch.cuda.synchronize()
    print(f"traced {2 + steps} multi-task steps at N={n} T={T}")


def main():
    argv = sys.argv[1:]
    if "--trace" in argv:
        i = argv.index("--trace")
        return trace(int(argv[i + 1]), int(argv[i + 2]), int(argv[i + 3]) if len(argv) > i + 3 else 3)
    shapes = "399x8,399x64,4096x8,4096x64"
    if "--shapes" in argv:
        shapes = argv[argv.index("--shapes") + 1]
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 5
    rows = []
    gx, gw = _gh()
    for s in shapes.split(","):
        n, T = (int(v) for v in s.split("x"))
        reps = 50 if n <= 1024 else (10 if T <= 8 else 4)
        x, F, K, Lq, m, y = _inputs(n, T)
        mt, _ = _mt_step_fn(n, T, K, Lq, m, y, gx, gw)
        bt, why = _batched_step_fn(n, T, K, Lq, m, y, gx, gw)
        for fn in (mt, bt):
            if fn is not None:
                for _ in range(3):
                    fn()
        torch.cuda.synchronize()
        t_mt, t_bt = [], []
        for _ in range(rounds):                              # the pair alternates: mt, batched, mt, batched, ...
            t_mt.append(_time(mt, reps))
            if bt is not None:
                t_bt.append(_time(bt, reps))
        row = {"N": n, "T": T, "reps": reps, "rounds": rounds, "mt_step_ms": float(np.median(t_mt)),
               "mt_step_ms_min_max": [min(t_mt), max(t_mt)]}
        line = f"N={n} T={T}: multi-task step {row['mt_step_ms']:.3f} ms ({min(t_mt):.3f} .. {max(t_mt):.3f})"
        if bt is not None:
            row.update({"batched_step_ms": float(np.median(t_bt)), "batched_step_ms_min_max": [min(t_bt), max(t_bt)]})
            line += (f"   batched gpcv_step B={T} {row['batched_step_ms']:.3f} ms ({min(t_bt):.3f} .. {max(t_bt):.3f})"
                     f"   x{row['batched_step_ms'] / row['mt_step_ms']:.1f}")
        else:
            row["batched"] = why
            line += "   batched: " + why
        del mt, bt
        torch.cuda.empty_cache()
        if "--no-trainer" not in argv:
            row["trainer_iter_ms"] = _trainer_ms(x, F, n, T, 20 if n <= 1024 else 5)
            line += f"   captured trainer iteration {row['trainer_iter_ms']:.3f} ms"
        print(line, flush=True)
        rows.append(row)
        torch.cuda.empty_cache()
    if "--json" in argv:
        path = argv[argv.index("--json") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
