"""Multi-task GPCV with the copula-process ("cv") likelihood, one warp per task (csrc/gpcv_mt_cv.hip): ms per ELBO +
gradient step at K = 1 and K = 5 next to the "exp" multi-task step and the batched single-task "cv" step
(ops.gpcv_cv_step at B = T, K = 5), all measured in the SAME process, alternating; and ms per captured iteration of
FitGPCVMultitask(param="cv", K=1, train_likelihood=True).

    python scripts/bench_gpcv_multitask_cv.py [--shapes 399x8,399x64,4096x8,4096x64] [--rounds 5] [--no-trainer] [--json PATH]
    python scripts/bench_gpcv_multitask_cv.py --trace N T [STEPS]   # warm-up + STEPS raw "cv" steps (K = 5), nothing timed:
                                                                    # for rocprofv3 --kernel-trace --stats -- python ...

Timing as scripts/bench_gpcv_multitask.py (whose inputs these are): device events after warm-up, `reps` back-to-back steps
per round, the variants alternate, median and min .. max over the rounds."""
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_gpcv_multitask import _gh, _inputs, _mt_step_fn, _time, dev                      # noqa: E402
from volt_amd import ops                                                                    # noqa: E402


def _abc(T, Kc):
    """Transformed a, b, c of VolatilityGaussianLikelihood's own draws, [T,3,Kc]."""
    g = torch.Generator().manual_seed(2)
    ra, rb, rc = torch.rand(T, Kc, generator=g), 0.1 * torch.rand(T, Kc, generator=g), torch.rand(T, Kc, generator=g)
    return torch.stack([torch.nn.functional.softplus(ra), 3 * torch.sigmoid(rb), 6 * torch.sigmoid(rc) - 3], 1).to(dev)


def _mt_cv_step_fn(n, T, Kc, K, Lq, m, y, gx, gw):
    g = torch.Generator().manual_seed(1)
    Lt = (torch.eye(T) + 0.1 * torch.randn(T, T, generator=g)).tril().to(dev)
    c = torch.full((T,), -1.5, device=dev)
    cf = (0.1 * torch.randn(T, generator=g)).to(dev)
    rv = torch.zeros(T, device=dev)
    M, Y, abc = m.t().contiguous(), y.t().contiguous(), _abc(T, Kc)
    ws = ops.GpcvMtWorkspace(n, T, False, torch.device(dev), Kc)
    return lambda: ops.gpcv_mt_step(K, M, c, Lq, Lt, cf, rv, Y, gx, gw, ws, w_ell=1 / n, w_kl=1 / (n * T), abc=abc)


def _batched_cv_step_fn(n, T, Kc, K, Lq, m, y, gx, gw):
    need = ops._lib.lib().volt_gpcv_cv_workspace_bytes(T, n, 0, Kc) + 3 * T * n * n * 4
    free, _ = torch.cuda.mem_get_info()
    if need > 0.9 * free:
        return None, f"skipped: the batched step needs {need / 2**30:.1f} GiB, {free / 2**30:.1f} GiB free"
    K3, L3 = K.expand(T, n, n), Lq.expand(T, n, n).contiguous()
    mu, abc = torch.full((T, n), -1.5, device=dev), _abc(T, Kc)
    ws = ops.GpcvWorkspace(T, n, False, torch.device(dev), Kc)
    return (lambda: ops.gpcv_cv_step(K3, m - mu, m, L3, y, abc, gx, gw, ws, w_ell=1 / n, w_kl=1 / n)), None


def _trainer_ms(x, F, reps):
    """ms per captured iteration of FitGPCVMultitask(param="cv", K=1, train_likelihood=True): two fits that differ by
    `reps` replays (the first fit pays the one-off set-up and is not used)."""
    from volt_amd.train_utils import FitGPCVMultitask
    xd, Fd = torch.tensor(x, device=dev), torch.tensor(F, device=dev)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for iters in (8, 8, 8 + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.manual_seed(0)
            torch.cuda.synchronize()
            a.record()
            FitGPCVMultitask(xd, Fd, train_iters=iters, graph=True, param="cv", K=1, train_likelihood=True)
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
    return (out[2] - out[1]) / reps


def trace(n, T, steps):
    _, _, K, Lq, m, y = _inputs(n, T)
    fn = _mt_cv_step_fn(n, T, 5, K, Lq, m, y, *_gh())
    for _ in range(2 + steps):
        fn()
    torch.cuda.synchronize()
    print(f"traced {2 + steps} multi-task cv steps (K = 5) at N={n} T={T}")


def main():
    argv = sys.argv[1:]
    if "--trace" in argv:
        i = argv.index("--trace")
        return trace(int(argv[i + 1]), int(argv[i + 2]), int(argv[i + 3]) if len(argv) > i + 3 else 3)
    shapes = argv[argv.index("--shapes") + 1] if "--shapes" in argv else "399x8,399x64,4096x8,4096x64"
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 5
    rows = []
    gx, gw = _gh()
    for s in shapes.split(","):
        n, T = (int(v) for v in s.split("x"))
        reps = 50 if n <= 1024 else (10 if T <= 8 else 4)
        x, F, K, Lq, m, y = _inputs(n, T)
        bt, why = _batched_cv_step_fn(n, T, 5, K, Lq, m, y, gx, gw)
        fns = {"exp": _mt_step_fn(n, T, K, Lq, m, y, gx, gw)[0], "cv_k1": _mt_cv_step_fn(n, T, 1, K, Lq, m, y, gx, gw),
               "cv_k5": _mt_cv_step_fn(n, T, 5, K, Lq, m, y, gx, gw)}
        if bt is not None:
            fns["batched_cv_k5"] = bt
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(rounds):                              # the variants alternate
            for k, fn in fns.items():
                t[k].append(_time(fn, reps))
        row = {"N": n, "T": T, "reps": reps, "rounds": rounds}
        for k, v in t.items():
            row[k + "_step_ms"], row[k + "_step_ms_min_max"] = float(np.median(v)), [min(v), max(v)]
        if bt is None:
            row["batched_cv_k5"] = why
        row["cv_k5_minus_exp_ms"] = row["cv_k5_step_ms"] - row["exp_step_ms"]
        line = f"N={n} T={T}: " + "   ".join(f"{k} {np.median(v):.3f} ms ({min(v):.3f} .. {max(v):.3f})" for k, v in t.items())
        del fns, bt
        torch.cuda.empty_cache()
        if "--no-trainer" not in argv:
            row["cv_k1_trainer_iter_ms"] = _trainer_ms(x, F, 20 if n <= 1024 else 5)
            line += f"   captured cv trainer iteration {row['cv_k1_trainer_iter_ms']:.3f} ms"
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
