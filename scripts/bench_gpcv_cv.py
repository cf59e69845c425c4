"""The "cv" GPCV step (volt_gpcv_cv_step_f32, csrc/gpcv.hip) next to the "exp" step (volt_gpcv_step_f32) on the same
inputs in the SAME process, alternating: ms per ELBO + gradient step, and per captured trainer iteration of FitGPCV.

    python scripts/bench_gpcv_cv.py [--shapes 1x399,64x399,8x4096,32x4096] [--kc 5] [--rounds 5] [--no-trainer] [--json PATH]
    python scripts/bench_gpcv_cv.py --trace B N [KC] [STEPS]    # warm-up + STEPS steps of each variant, nothing timed: for
                                                                # rocprofv3 --kernel-trace --stats -- python ...

Device events after warm-up; a "round" times `reps` back-to-back steps of one variant, the variants alternate, and the
spread over the rounds (min .. max of the per-round means) is printed next to the median.  The two steps differ in the
row kernel only (gh_ell_kernel / gh_cv_ell_kernel<KC> + cv_abc_reduce_kernel), so the difference of the step times should
be the difference of those kernels' times: the --trace run gives the latter."""
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


def _inputs(B, n, Kc):
    x, F, _ = sde_batch(B, n, seed=5)
    xt = torch.tensor(x, dtype=torch.float64)
    Ft = torch.tensor(F, dtype=torch.float64)
    yy = ((Ft[:, 1:] - Ft[:, :-1]) / Ft[:, :-1] / (xt[1] - xt[0]) ** 0.5)                  # [B,n]
    g = torch.Generator().manual_seed(0)
    K = (0.2 * torch.minimum(xt[:, None], xt[None, :])).float().to(dev).expand(B, n, n)    # shared prior: batch stride 0
    Lq = (0.05 * torch.eye(n) + 0.001 * torch.randn(n, n, generator=g)).tril().to(dev).expand(B, n, n).contiguous()
    m = yy.abs().clamp_min(1e-2).log().float().to(dev)
    raw = [torch.rand(B, Kc, generator=g), 0.1 * torch.rand(B, Kc, generator=g), torch.rand(B, Kc, generator=g)]
    abc = torch.stack([torch.nn.functional.softplus(raw[0]), 3 * torch.sigmoid(raw[1]), 6 * torch.sigmoid(raw[2]) - 3], 1)
    return x, F, K, Lq, m, yy.float().to(dev), abc.to(dev).contiguous()


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _step_fns(B, n, Kc, K, Lq, m, y, abc, gx, gw):
    mu = torch.full((B, n), -1.5, device=dev)
    r = m - mu
    we = ops.GpcvWorkspace(B, n, False, torch.device(dev))
    wc = ops.GpcvWorkspace(B, n, False, torch.device(dev), Kc=Kc)
    exp = lambda: ops.gpcv_step(K, r, m, Lq, y, gx, gw, we, w_ell=1 / n, w_kl=1 / n)
    cv = lambda: ops.gpcv_cv_step(K, r, m, Lq, y, abc, gx, gw, wc, w_ell=1 / n, w_kl=1 / n)
    return exp, cv


def _trainer_ms(x, F, reps, **kw):
    """ms per captured iteration of FitGPCV's loop: two runs of the loop driver that differ by `reps` replays."""
    import warnings
    from volt_amd.train_utils import LR_GPCV, FitGPCV, _adam, _run_iterations
    from volt_amd.variational import VariationalELBO, num_gauss_hermite_locs
    xd, Fd = torch.tensor(x, device=dev), torch.tensor(F[0], device=dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model, lh, _ = FitGPCV(xd, Fd, train_iters=0, **kw)
    model.train()
    dt = xd[1] - xd[0]
    yy = (Fd[1:] - Fd[:-1]) / Fd[:-1] / dt ** 0.5
    elbo = VariationalELBO(lh, model, yy.shape[-1])
    params = [p for p in model.parameters() if p.requires_grad]        # (the likelihood's are among them: the model registers it)

    def iteration():
        with num_gauss_hermite_locs(75):
            loss = -elbo(model(xd), yy)
            loss.backward()
        return loss

    out = []
    for iters in (8, 8, 8 + reps):                       # (the first run pays the one-off set-up: not used)
        opt = _adam([{"params": params}], LR_GPCV, True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        _run_iterations(iteration, opt, iters, False, graph=True)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return (out[2] - out[1]) / reps


def trace(B, n, Kc, steps):
    _, _, K, Lq, m, y, abc = _inputs(B, n, Kc)
    gx, gw = _gh()
    exp, cv = _step_fns(B, n, Kc, K, Lq, m, y, abc, gx, gw)
    for _ in range(2 + steps):
        exp()
        cv()
    torch.cuda.synchronize()
    print(f"traced {2 + steps} exp and cv steps at B={B} N={n} Kc={Kc}")


def main():
    argv = sys.argv[1:]
    if "--trace" in argv:
        i = argv.index("--trace")
        rest = [int(v) for v in argv[i + 1:i + 5]]
        return trace(rest[0], rest[1], rest[2] if len(rest) > 2 else 5, rest[3] if len(rest) > 3 else 5)
    shapes = argv[argv.index("--shapes") + 1] if "--shapes" in argv else "1x399,64x399,8x4096,32x4096"
    Kc = int(argv[argv.index("--kc") + 1]) if "--kc" in argv else 5
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 5
    rows = []
    gx, gw = _gh()
    for s in shapes.split(","):
        B, n = (int(v) for v in s.split("x"))
        reps = 50 if n <= 1024 else (10 if B <= 8 else 4)
        x, F, K, Lq, m, y, abc = _inputs(B, n, Kc)
        exp, cv = _step_fns(B, n, Kc, K, Lq, m, y, abc, gx, gw)
        for _ in range(3):
            exp()
            cv()
        torch.cuda.synchronize()
        t_e, t_c = [], []
        for _ in range(rounds):                              # the pair alternates: exp, cv, exp, cv, ...
            t_e.append(_time(exp, reps))
            t_c.append(_time(cv, reps))
        row = {"B": B, "N": n, "Kc": Kc, "reps": reps, "rounds": rounds, "exp_step_ms": float(np.median(t_e)),
               "exp_step_ms_min_max": [min(t_e), max(t_e)], "cv_step_ms": float(np.median(t_c)),
               "cv_step_ms_min_max": [min(t_c), max(t_c)]}
        line = (f"B={B} N={n} Kc={Kc}: exp step {row['exp_step_ms']:.4f} ms ({min(t_e):.4f} .. {max(t_e):.4f})   "
                f"cv step {row['cv_step_ms']:.4f} ms ({min(t_c):.4f} .. {max(t_c):.4f})   "
                f"difference {1e3 * (row['cv_step_ms'] - row['exp_step_ms']):+.1f} us")
        del exp, cv
        torch.cuda.empty_cache()
        if "--no-trainer" not in argv and B == 1 and n <= 1024:
            row["trainer_iter_ms_exp"] = _trainer_ms(x, F, 40)
            row["trainer_iter_ms_cv"] = _trainer_ms(x, F, 40, param="cv", K=1, train_likelihood=True)
            line += (f"   captured trainer iteration: exp {row['trainer_iter_ms_exp']:.4f} ms, "
                     f"cv (K=1, likelihood trained) {row['trainer_iter_ms_cv']:.4f} ms")
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
