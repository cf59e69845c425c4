"""Forecasting from the volatility-kernel data model with predict_solver="linear" (volt_vk_forms_*, csrc/bm.hip)
against the dense route, in ONE process: per shape the arms alternate (dense, linear, dense, linear, ...) and the median of the
rounds is reported, each round `iters` eager calls between two device events after a warm-up.  The calls are timed eagerly, host
work included: both routes read their jitter ladder's info on the host, so neither replays from a graph.
  standard_mean  forecast._standard_mean_prediction at 64 x 399, S = 1000, H = 20 (the stocks driver's shape): B x S
                 factorisations of an N x N block against ONE volt_vk_forms launch for the B series
  train_block    rollout_engine.train_block_terms "factor" -> "chain" at 8 x 4096 (config 5's share) and 1 x 399
  method         the model method GeneratePrediction (n_sample = 8) at 1 x 4096, H = 20
  linear_only    the model method and train_block_terms("chain") at 8 x 65536 (one dense fp32 block of that size is 17 GB)
The standard-mean shape runs last, one call per window (its dense arm is 64 000 factorisations per call).
Prints ONE JSON line; no figure here is a gate.  Kernel times: `rocprofv3 --kernel-trace --stats -- python
scripts/bench_predict_linear.py` in a run of its own.
Usage: bench_predict_linear.py [--iters K] [--warmup W] [--rounds R]"""
import argparse
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_bm_linear import alternate, prepare                        # noqa: E402
from volt_amd import forecast, gp, ops, rollout_engine, train_utils   # noqa: E402
from volt_amd.models import VoltMagpie, VoltronGP                     # noqa: E402
from volt_amd.synthetic import rollout_inputs, sde_batch              # noqa: E402

K_TAPS = 25


def dev(a):
    return torch.tensor(a, device="cuda", dtype=torch.float32)


def data(B, N, S, H):
    x, F, vol = sde_batch(B, N, seed=3)
    pv, z = rollout_inputs(vol[:, -1], S, H, seed=4)
    tx = dev(x)
    return tx, torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1], dev(F), dev(vol), dev(pv), dev(z)


def standard_mean_arms(B, N, S, H, warmup, solvers):
    tx, test_x, F, vp, pv, z = data(B, N, S, H)
    log_y = F[:, 1:].log()
    m = VoltMagpie(tx, log_y, gp.GaussianLikelihood(batch_shape=torch.Size([B])).cuda(), vp, k=K_TAPS).cuda()
    train_utils._set_mean(m, "constant", tx, log_y, K_TAPS, 0.5, torch.Size([B]))      # the driver's standard-mean model
    with torch.no_grad():
        m.mean_module.constant.copy_(log_y.mean(-1).reshape(m.mean_module.constant.shape))
    return {s: prepare(lambda s=s: forecast._standard_mean_prediction(m, tx, log_y, vp, test_x, pv, z, s), warmup, False)
            for s in solvers}


def train_block_arms(B, N, warmup, solves):
    tx, test_x, F, vp, _, _ = data(B, N, 1, 1)
    log_y = F[:, 1:].log()
    U = ops.cumtrapz(torch.cat((vp, vp[:, -1:]), -1), torch.cat((tx, test_x)), square=True)[:, :N].contiguous()
    r_tr = (log_y - ops.ewma(log_y, K_TAPS)[:, :-1]).contiguous()
    return {s: prepare(lambda s=s: rollout_engine.train_block_terms(U, r_tr, s), warmup, False) for s in solves}


def method_arms(B, N, H, ns, warmup, solvers):
    tx, test_x, F, vp, pv, _ = data(B, N, 1, H)
    batched = B > 1
    log_y, vol, pred_vol = (F[:, 1:].log(), vp, pv[:, 0]) if batched else (F[0, 1:].log(), vp[0], pv[0, 0])
    arms = {}
    for s in solvers:
        lh = gp.GaussianLikelihood(batch_shape=torch.Size([B]) if batched else torch.Size()).cuda()
        # (VoltronGP: its linear mean takes the H points at once; the EWMA mean of VoltMagpie predicts one point at a time)
        m = VoltronGP(tx, log_y, lh, vol, data_solver="linear" if s == "linear" else "dense",
                      vol_solver="linear" if s == "linear" else "dense", predict_solver=s).cuda()
        with torch.no_grad():
            m.mean_module.weights.fill_(0.01)
            m.mean_module.bias.fill_(2.0)
        arms[s] = prepare(lambda m=m: m.GeneratePrediction(test_x, pred_vol, ns), warmup, False)
    return arms


def with_speedup(res, slow, fast):
    res["speedup"] = round(res[slow] / res[fast], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict_linear.py measures on the MI355X; no GPU, no number")
    warnings.simplefilter("ignore", gp.NumericalWarning)              # (a dense fp32 factor that takes a rung says so on every call)
    out = {"metric": "ms per eager call (host work included), median of alternating rounds", "measured": True,
           "device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds}

    def note(key, res):
        out[key] = res
        print(json.dumps({key: res}), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    both = ("dense", "linear")
    for B, N in ((8, 4096), (1, 399)):
        note(f"train_block/{B}x{N}", with_speedup(alternate(train_block_arms(B, N, a.warmup, ("factor", "chain")), a.iters, a.rounds), "factor", "chain"))
    note("method/1x4096_H20_n8", with_speedup(alternate(method_arms(1, 4096, 20, 8, a.warmup, both), a.iters, a.rounds), "dense", "linear"))
    note("linear_only/method/8x65536_H20_n8", alternate(method_arms(8, 65536, 20, 8, a.warmup, ("linear",)), a.iters, a.rounds))
    note("linear_only/train_block/8x65536", alternate(train_block_arms(8, 65536, a.warmup, ("chain",)), a.iters, a.rounds))
    note("standard_mean/64x399_S1000_H20", with_speedup(alternate(standard_mean_arms(64, 399, 1000, 20, a.warmup, both), 1, a.rounds), "dense", "linear"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
