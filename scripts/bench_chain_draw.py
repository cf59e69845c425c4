"""The two joint draws of the forecast, the H x H route against the chain (csrc/chain_draw.hip), in ONE process
(the protocol of DESIGN 4.11): per shape the two arms alternate (factor, chain, factor, chain, ...) and the median of the
rounds is reported, each round `iters` eager calls between two device events after a warm-up, host work and host reads
included.
  predict     forecast._standard_mean_prediction_linear, draw="factor" -> "chain", at B x S x H = 64 x 1000 x 20 (N = 399),
              1 x 1000 x 100, 8 x 10000 x 256, and 2 x 4096 x 1024 chain only (the factor route's blocks would be 34 GB)
  vol         posterior.sample([S]) of BMGP(solver="linear") with posterior="sweep" -> "chain" at T x H = 64 x 20, 8 x 100,
              8 x 1024 (S = 1000), and of MultitaskBMGP at T = 64, H = 100; the posterior itself is built once, outside
  kernel      ops.markov_draw / ops.vk_draw alone at their largest shapes, inputs resident, captured into a hipGraph: ms per
              launch, ns per path-step, and the clocks (nominal 2.4 GHz) a wave spends per step of its 64 paths
Every shape is reported, also where the chain loses.  Prints ONE JSON line and writes it to --out when given, with the kernels'
register / LDS figures (a cross-compile, as scripts/resource_usage.py reads them); no figure here is a gate.
Usage: bench_chain_draw.py [--iters K] [--warmup W] [--rounds R] [--out FILE] [--skip-long]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_bm_linear import NOMINAL_GHZ, alternate, data, prepare, window  # noqa: E402
from volt_amd import gp, ops                                               # noqa: E402
from volt_amd.forecast import _standard_mean_prediction_linear             # noqa: E402
from volt_amd.models import BMGP, MultitaskBMGP                            # noqa: E402

PREDICT_SHAPES = [(64, 1000, 20, True), (1, 1000, 100, True), (8, 10000, 256, True), (2, 4096, 1024, False)]   # B, S, H, factor too
VOL_SHAPES = [(64, 20), (8, 100), (8, 1024)]                                # T x H, S = 1000
N = 399


def predict_arms(B, S, H, factor, warmup):
    tx, vp = data(B, N)
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    g = torch.Generator(device="cuda").manual_seed(2)
    pred_vol = (vp[:, -1:, None].log() + 0.01 * torch.randn(B, S, H, device="cuda", generator=g).cumsum(-1)).exp()
    z = torch.randn(B, S, H, device="cuda", generator=g)
    resid = 0.01 * torch.randn(B, N, device="cuda", generator=g).cumsum(-1)
    m_te = torch.full((B, H), 4.0, device="cuda")
    call = lambda draw: _standard_mean_prediction_linear(tx, resid, m_te, vp, test_x, pred_vol, z, draw=draw)
    arms = {"chain": prepare(lambda: call("chain"), warmup, False)}
    if factor:
        arms = {"factor": prepare(lambda: call("factor"), warmup, False), **arms}
    return arms


def vol_arms(post_of, shape, S, warmup):
    arms = {}
    for posterior in ("sweep", "chain"):
        post = post_of(posterior)
        base = torch.randn(S, *shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        arms[posterior] = prepare(lambda post=post, base=base: post.sample(base_samples=base), warmup, False)
    return arms


def bmgp_post(T, H, posterior):
    tx, vp = data(T, N)
    lh = gp.GaussianLikelihood(batch_shape=torch.Size([T])).cuda()
    m = BMGP(tx, vp.log(), lh, solver="linear", posterior=posterior).cuda().eval()
    return m(torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1])


def multitask_post(T, H, posterior):
    tx, vp = data(T, N)
    lh = gp.MultitaskGaussianLikelihood(num_tasks=T).cuda()
    lh.noise = 1e-3
    m = MultitaskBMGP(tx, vp.log().t().contiguous(), lh, solver="linear", posterior=posterior).cuda().eval()
    return m(torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1])


def kernel_arms(warmup):
    g = torch.Generator(device="cuda").manual_seed(3)
    G, S, H = 8, 1000, 1024
    diag = (0.01 * (1 + torch.arange(H, device="cuda", dtype=torch.float64))).expand(G, H).contiguous()
    z = torch.randn(G, S, H, device="cuda", generator=g)
    out, info = torch.empty_like(z), torch.empty(G, dtype=torch.int32, device="cuda")
    jit = torch.zeros(G, dtype=torch.float64, device="cuda")
    off = 0.9 * diag
    markov = prepare(lambda: ops.markov_draw(diag, diag, off, z, jit, out=out, info=info), warmup, True)
    B, S2, H2 = 2, 4096, 1024
    pv = 0.2 * (0.01 * torch.randn(B, S2, H2, device="cuda", generator=g).cumsum(-1)).exp()
    z2 = torch.randn(B, S2, H2, device="cuda", generator=g)
    out2, info2 = torch.empty_like(z2), torch.empty(B, S2, dtype=torch.int32, device="cuda")
    vl, vlr, dx, jit2 = (torch.full((B,), v, dtype=torch.float64, device="cuda") for v in (0.2, 1e-4, 1 / 252, 0.0))
    mean = torch.full((B, H2), 4.0, dtype=torch.float64, device="cuda")
    vk = prepare(lambda: ops.vk_draw(pv, vl, vlr, dx, mean, z2, jit2, out=out2, info=info2), warmup, True)
    return {"markov_8x1000x1024": (markov, G * S * H, G * 8), "vk_2x4096x1024": (vk, B * S2 * H2, B * S2 // 64)}


def resource_usage():
    """VGPRs, occupancy, LDS, scratch and spills of the chain-draw kernels from a gfx950 cross-compile."""
    from volt_amd.build import CSRC, FLAGS, _hipcc
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([_hipcc(), *FLAGS, "-c", os.path.join(CSRC, "chain_draw.hip"), "-o", os.path.join(tmp, "cd.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    out = {}
    for b in r.stderr.split("Function Name: ")[1:]:
        name = b.split()[0]
        if "draw_kernel" in name:
            grab = lambda pat: int(re.search(pat, b).group(1))
            out[name] = {"vgprs": grab(r" VGPRs: (\d+)"), "occupancy": grab(r"Occupancy \[waves/SIMD\]: (\d+)"),
                         "static_lds": grab(r"LDS Size \[bytes/block\]: (\d+)"), "scratch": grab(r"ScratchSize \[bytes/lane\]: (\d+)"),
                         "vgpr_spill": grab(r"VGPRs Spill: (\d+)"), "sgpr_spill": grab(r"SGPRs Spill: (\d+)")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-long", action="store_true", help="leave out 8 x 10000 x 256 (its factor arm walks 20 blocks of 2.6 GB)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_chain_draw.py needs the MI355X: there is no CPU path to time")
    warnings.simplefilter("ignore")                                 # (a jittered pivot of the fp32 H x H factor is not this script's)
    res = {"bench": "chain_draw", "device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds,
           "unit": "ms per eager call, median of rounds, host work included", "predict": {}, "vol": {}, "kernel": {}}
    for B, S, H, factor in PREDICT_SHAPES:
        if a.skip_long and S * H > 2 ** 20 and factor:
            continue
        big = S * H > 2 ** 20
        t = alternate(predict_arms(B, S, H, factor, 1 if big else a.warmup), 2 if big else a.iters, 3 if big else a.rounds)
        if factor:
            t["speedup"] = round(t["factor"] / t["chain"], 3)
        res["predict"][f"{B}x{S}x{H}"] = t
        torch.cuda.empty_cache()
    for T, H in VOL_SHAPES:
        t = alternate(vol_arms(lambda p: bmgp_post(T, H, p), (T, H), 1000, a.warmup), a.iters, a.rounds)
        res["vol"][f"bmgp_{T}xH{H}_S1000"] = dict(t, speedup=round(t["sweep"] / t["chain"], 3))
    t = alternate(vol_arms(lambda p: multitask_post(64, 100, p), (100, 64), 1000, a.warmup), a.iters, a.rounds)
    res["vol"]["multitask_64xH100_S1000"] = dict(t, speedup=round(t["sweep"] / t["chain"], 3))
    for name, (run, steps, waves) in kernel_arms(a.warmup).items():
        ms = sorted(window(run, a.iters) for _ in range(a.rounds))[a.rounds // 2]
        res["kernel"][name] = {"ms": round(ms, 5), "ns_per_path_step": round(ms * 1e6 / steps, 4),
                               "clocks_per_wave_step": round(ms * 1e-3 * NOMINAL_GHZ * 1e9 * waves * 64 / steps, 1)}
    res["resources"] = resource_usage()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
