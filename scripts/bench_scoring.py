#!/usr/bin/env python3
"""Path summaries on the device against what a consumer of the sample tensor can do today (DESIGN: "Path summaries").

Per shape (G series x S paths x H steps of fp32 log-values), three variants, alternated inside ONE process:

    (a) summarize   scoring.summarize_paths: 19 levels, 8 strikes, truth, exp  (volt_path_summary_f32: two launches)
    (b) torch       the same statistics composed from torch's own device ops: sort(dim=1), gathers, means, in fp64
    (c) cpu_copy    samples.cpu() alone: what every current consumer pays before it computes anything

Device events around synchronised work; every shape is warmed; a timed window is at least --window seconds (the repeat
count is calibrated per variant); --rounds windows per variant, median and minimum reported.  Also printed: the bytes the
two kernels must move, from the shapes (samples read once, the transposed scratch written and read once), to be set against
the kernel times of a `rocprofv3 --kernel-trace --stats` run of this script (--profile: one warm call + 5 calls of (a) per
shape, nothing else).  One JSON line per shape on stdout.

    python scripts/bench_scoring.py [--shapes 8x10000x256,64x1000x20,...] [--window 0.5] [--rounds 3] [--profile]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from volt_amd import _lib, scoring  # noqa: E402

SHAPES = "8x10000x256,64x1000x20,1x1000x100,1x50x20"
LEVELS = tuple(0.05 * j for j in range(1, 20))


def torch_summary(x, q, truth, strikes):
    """(b): the statistics of summarize_paths(exp=True) from torch's device ops, fp64 after the sort."""
    G, S, H = x.shape
    v = torch.sort(x, dim=1).values.double().exp()
    mean = v.mean(1)
    std = v.std(1)
    pos = q * (S - 1)
    lo = pos.floor().long().clamp(0, S - 1)
    hi = (lo + 1).clamp(max=S - 1)
    vl, vh = v[:, lo], v[:, hi]
    quant = vl + (vh - vl) * (pos - lo).reshape(1, -1, 1)
    y = truth.double().unsqueeze(1)
    n_lt = (v < y).sum(1)
    n_le = (v <= y).sum(1)
    w = (2 * torch.arange(1, S + 1, device=x.device, dtype=torch.float64) - S - 1).reshape(1, S, 1)
    crps = (v - y).abs().mean(1) - (w * v).sum(1) / (float(S) * S)
    call = torch.stack([(v - strikes[:, m].double().reshape(G, 1, 1)).clamp_min(0).mean(1) for m in range(strikes.shape[1])], 1)
    put = torch.stack([(strikes[:, m].double().reshape(G, 1, 1) - v).clamp_min(0).mean(1) for m in range(strikes.shape[1])], 1)
    return [t.float() for t in (mean, std, v[:, 0], v[:, -1], quant, crps, call, put)] + [n_lt, n_le]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps          # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="only (a): one warm call + 5 calls per shape, for a kernel trace")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_scoring.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    for spec in args.shapes.split(","):
        G, S, H = (int(t) for t in spec.split("x"))
        g = torch.Generator(device=dev).manual_seed(G * 1000003 + S * 101 + H)
        x = 0.2 * torch.randn(G, S, H, device=dev, generator=g)
        truth = (0.2 * torch.randn(G, H, device=dev, generator=g)).exp()
        strikes = (0.2 * torch.randn(G, 8, device=dev, generator=g)).exp()
        q = torch.tensor(LEVELS, dtype=torch.float64, device=dev)
        variants = {
            "summarize": lambda: scoring.summarize_paths(x, q=LEVELS, truth=truth, strikes=strikes, exp=True),
            "torch": lambda: torch_summary(x, q, truth, strikes),
            "cpu_copy": lambda: x.cpu(),
        }
        if args.profile:
            for _ in range(6):
                variants["summarize"]()
            torch.cuda.synchronize()
            continue
        # the two computations agree (fp32 outputs of fp64 arithmetic: an ulp or two apart)
        s = variants["summarize"]()
        t = variants["torch"]()
        agree = max(float(((a - b).abs() / (b.abs() + 1e-30)).max()) for a, b in
                    ((s.mean, t[0]), (s.std, t[1]), (s.quantiles, t[4]), (s.call, t[6])))
        counts_equal = bool(torch.equal(s.n_lt.long(), t[8]) and torch.equal(s.n_le.long(), t[9]))
        res = {}
        reps = {}
        for name, fn in variants.items():
            fn()
            reps[name] = max(1, int(args.window * 1e3 / max(timed(fn, 2), 1e-3)) + 1)
        for _ in range(args.rounds):
            for name, fn in variants.items():                 # alternate the variants
                res.setdefault(name, []).append(timed(fn, reps[name]))
        sample_bytes = G * S * H * 4
        scratch_bytes = int(_lib.lib().volt_path_summary_scratch_bytes(G, S, H))
        line = {
            "shape": [G, S, H], "columns": G * H,
            "ms": {k: {"median": statistics.median(v), "min": min(v), "reps": reps[k]} for k, v in res.items()},
            "speedup_vs_torch": statistics.median(res["torch"]) / statistics.median(res["summarize"]),
            "speedup_vs_cpu_copy": statistics.median(res["cpu_copy"]) / statistics.median(res["summarize"]),
            "bytes": {"samples": sample_bytes, "scratch": scratch_bytes, "transpose_kernel": sample_bytes + scratch_bytes,
                      "column_kernel": scratch_bytes},
            "max_rel_diff_vs_torch": agree, "counts_equal": counts_equal,
            "source_hash": _lib.lib().volt_source_hash().decode(),
        }
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
