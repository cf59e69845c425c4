"""The fp64 definition of every output of volt_path_summary_f32 (include/volt_hip.h), in plain torch on the CPU: sort, then
the formulas of the header.  It is the yardstick of tests/test_scoring_host.py and tests/test_gpu_scoring.py and never runs on
the device.  Outputs stay fp64 (counts int64): a test rounds to fp32 where it compares exactly."""
import math

import torch

NAN = float("nan")


def summarize(samples, q=(), truth=None, strikes=None, exp=False):
    """samples [G,S,H] (any float dtype; read as the fp32 values the kernel sees), q [Q] levels, truth [G,H] or None,
    strikes [G,M] or None.  Returns a dict of fp64 / int64 CPU tensors with the kernel's layouts:
    moments [G,4,H], quant [G,Q,H], counts [G,3,H], crps [G,H], call / put [G,M,H]."""
    x = samples.detach().cpu().to(torch.float32).to(torch.float64)
    G, S, H = x.shape
    xs = torch.sort(x, dim=1)[0]                                   # NaN sorts last; such columns are overwritten below
    v = xs.exp() if exp else xs
    q = torch.as_tensor(list(q) if not torch.is_tensor(q) else q, dtype=torch.float64).reshape(-1)
    Q = q.numel()
    mean = v.sum(1) / S
    dev = ((v - mean.unsqueeze(1)) ** 2).sum(1)
    std = (dev / (S - 1)).sqrt() if S > 1 else torch.full((G, H), NAN, dtype=torch.float64)
    moments = torch.stack((mean, std, v[:, 0], v[:, S - 1]), 1)
    pos = q * (S - 1)
    lo = pos.floor().clamp(0, S - 1).long()
    hi = (lo + 1).clamp(max=S - 1)
    quant = v[:, lo] + (v[:, hi] - v[:, lo]) * (pos - lo.to(torch.float64)).reshape(1, Q, 1)
    n_nan = torch.isnan(x).sum(1)
    if truth is None:
        y = torch.full((G, H), NAN, dtype=torch.float64)
    else:
        y = truth.detach().cpu().to(torch.float32).to(torch.float64).reshape(G, H)
    known = ~torch.isnan(y)
    n_lt = torch.where(known, (v < y.unsqueeze(1)).sum(1), torch.full((G, H), -1))
    n_le = torch.where(known, (v <= y.unsqueeze(1)).sum(1), torch.full((G, H), -1))
    i1 = torch.arange(1, S + 1, dtype=torch.float64).reshape(1, S, 1)
    crps = (v - y.unsqueeze(1)).abs().sum(1) / S - ((2 * i1 - S - 1) * v).sum(1) / (float(S) * float(S))
    if strikes is None:
        k = torch.zeros(G, 0, dtype=torch.float64)
    else:
        k = strikes.detach().cpu().to(torch.float32).to(torch.float64).reshape(G, -1)
    d = v.unsqueeze(1) - k.reshape(G, -1, 1, 1)                     # [G,M,S,H]
    call = d.clamp_min(0).sum(2) / S
    put = (-d).clamp_min(0).sum(2) / S
    bad = n_nan > 0                                                # a column with a NaN sample: NaN everywhere, counts -1
    moments = torch.where(bad.unsqueeze(1), torch.full_like(moments, NAN), moments)
    quant = torch.where(bad.unsqueeze(1), torch.full_like(quant, NAN), quant)
    call = torch.where(bad.unsqueeze(1), torch.full_like(call, NAN), call)
    put = torch.where(bad.unsqueeze(1), torch.full_like(put, NAN), put)
    crps = torch.where(bad, torch.full_like(crps, NAN), crps)
    n_lt = torch.where(bad, torch.full_like(n_lt, -1), n_lt)
    n_le = torch.where(bad, torch.full_like(n_le, -1), n_le)
    return dict(moments=moments, quant=quant, counts=torch.stack((n_nan, n_lt, n_le), 1), crps=crps, call=call, put=put,
                vmax=torch.where(bad, torch.full_like(mean, NAN), v.abs().amax(1)))


def crps_pairwise(v, y):
    """The O(S^2) form, mean |v - y| - 1/2 mean |v_i - v_j|, for one column v [S] (fp64) and a scalar y."""
    v = v.to(torch.float64)
    return (v - y).abs().mean() - 0.5 * (v.unsqueeze(0) - v.unsqueeze(1)).abs().mean()


def scratch_bytes(G, S, H):
    """volt_path_summary_scratch_bytes: the transposed samples, a column padded to a multiple of 64 floats."""
    if G < 1 or H < 1 or S < 1 or S > 32768:
        return 0
    return G * H * ((S + 63) // 64 * 64) * 4


def pricer_bound(vmax, S, value):
    """Bound on |scoring_ref - the reference Pricer's valuation|: 4 x 2^-23 of the largest price (one fp32 ulp each of the
    reference's exp, of its subtraction and of the cast) plus numpy's pairwise fp32 mean (log2 S roundings of 2^-24
    relative to the value)."""
    return 4 * 2.0 ** -23 * vmax + math.log2(S) * 2.0 ** -24 * value
