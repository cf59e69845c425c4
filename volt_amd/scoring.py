"""Scoring forecast paths on the device: what the reference's consumers compute on the host after ``samples.cpu()`` --
``ECDF`` / ``Pricer`` of voltron/option_utils.py:26-52 and the weather calibration notebook's per-step ECDF,
``Calibration`` and Gaussian NLL -- from ONE library call over the sample tensor (volt_path_summary_f32, csrc/summary.hip).

    s = summarize_paths(samples, q=(0.05, 0.5, 0.95), truth=realised, strikes=K, exp=True)
    calibration(s.pit, levels), gaussian_nll(s, realised)

``summarize_paths`` is the kernel; ``calibration`` and ``gaussian_nll`` are a few torch ops on its [G,H] outputs.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import ops

DEFAULT_LEVELS = (0.05, 0.25, 0.5, 0.75, 0.95)


@dataclass
class PathSummary:
    """Per series and horizon step ([G,H]; [H] for unbatched samples), device tensors.  ``quantiles`` [G,Q,H], ``call`` /
    ``put`` [G,M,H].  ``n_lt`` / ``n_le`` are -1 (and ``pit`` / ``crps`` NaN) where there is no truth; a column with a NaN
    sample has ``n_nan`` > 0 and NaN in every float field."""
    mean: torch.Tensor
    std: torch.Tensor
    min: torch.Tensor
    max: torch.Tensor
    quantiles: torch.Tensor
    n_nan: torch.Tensor
    n_lt: torch.Tensor
    n_le: torch.Tensor
    pit: torch.Tensor
    crps: torch.Tensor
    call: torch.Tensor
    put: torch.Tensor
    q: tuple
    nsample: int

    def fields(self):
        return {k: v for k, v in self.__dict__.items() if torch.is_tensor(v)}

    def cpu(self):
        return PathSummary(**{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in self.__dict__.items()})


@dataclass
class SummarySpec:
    """What the batch drivers summarise each window with (forecast.py): quantile levels, strikes [M] or [G,M] in value
    units, and whether the samples are logs of the values (the drivers' rollouts are log-prices: exp=True)."""
    q: Sequence[float] = DEFAULT_LEVELS
    strikes: Optional[torch.Tensor] = None
    exp: bool = True


def summarize_paths(samples, q=DEFAULT_LEVELS, truth=None, strikes=None, exp=False) -> PathSummary:
    """samples [S,H] or [G,S,H] (device, fp32; a view with a contiguous last dimension -- ``preds[:, a:b]`` -- is read in
    place).  truth [H] / [G,H] in value units (NaN = unknown); strikes [M] or [G,M]; exp: the statistics are those of
    exp(samples) (taken in fp64).  One library call, no host synchronisation."""
    batched = samples.ndim == 3
    if samples.ndim not in (2, 3):
        raise ValueError("samples must be [S,H] or [G,S,H]")
    x = samples if batched else samples.unsqueeze(0)
    G, S, H = x.shape
    if truth is not None:
        truth = torch.as_tensor(truth, dtype=torch.float32, device=x.device).reshape(G, H)
    if strikes is not None:
        strikes = torch.as_tensor(strikes, dtype=torch.float32, device=x.device)
        strikes = strikes.reshape(1, -1).expand(G, -1) if strikes.ndim == 1 else strikes.reshape(G, -1)
    levels = tuple(float(v) for v in (q.tolist() if torch.is_tensor(q) else q))
    moments, quant, counts, crps, call, put = ops.path_summary(x, levels, truth, strikes, exp)
    n_lt = counts[:, 1]
    # n_lt / S correctly rounded to fp32, as the reference's host division gives it: the device divides a tensor by a scalar
    # as a product with the reciprocal, which in fp32 is an ulp off for some counts; in fp64 that error is far below the
    # distance of n / S (n < S <= 2^15) from any fp32 rounding boundary
    pit = torch.where(n_lt >= 0, (n_lt.to(torch.float64) / S).to(torch.float32), torch.full_like(crps, float("nan")))
    out = dict(mean=moments[:, 0], std=moments[:, 1], min=moments[:, 2], max=moments[:, 3], quantiles=quant,
               n_nan=counts[:, 0], n_lt=n_lt, n_le=counts[:, 2], pit=pit, crps=crps, call=call, put=put)
    if not batched:
        out = {k: v[0] for k, v in out.items()}
    return PathSummary(q=levels, nsample=S, **out)


def calibration(pit, levels):
    """The notebook's ``Calibration(pcts, level)`` for every level at once: the share of PIT values below each level
    (NaN entries -- windows without a realised value -- are left out).  pit: any shape; returns [len(levels)]."""
    pit = torch.as_tensor(pit).reshape(-1)
    levels = torch.as_tensor(levels, dtype=pit.dtype, device=pit.device).reshape(-1)
    known = ~torch.isnan(pit)
    below = (pit.unsqueeze(0) < levels.unsqueeze(1)) & known.unsqueeze(0)
    return below.sum(1).to(pit.dtype) / known.sum().clamp_min(1)


def gaussian_nll(summary: PathSummary, truth):
    """The notebook's NLL: -log N(truth; mean, std^2) from the sample mean and standard deviation, elementwise."""
    truth = torch.as_tensor(truth, dtype=summary.mean.dtype, device=summary.mean.device).reshape(summary.mean.shape)
    var = summary.std ** 2
    return 0.5 * (math.log(2 * math.pi) + var.log() + (truth - summary.mean) ** 2 / var)
