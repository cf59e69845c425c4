"""Drop-in for the two compute functions of voltron/option_utils.py (``ECDF`` :48-52, ``Pricer`` :26-45) on the device path
summary (scoring.summarize_paths -> volt_path_summary_f32).  The reference's pandas date helpers (GetTrainingData,
GetTrueValue, GetTradingDays, FindLastTradingDays) are not compute and are not reproduced.

The reference's quirks, kept:
* ``ECDF`` compares in LOG space (``sample_pxs.log() < true_px.log()``, both in the samples' dtype) with a strict ``<``, so
  a sample equal to the realised price does not count;
* ``Pricer`` returns one row per (expiry, option) in the order of ``edays`` and, inside an expiry, of ``options``' rows,
  with the reference's ten column names; its per-row ``np.mean(np.maximum(mc_pxs[:, e].numpy() - K, 0))`` and per-row ECDF
  are ONE summarize_paths call over all expiries and strikes here.
"""
from __future__ import annotations

import torch

from .scoring import summarize_paths

COLUMNS = ['Expiry', "Strike", "Bid", "Ask", "Voltron", "Return", "ExpClose", "QuoteClose", "Year", "Sample_Percentile"]


def ECDF(sample_pxs, true_px):
    """Share of the sampled prices strictly below the realised one, compared in log space (option_utils.py:48-52).
    sample_pxs [S] prices on the device; true_px a scalar (tensor or number).  Returns a Python float."""
    smp = sample_pxs.reshape(-1, 1).log()
    log_px = torch.as_tensor(true_px, dtype=smp.dtype, device=smp.device).reshape(1).log()
    s = summarize_paths(smp, q=(), truth=log_px)
    return s.pit[0].item()                                       # n_lt / S, correctly rounded to fp32 like the reference's


def Pricer(mc_pxs, options, edays, true_pxs, quote_price):
    """option_utils.py:26-45.  mc_pxs [S, len(edays)] sampled prices (device), options a DataFrame with columns
    expiration / strike / bid / ask, true_pxs [len(edays)] realised prices.  Returns the reference's DataFrame.
    Valuations are fp64 means of max(price - K, 0) rounded once to fp32 (the reference: an fp32 numpy mean);
    Sample_Percentile is the share of prices strictly below the realised one (the reference compares their fp32 logs:
    the same count unless a price sits within an ulp of the log of the realised price)."""
    import numpy as np
    import pandas as pd
    true_pxs = torch.as_tensor(true_pxs)
    groups = []
    for eday_idx, eday in enumerate(edays):
        eday = pd.Timestamp(eday)
        groups.append((eday_idx, eday, options[options.expiration == eday]))
    E = len(groups)
    M = max([len(opts) for _, _, opts in groups] + [0])
    strikes = np.zeros((E, M), dtype=np.float32)                 # [expiry, option]; unused slots price a strike of 0
    for e, (_, _, opts) in enumerate(groups):
        strikes[e, :len(opts)] = np.asarray(opts.strike, dtype=np.float32)
    dev = mc_pxs.device
    logger = []
    if E and M:
        # one column per expiry: G = E series of S samples and a single step, so that each expiry has its own strikes
        samples = mc_pxs.to(torch.float32).t().unsqueeze(-1)     # [E, S, 1] view of [S, E]
        s = summarize_paths(samples, q=(), truth=true_pxs.to(device=dev, dtype=torch.float32).reshape(E, 1),
                            strikes=torch.from_numpy(strikes).to(dev))
        call = s.call[:, :, 0].cpu().numpy()                      # [E, M]
        pct = s.pit[:, 0].cpu().numpy()                           # n_lt / S, correctly rounded to fp32
    true_cpu = true_pxs.detach().cpu()
    for e, (eday_idx, eday, opts) in enumerate(groups):
        year = pd.DatetimeIndex([eday])[0].year
        for m, (idx, row) in enumerate(opts.iterrows()):
            K = row.strike
            rtn = np.maximum(true_cpu[eday_idx] - K, 0)
            logger.append([eday, K, row.bid, row.ask, call[e, m], rtn.item(), true_cpu[eday_idx].item(), quote_price, year,
                           pct[e].item()])
    df = pd.DataFrame(logger)
    df.columns = COLUMNS
    return df
