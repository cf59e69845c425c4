#!/usr/bin/env python3
"""Golden vectors for the path-summary stage, made by EXECUTING the reference's own consumers of a sample tensor:

    voltron/option_utils.py:26-45   Pricer  (the ``Voltron`` valuation and ``Sample_Percentile`` columns)
    voltron/option_utils.py:48-52   ECDF

The module is loaded by file path (the package ``__init__`` would pull in gpytorch); it needs numpy, torch and pandas.
Runs only where the reference is checked out (the location is ``make_golden_gpcv.REF``); writes ``scoring.npz`` next to
itself.  Only inputs and recorded results are stored.

The fixture: 1000 paths x 3 expiries, log p = log 400 + 0.05 cumsum(randn) (seed 7, fp32), prices = exp(log p) in fp32 as a
driver would hand them over; strikes 360 .. 500 in steps of 20 at every expiry; realised prices 398, 411, 385.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_scoring.py
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
EDAYS = ("2021-01-15", "2021-02-19", "2021-03-19")
STRIKES = tuple(float(k) for k in range(360, 501, 20))
TRUE_PXS = (398.0, 411.0, 385.0)
QUOTE = 400.0


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(OUT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def fixture():
    g = torch.Generator().manual_seed(7)
    log_p = (torch.log(torch.tensor(400.0)) + 0.05 * torch.randn(1000, len(EDAYS), generator=g).cumsum(1)).float()
    return log_p, log_p.exp()


def options_frame(pd):
    rows = [[pd.Timestamp(e), k, 1.0 + i, 2.0 + i] for e in EDAYS for i, k in enumerate(STRIKES)]
    return pd.DataFrame(rows, columns=["expiration", "strike", "bid", "ask"])


def main():
    import pandas as pd
    ref = os.path.join(_sibling("make_golden_gpcv").REF, "option_utils.py")
    spec = importlib.util.spec_from_file_location("ref_option_utils", ref)
    ou = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ou)
    log_p, pxs = fixture()
    true_pxs = torch.tensor(TRUE_PXS)
    df = ou.Pricer(pxs, options_frame(pd), EDAYS, true_pxs, QUOTE)
    out = dict(log_p=log_p.numpy(), pxs=pxs.numpy(), true_pxs=true_pxs.numpy(), strikes=np.array(STRIKES),
               quote=np.array(QUOTE), edays=np.array(EDAYS), columns=np.array(list(df.columns)),
               strike_col=df["Strike"].to_numpy(np.float64), expiry_col=np.array([str(t.date()) for t in df["Expiry"]]),
               voltron=df["Voltron"].to_numpy(np.float32), pct=df["Sample_Percentile"].to_numpy(np.float64),
               ret=df["Return"].to_numpy(np.float64), year=df["Year"].to_numpy(np.int64),
               ecdf=np.array([ou.ECDF(pxs[:, e], true_pxs[e]) for e in range(len(EDAYS))]))
    np.savez(os.path.join(OUT, "scoring.npz"), **out)
    print("scoring.npz:", {k: v.shape for k, v in out.items()}, "pandas", pd.__version__)


if __name__ == "__main__":
    main()
