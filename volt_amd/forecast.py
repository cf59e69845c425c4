"""Batched forecast drivers -- SURVEY 8(f) row 3: the sliding-window schedule and output format of
experiments/stocks/GenerateMultiMeanPreds.py:63-137 (and of the weather driver's volt/ewma branch,
experiments/weather/GPGenerator.py:20-112), with the reference's per-ticker / per-station Python ``for``
(ForecastGenerator.py:27-41, GPGenerator.py --stn_idx) replaced by one batched pass per window:

    window -> LearnGPCV for all tickers at once (batched variational fit, HIP ELBO step)          (:95-96)
           -> TrainVoltMagpieBatch (all tickers in one batched model, HIP MLL step)               (:99-103)
           -> TrainVolModelBatch + posterior samples of the vol forecasters (batched BM-GP, HIP factorisation)
           -> rollout engine for all tickers x paths in one launch                                (:105-107)
           -> torch.save(samples[S,H], "saved-outputs/<ticker>/<model>_<date>.pt")                (:128)

``vol_fn(train_x, prices [B,N+1]) -> vol [B,N]`` is the volatility-extraction stage: by default the reference's
LearnGPCV (train_utils.py:15-67) fitted for all tickers in one batch; ``realised_vol`` is a cheap non-reference
estimator kept for quick smoke runs.
"""
from __future__ import annotations

import os
import warnings

import torch

from . import rollout_engine
from .distributed import shard_range
from .rollout_utils import _linear_draw, _posterior_draw, _resolve_draw, _resolve_solver
from .safe import NanError, NotPSDError, NumericalWarning, _safe_draw, _safe_forms
from .train_utils import LearnGPCV, LearnGPCVMultitask, TrainVoltMagpieBatch, TrainVolModelBatch, TrainVolModelMultitask

_MODES = {"ewma": 0, "dewma": 1, "tewma": 2}
_STANDARD = ("constant", "loglinear", "linear")


def realised_vol(train_x, prices, span=20, floor=1e-3):
    """Annualised EWMA of |log-returns| -- a stand-in for the GPCV scale (NOT the reference's estimator).
    prices [B, N+1] -> vol [B, N]."""
    dt = (train_x[1] - train_x[0]).item()
    r = (prices[:, 1:].log() - prices[:, :-1].log()).abs() / dt ** 0.5
    from . import ops
    v = ops.ewma(r, span)[:, 1:]
    return v.clamp_min(floor)


def _standard_mean_prediction_linear(train_x, resid, m_te, vol, test_x, pred_vol, z, jitter=1e-4, max_blocks=4096,
                                     draw="factor"):
    """`_standard_mean_prediction` with solver="linear" (DESIGN 4.15): the train blocks of all B series are conditioned on by
    ONE volt_vk_forms_* launch (safe._safe_forms) instead of B x S factorisations, and nothing is N x N or N x H.  The stacked
    integrated path of rollout_utils.py:17-26 splits at the last train point: its train part U [B,N] keeps the full weight
    on point N-1 (the halved last weight sits on the last test point), and what the H appended points add on top of U[N-1] is
    the CumTrapz of [vol_{N-1}, pred_vol] less its first entry -- both from ops.cumtrapz in fp64.  The H x H predictive
    blocks of ``max_blocks`` (series, path) pairs at a time go through `_linear_draw`.
    ``draw="chain"``: ONE ops.vk_draw launch for all B series instead -- the test part of the integrated path
    is formed inside the kernel, so there is no ``tail`` / ``V_te`` tensor, no H x H block and no ``max_blocks`` loop: nothing
    beyond the inputs and the [B,S,H] result."""
    from . import ops
    B, S, H = pred_vol.shape
    N = train_x.numel()
    f64 = torch.float64
    x64 = torch.cat((train_x, test_x)).to(f64)
    U = ops.cumtrapz(torch.cat((vol, vol[:, -1:]), -1).to(f64), x64[:N + 1], square=True)[:, :N]      # [B,N]
    forms, _ = _safe_forms(U, resid.to(f64), jitter)                                                   # one launch, B series
    if draw == "chain":
        mean = forms[:, 1:2] + m_te.to(f64)                                                            # tau + m(x_t), [B,H]
        vlr = U[:, -1] - forms[:, 0]
        pv, zz = pred_vol.to(torch.float32), z.to(torch.float32)
        out, _ = _safe_draw(lambda j: ops.vk_draw(pv, vol[:, -1], vlr, x64[1] - x64[0], mean, zz, j), (pv, vlr, mean, zz), jitter)
        return out
    tail = ops.cumtrapz(torch.cat((vol[:, -1:, None].expand(B, S, 1), pred_vol), -1).to(f64), x64[:H + 1], square=True)
    V_last = U[:, -1]
    V_te = V_last[:, None, None] + (tail[..., 1:] - tail[..., :1])                                     # [B,S,H]
    out = torch.empty(B, S, H, device=train_x.device)
    step = max(1, max_blocks // S)
    for b0 in range(0, B, step):
        sl = slice(b0, min(B, b0 + step))
        nb = sl.stop - sl.start
        rep = lambda t: t[sl].repeat_interleave(S)
        draw = _linear_draw(rep(forms[:, 0]), rep(forms[:, 1]), rep(V_last), V_te[sl].reshape(nb * S, H),
                            m_te[sl, None, :, None].expand(nb, S, H, 1).reshape(nb * S, H, 1), z[sl].reshape(nb * S, H, 1),
                            jitter, None, 0.5, torch.float32)
        out[sl] = draw.reshape(nb, S, H)
    return out


def _standard_mean_prediction(model, train_x, log_y, vol, test_x, pred_vol, z, solver="dense", draw="factor"):
    """"VOLT + standard mean" (GenerateMultiMeanPreds.py:113-119): ONE joint draw over the whole horizon per path,
    GeneratePrediction(train_x, train_y, test_x, predvol, voltron) with predvol [S,H] -- rollout_utils.py:6-53 -- for
    every series of the batched model in turn (each is its own GP; the S systems of a series run batched on the
    device exactly as in the per-series function).  pred_vol, z [B,S,H] -> samples [B,S,H].
    ``solver="linear"``: `_standard_mean_prediction_linear`, which takes ``draw``."""
    B, S, H = pred_vol.shape
    N = train_x.numel()
    full_x = torch.cat((train_x, test_x))
    with torch.no_grad():
        m_tr = model.mean_module(train_x.unsqueeze(-1)).reshape(B, N)
        m_te = model.mean_module(test_x.unsqueeze(-1)).reshape(B, H)
    solver = _resolve_solver(solver)
    draw = _resolve_draw(draw, solver)
    if solver == "linear":
        return _standard_mean_prediction_linear(train_x, log_y - m_tr, m_te, vol, test_x, pred_vol, z, draw=draw)
    out = torch.empty(B, S, H, device=train_x.device)
    for b in range(B):
        full_vol = torch.cat((vol[b].unsqueeze(0).expand(S, N), pred_vol[b]), -1)        # :17-20
        draw = _posterior_draw(model.covar_module, full_x, full_vol, N, (log_y[b] - m_tr[b]).reshape(1, N, 1),
                               m_te[b].reshape(1, H, 1), z[b].reshape(S, H, 1), 1e-4)      # :26-53
        out[b] = draw.squeeze(-1)
    return out


def _check_vol_posterior(vol_posterior, vol_solver):
    """Before any window trains: the vol forecaster's constructor would raise the same, one GPCV fit later."""
    from .models._posterior import check_options
    check_options("vol_posterior", vol_solver, vol_posterior)


GPCV_OPTIONS = ("param", "K", "train_likelihood", "optimizer", "ng_step")      # what gpcv_options may carry to the GPCV fit
MULTITASK_GPCV = (False, True, "markov")               # True: the dense joint model; "markov": its Markov family


def _check_gpcv_options(gpcv_options, multitask_gpcv, gpcv_solver, nseries, vol_fn):
    """Before any window trains.  Returns the options as a dict."""
    opts = dict(gpcv_options or {})
    unknown = sorted(set(opts) - set(GPCV_OPTIONS))
    if unknown:
        raise ValueError(f"gpcv_options: unknown keys {unknown}; it takes {list(GPCV_OPTIONS)}")
    if multitask_gpcv not in MULTITASK_GPCV:
        raise ValueError(f"multitask_gpcv must be one of {list(MULTITASK_GPCV)}, got {multitask_gpcv!r}")
    if vol_fn is None and ("optimizer" in opts or "ng_step" in opts):     # (natural-gradient updates: FitGPCV)
        from .train_utils import _check_gpcv_optimizer
        _check_gpcv_optimizer(opts.get("optimizer", "adam"), opts.get("ng_step", 1.0), gpcv_solver, multitask=bool(multitask_gpcv))
        if multitask_gpcv:                               # (the joint fit has Adam only and takes neither key)
            opts.pop("optimizer", None)
            opts.pop("ng_step", None)
    if multitask_gpcv and vol_fn is None:
        from . import ops
        what = 'multitask_gpcv="markov" chooses the joint model\'s own solver' if multitask_gpcv == "markov" else \
            "multitask_gpcv=True runs the dense multi-task step"
        if gpcv_solver == "markov":
            raise ValueError(f'{what}: it does not combine with gpcv_solver="markov" (the Markov variational family of the '
                             'multi-task model is spelled multitask_gpcv="markov"; gpcv_solver is the single-task fit\'s)')
        if gpcv_solver == "linear":
            raise ValueError(f'{what}: it does not combine with gpcv_solver="linear" '
                             "(the multi-task model has no lazy Brownian prior)")
        if nseries > ops.GPCV_MT_T_MAX:
            raise ValueError(f"multitask_gpcv=True takes at most {ops.GPCV_MT_T_MAX} series per rank (got {nseries})")
    return opts


def _window_pass(train_x, test_x, train_y, nsample, mean, k, gpcv_iters, vol_iters, data_iters, theta, vol_fn, generator,
                 graph, vol_solver="dense", gpcv_solver="dense", data_solver="dense", multitask_vol=False,
                 predict_solver="dense", vol_posterior="solve", predict_draw="factor", multitask_gpcv=False,
                 gpcv_options=None, debug=None):
    """One window for the series in train_y [b, ntrain] (prices): GPCV -> data model -> vol forecasters -> rollouts,
    every stage for all b series at once.  Returns samples [b, S, H] on the device."""
    dev = train_y.device
    b, H = train_y.shape[0], test_x.numel()
    predict_solver = _resolve_solver(predict_solver)
    if vol_fn is None and multitask_gpcv:                # ONE joint model over the rank's series: the prior is factored once
        vol = LearnGPCVMultitask(train_x, train_y, train_iters=gpcv_iters, graph=graph,
                                 solver="markov" if multitask_gpcv == "markov" else "dense", **(gpcv_options or {}))
    elif vol_fn is None:
        vol = LearnGPCV(train_x, train_y, train_iters=gpcv_iters, graph=graph, solver=gpcv_solver,
                        **(gpcv_options or {}))                                          # all series at once
    else:
        vol = vol_fn(train_x, train_y)                                                   # [b, ntrain-1]
    # the shards are independent series and the ranks may run different numbers of fits (a failed window is redone series
    # by series on the rank that saw it): no collective in here
    model, lh, _ = TrainVoltMagpieBatch(train_x, train_y[:, 1:], vol, train_iters=data_iters, k=k, mean_func=mean,
                                        graph=graph, reduce_across_ranks=False, solver=data_solver)
    if multitask_vol:      # the reference's own vol forecaster of the batched models: ONE Kronecker GP over the b log-vol paths
        vmod, vlh = TrainVolModelMultitask(train_x, vol, train_iters=vol_iters, graph=graph, solver=vol_solver,
                                           vol_posterior=vol_posterior)
        vmod.eval()
        pred_vol = vmod(test_x).sample(torch.Size((nsample,))).exp().permute(2, 0, 1).contiguous().detach()   # [S,H,b] -> [b,S,H]
    else:
        vmod, vlh = TrainVolModelBatch(train_x, vol, train_iters=vol_iters, graph=graph, solver=vol_solver,
                                       vol_posterior=vol_posterior)
        vmod.eval()
        pred_vol = vmod(test_x).sample(torch.Size((nsample,))).exp().transpose(0, 1).contiguous().detach()   # [b,S,H]
    z = torch.randn(b, nsample, H, device=dev, generator=generator)
    latent = train_y.log().mean(-1) if theta is not None else None                       # rollout_utils.py:60-63
    if mean in _MODES:                                                                   # Rollouts, :110-112
        samples, info = rollout_engine.rollout_series(train_x, train_y[:, 1:].log(), vol.log(), test_x, pred_vol, z,
                                                      _MODES[mean], k, latent_mean=latent, theta=theta,
                                                      solve="chain" if predict_solver == "linear" else "factor")
        rollout_engine.report_info(info)                # raises where psd_safe_cholesky(pred_cov) would have (:46), warns on a jittered pivot
    else:                                                                                # VOLT + standard mean, :113-119
        samples = _standard_mean_prediction(model, train_x, train_y[:, 1:].log(), vol, test_x, pred_vol, z, predict_solver,
                                            predict_draw)
    if debug is not None:
        debug.update(vol=vol, pred_vol=pred_vol, z=z, model=model, train_y=train_y)
    return samples.detach()                                                              # .detach(): :118


def _window_summary(samples, series, last_day, spec):
    """Summary of one window's samples [B,S,H] on the device against the realised continuation series[:, e:e+H] (NaN where
    the series ends): scoring.summarize_paths, nothing comes to the host."""
    from . import scoring
    B, _, H = samples.shape
    truth = torch.full((B, H), float("nan"), device=samples.device)
    have = max(0, min(H, series.shape[1] - last_day))
    if have:
        truth[:, :have] = series[:, last_day:last_day + have].float()
    return scoring.summarize_paths(samples, q=spec.q, truth=truth, strikes=spec.strikes, exp=spec.exp)


def _forecast_windows(names, series, end_idxs, ntrain, train_x, test_x, nsample, mean, k, gpcv_iters, vol_iters,
                      data_iters, theta, vol_fn, generator, save, path_fn, debug=None, graph=None, summary=None,
                      keep_samples=True, vol_solver="dense", gpcv_solver="dense", data_solver="dense", multitask_vol=False,
                      predict_solver="dense", vol_posterior="solve", predict_draw="factor", multitask_gpcv=False,
                      gpcv_options=None):
    """One batched pass per window (series [B,T] prices; the window ending at index e trains on series[:, e-ntrain:e]).
    A numerical failure anywhere in the batched pass (NotPSDError / NanError after the jitter ladders) must not take the
    other series down with it: the window is then redone one series at a time, and a series that still fails gets NaN
    samples and a "Failed:" line -- what the reference's per-ticker try / except does
    (experiments/stocks/GenerateMultiMeanPreds.py:185-198).
    ``debug`` (a dict) receives the last window's intermediates (vol, pred_vol, z, model) for tests.
    ``summary`` (a scoring.SummarySpec): every window is also summarised on the device (_window_summary) and
    ``<sample file stem>_summary.pt`` saved next to the sample files; the return is then (last samples, [PathSummary per
    window]).  ``keep_samples=False`` (with a summary) skips the copy of the samples to the host and the sample files and
    returns (None, summaries)."""
    if not keep_samples and summary is None:
        raise ValueError("keep_samples=False leaves nothing to return without summary=")
    B = series.shape[0]
    gpcv_options = _check_gpcv_options(gpcv_options, multitask_gpcv, gpcv_solver, B, vol_fn)
    summaries = []
    H = test_x.numel()
    args = (nsample, mean, k, gpcv_iters, vol_iters, data_iters, theta, vol_fn, generator, graph, vol_solver, gpcv_solver,
            data_solver, multitask_vol, predict_solver, vol_posterior, predict_draw, multitask_gpcv, gpcv_options)
    last = None
    for last_day in end_idxs:
        train_y = series[:, last_day - ntrain:last_day].float()                          # [B, ntrain] prices
        try:
            samples = _window_pass(train_x, test_x, train_y, *args, debug=debug)
        except (NotPSDError, NanError) as err:
            warnings.warn(f"window ending at {last_day}: the batched pass failed ({err}); redoing it series by series",
                          NumericalWarning)
            samples = torch.full((B, nsample, H), float("nan"), device=series.device)
            for b in range(B):
                try:
                    samples[b] = _window_pass(train_x, test_x, train_y[b:b + 1], *args)[0]
                except (NotPSDError, NanError):
                    print("Failed: ", names[b], mean, k)
        if summary is not None:
            summaries.append(_window_summary(samples, series, last_day, summary))
        if keep_samples:
            last = samples.cpu()
        if save:
            host = summaries[-1].cpu() if summary is not None else None
            for b, name in enumerate(names):
                path = path_fn(name, last_day)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                if keep_samples:
                    torch.save(last[b], path)
                if host is not None:
                    torch.save({f: v[b] for f, v in host.fields().items()}, os.path.splitext(path)[0] + "_summary.pt")
    if summary is None:
        return last
    return last, summaries


def GenerateStockPredictionsBatch(tickers, closes, dates=None, forecast_horizon=20, train_iters=400, nsample=1000,
                                  ntrain=400, mean="ewma", save=False, k=300, ntimes=-1, vol_fn=None,
                                  vol_iters=None, par_dir="./saved-outputs/", generator=None, debug=None, graph=None,
                                  summary=None, keep_samples=True, vol_solver="dense", gpcv_solver="dense",
                                  data_solver="dense", multitask_vol=False, predict_solver="dense",
                                  vol_posterior="solve", predict_draw="factor", multitask_gpcv=False, gpcv_options=None):
    """closes [B, T] prices for B tickers on a common calendar (device tensor).  Same window schedule,
    model name and file layout as GenerateStockPredictions (GenerateMultiMeanPreds.py:69-83,128); ``mean`` in
    ewma / dewma / tewma takes the Rollouts branch (:110-112), constant / loglinear / linear the "VOLT + standard
    mean" branch (:113-119: one multi-point GeneratePrediction per path).
    Under torch.distributed each rank takes a contiguous shard of the tickers.  Returns the samples of
    the last window, [B_local, nsample, forecast_horizon] on the CPU.
    ``summary=scoring.SummarySpec(...)``: each window's paths are summarised on the device against the realised
    continuation and the return is (samples, [PathSummary per window]); with ``keep_samples=False`` the samples never
    come to the host (no sample files either) and the first element is None.
    ``vol_solver="linear"``: the vol forecaster's fit and posterior on the linear-time Brownian-motion solver
    (TrainVolModelBatch(solver=...), csrc/bm.hip); the default "dense" changes nothing.
    ``gpcv_solver="markov"``: the GPCV stage in O(N) with the Markov variational family (csrc/gpcv_markov.hip).
    ``gpcv_solver="linear"``: the GPCV stage's ELBO step in O(N^2) (LearnGPCV(solver=...), csrc/gpcv_bm.hip); independent of
    ``vol_solver``, ignored with a ``vol_fn``, and "dense" changes nothing.
    ``data_solver="linear"``: the data model's fit on the linear-time step over each series' integrated vol path
    (TrainVoltMagpieBatch(solver=...), csrc/bm.hip) -- no N x N matrix per series; independent of the other two, and "dense"
    changes nothing.
    ``multitask_vol=True``: the vol forecaster is ONE MultitaskBMGP over the tickers' log-vol paths (TrainVolModelMultitask;
    T <= 64 tickers per rank) instead of a BM-GP per ticker, so the vol paths of a draw are correlated across tickers; with
    ``vol_solver="linear"`` it runs on the linear-time Kronecker step.
    ``predict_solver="linear"``: the forecast conditions on each series' train block through the O(N) chain (volt_vk_forms_*,
    DESIGN 4.15) -- solve="chain" on the Rollouts branch, one launch for all tickers on the standard-mean branch -- instead
    of filling and factoring an N x N block per series (per path, on the standard-mean branch); independent of the other
    three, and "dense" changes nothing.
    ``vol_posterior="sweep"`` (with ``vol_solver="linear"``): the vol forecaster's posterior from ONE forward sweep per window
    (BMGP / MultitaskBMGP(posterior="sweep"), volt_bm_post_*) instead of a chain solve on K_t* [T,N,H]; the
    default "solve" changes nothing.  ``vol_posterior="chain"``: the same sweep, and the vol paths are drawn in O(S H) without the
    H x H covariance (ops.markov_draw).
    ``predict_draw="chain"`` (with ``predict_solver="linear"``): the joint draw of the standard-mean branch from ONE ops.vk_draw
    launch for all tickers, with no H x H block per path; the Rollouts branch has its own recursion and is not
    changed by it; the default "factor" changes nothing.
    ``multitask_gpcv=True``: the window's vol paths come from ONE LearnGPCVMultitask call over the rank's series (the joint
    Kronecker variational GP: one prior factorisation for all of them, T <= 64 per rank) instead of the batched single-task
    LearnGPCV; not with ``gpcv_solver="linear"`` or ``"markov"``.  The series-by-series redo after a failed window then runs
    T = 1.  ``multitask_gpcv="markov"``: the same joint model with the Markov variational family under the level-jitter
    Brownian prior (LearnGPCVMultitask(solver="markov"), csrc/gpcv_mt_markov.hip): O(N T), no N x N array.
    ``gpcv_options``: a dict with keys out of ``param``, ``K``, ``train_likelihood``, ``optimizer``, ``ng_step`` (the last two:
    ``{"optimizer": "natgrad"}`` with ``gpcv_solver="markov"`` fits q by natural-gradient updates, FitGPCV),
    forwarded to whichever GPCV fit runs (FitGPCV / FitGPCVMultitask); unknown keys raise.  Both are ignored with a ``vol_fn``; the defaults change nothing."""
    _check_vol_posterior(vol_posterior, vol_solver)
    _resolve_draw(predict_draw, predict_solver)
    if mean not in _MODES and mean not in _STANDARD:
        raise ValueError(f"unknown mean {mean!r}: one of {sorted(_MODES) + list(_STANDARD)}")
    dev = closes.device
    lo, hi = shard_range(len(tickers))
    tickers, closes = list(tickers)[lo:hi], closes[lo:hi]
    T = closes.shape[1]
    if ntimes == -1:
        end_idxs = torch.arange(ntrain, T)
    else:
        end_idxs = torch.arange(ntrain, T, int((T - ntrain) / ntimes))
    dt = 1. / 252
    model_name = "volt_" + mean + str(k) + "_"
    vol_iters = train_iters if vol_iters is None else vol_iters
    train_x = torch.arange(ntrain - 1, device=dev) * dt                                  # :89
    test_x = torch.arange(forecast_horizon, device=dev) * dt + train_x[-1] + train_x[1]  # :90

    def path_fn(tckr, last_day):
        date = str(last_day) if dates is None else str(dates[last_day])
        return os.path.join(par_dir, tckr, model_name + date + ".pt")                    # :128
    return _forecast_windows(tickers, closes, end_idxs.tolist(), ntrain, train_x, test_x, nsample, mean, k,
                             train_iters, vol_iters, train_iters, None, vol_fn, generator, save, path_fn, debug, graph,
                             summary, keep_samples, vol_solver, gpcv_solver, data_solver, multitask_vol, predict_solver,
                             vol_posterior, predict_draw, multitask_gpcv, gpcv_options)


def GenerateWindPredictionsBatch(stations, data, forecast_horizon=100, ntrain=400, n_test_times=10, nsample=1000, k=400,
                                 theta=0.01, gpcv_iters=200, vol_iters=500, data_iters=0, save=False, vol_fn=None,
                                 par_dir="./saved-outputs/", generator=None, graph=None, summary=None, keep_samples=True,
                                 vol_solver="dense", gpcv_solver="dense", data_solver="dense", multitask_vol=False,
                                 predict_solver="dense", vol_posterior="solve", predict_draw="factor", multitask_gpcv=False,
                                 gpcv_options=None):
    """The ``--kernel volt --mean ewma`` branch of experiments/weather/GPGenerator.py:20-112 for B stations at once:
    data [B,T] wind speeds (missing = -99 -> 0, then +1 as at :47,55), dt = 1/365 (:38-41), the schedule of test
    windows of :33-34, GPCV 200 / vol model 500 / data model 0 iterations (:64-67,89-92), EWMA(k=400) mean and
    mean-reverting rollouts with theta = 0.01 (:96-102), files ``stn<idx>/volt_ema<k>_theta<theta>_<last_day>.pt``
    (:103-106).  Stations shard across ranks like tickers.  Returns the last window's samples [B_local,S,H] (CPU).
    ``summary`` / ``keep_samples`` / ``vol_solver`` / ``gpcv_solver`` / ``data_solver`` / ``multitask_vol`` / ``predict_solver`` / ``vol_posterior`` / ``predict_draw`` / ``multitask_gpcv`` / ``gpcv_options``: as for GenerateStockPredictionsBatch (the truth is the shifted series,
    data + 1)."""
    _check_vol_posterior(vol_posterior, vol_solver)
    _resolve_draw(predict_draw, predict_solver)
    dev = data.device
    lo, hi = shard_range(len(stations))
    stations, data = list(stations)[lo:hi], data[lo:hi].float()
    data = torch.where(data == -99.0, torch.zeros_like(data), data) + 1                  # :47,55
    ntime = data.shape[1]
    step = int((ntime - forecast_horizon - ntrain) / n_test_times)
    end_idxs = torch.arange(ntrain, ntime - forecast_horizon, step).tolist()            # :33-34
    train_x = torch.arange(ntrain - 1, device=dev).float() / 365                         # :38
    test_x = torch.arange(ntrain, ntrain + forecast_horizon, device=dev).float() / 365   # :41 (absolute day index, as written)

    def path_fn(stn, last_day):
        return os.path.join(par_dir, "stn" + str(stn), "volt_ema" + str(k) + "_theta" + str(theta) + "_" +
                            str(last_day) + ".pt")
    return _forecast_windows(stations, data, end_idxs, ntrain, train_x, test_x, nsample, "ewma", k, gpcv_iters,
                             vol_iters, data_iters, theta, vol_fn, generator, save, path_fn, None, graph, summary,
                             keep_samples, vol_solver, gpcv_solver, data_solver, multitask_vol, predict_solver, vol_posterior,
                             predict_draw, multitask_gpcv, gpcv_options)
